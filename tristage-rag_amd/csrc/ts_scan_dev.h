// Device code shared by the scan kernels (ts_scan.hip: dense / filter scans; ts_fused.hip: the
// one-launch search).  Not part of the public ABI.
#pragma once
#include "ts_common.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifndef SCAN_THREADS
#define SCAN_THREADS 512
#endif
#define SCAN_WAVES (SCAN_THREADS / 64)

__device__ __forceinline__ u32x4 stream_load(const u32x4* p) {
#ifndef TS_PLAIN_LOADS  // non-temporal: the corpus is read once per batch, keep it out of L2/MALL
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}

template <int DT>
__device__ __forceinline__ void mma_group(f32x16& acc, const u32x4& a,
                                          const u32x4& b) {
#if defined(TS_TUNING) && defined(DBG_NO_MFMA)  // ablation builds only: keep the operands live, skip the matrix op
  acc[0] += __uint_as_float((a[0] ^ b[0]) & 0x007fffffu);
  acc[1] += __uint_as_float((a[1] ^ b[1]) & 0x007fffffu);
  acc[2] += __uint_as_float((a[2] ^ b[2]) & 0x007fffffu);
  acc[3] += __uint_as_float((a[3] ^ b[3]) & 0x007fffffu);
  return;
#endif
  if constexpr (DT == TS_F16) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(
        __builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), acc, 0, 0, 0);
  } else if constexpr (DT == TS_BF16) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
        __builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), acc, 0, 0, 0);
  } else {
    const f32x4 af = __builtin_bit_cast(f32x4, a);
    const f32x4 bf = __builtin_bit_cast(f32x4, b);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0], bf[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1], bf[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[2], bf[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[3], bf[3], acc, 0, 0, 0);
  }
}

// row inside the 32-row block held by accumulator register r of this lane
// (C/D map of the 32x32 MFMA shapes: col = lane & 31, row below)
__device__ __forceinline__ int acc_row(int r, int lane) {
  return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

__device__ __forceinline__ float acc_max(const f32x16& a) {
  float m0 = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
  float m1 = fmaxf(fmaxf(a[4], a[5]), fmaxf(a[6], a[7]));
  float m2 = fmaxf(fmaxf(a[8], a[9]), fmaxf(a[10], a[11]));
  float m3 = fmaxf(fmaxf(a[12], a[13]), fmaxf(a[14], a[15]));
  return fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
}

template <int QH>
__device__ __forceinline__ void epilogue_dense(const ScanParams& p,
                                               const f32x16 (&acc)[QH],
                                               int64_t w, int64_t blk,
                                               int lane) {
  const int j = lane & 31;
  const int64_t row_base = blk * TS_ROWS_PER_BLOCK;
#pragma unroll
  for (int hq = 0; hq < QH; ++hq) {
    const int q = hq * 32 + j;
    if (q < p.nq) {
      float* dst = p.dense + (int64_t)q * p.dense_ld + w * TS_ROWS_PER_BLOCK;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int i0 = 8 * r4 + 4 * (lane >> 5);
        float4 v;
        v.x = (row_base + i0 + 0 < p.ntotal) ? acc[hq][4 * r4 + 0] : -3.402823466e38f;
        v.y = (row_base + i0 + 1 < p.ntotal) ? acc[hq][4 * r4 + 1] : -3.402823466e38f;
        v.z = (row_base + i0 + 2 < p.ntotal) ? acc[hq][4 * r4 + 2] : -3.402823466e38f;
        v.w = (row_base + i0 + 3 < p.ntotal) ? acc[hq][4 * r4 + 3] : -3.402823466e38f;
        *reinterpret_cast<float4*>(dst + i0) = v;
      }
    }
  }
}

// Survivors of the threshold test are parked in LDS and written to the
// per-query candidate lists once, by the whole workgroup, when it has finished
// streaming.  (Appending from the hot loop with returning global atomics costs
// 27 % of the kernel at 10M x 768: each append stalls its wave for microseconds
// behind the HBM stream — measured, DESIGN.md "candidate staging".)
#define STAGE_CAP 2048
template <int CAP>
struct StageLdsT {
  static constexpr uint32_t kCap = CAP;
  uint32_t cnt;
  uint32_t tau_flag;        // ts_fused.hip: wave 0 has published this launch's thresholds in tauv[]
  uint32_t arrived;         // ts_fused.hip: waves of this workgroup that have delivered their sample
  uint32_t pad[1];
  float tauv[TS_MAX_Q];     // ts_fused.hip: the thresholds, once tau_flag is set
  uint32_t qcnt[TS_MAX_Q];
  uint32_t qbase[TS_MAX_Q];
  uint32_t qoff[TS_MAX_Q];
  float score[CAP];
  int32_t id[CAP];
  uint8_t q[CAP];
};
typedef StageLdsT<STAGE_CAP> StageLds;

// MASKED (scan_kernel over a masked WALK, filtered searches): on the rare path a survivor of query hq*32 + (lane & 31)
// also needs its bit in mw[hq], that query's allow word of this row block (bit i = row 32*blk + i).  The
// common path is the same ballot: the mask costs nothing there.
template <int QH, class SL, bool MASKED = false>
__device__ __forceinline__ void epilogue_filter(const ScanParams& p, SL* st,
                                                const f32x16 (&acc)[QH],
                                                const float (&tau)[QH],
                                                int64_t blk, int lane, const uint32_t* mw = nullptr) {
  bool hit = false;
#pragma unroll
  for (int hq = 0; hq < QH; ++hq) hit |= (acc_max(acc[hq]) >= tau[hq]);
  if (__builtin_amdgcn_ballot_w64(hit) == 0ull) return;  // the common case
  // Rare path: some lane holds at least one surviving score.
  const int64_t row_base = blk * TS_ROWS_PER_BLOCK;
#pragma unroll
  for (int hq = 0; hq < QH; ++hq) {
    const int q = hq * 32 + (lane & 31);
    uint32_t mask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      bool ok = (acc[hq][r] >= tau[hq]) &&
                (row_base + acc_row(r, lane) < p.ntotal);
      if constexpr (MASKED) ok = ok && ((mw[hq] >> acc_row(r, lane)) & 1u);
      mask |= ok ? (1u << r) : 0u;
    }
    if (mask) {
      uint32_t slot = atomicAdd(&st->cnt, (uint32_t)__builtin_popcount(mask));  // LDS
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (mask & (1u << r)) {
          const int32_t id = (int32_t)(row_base + acc_row(r, lane));
          if (slot < SL::kCap) {
            st->score[slot] = acc[hq][r];
            st->id[slot] = id;
            st->q[slot] = (uint8_t)q;
          } else {
            // staging area full (heavily clustered hits): append directly
            const uint32_t g = atomicAdd(&p.cand_cnt[q], 1u);
            if (g < p.cand_cap) {
              p.cand_score[(size_t)q * p.cand_cap + g] = acc[hq][r];
              p.cand_id[(size_t)q * p.cand_cap + g] = id;
            }
          }
          ++slot;
        }
      }
    }
  }
}

// Workgroup-wide: move the staged survivors to the per-query lists.  One global
// atomic per (workgroup, query) reserves the slots.
template <class SL>
__device__ __forceinline__ void flush_stage(const ScanParams& p, SL* st, int tid) {
  __syncthreads();
  const uint32_t n = st->cnt < SL::kCap ? st->cnt : SL::kCap;
  if (n == 0) return;  // uniform: cnt is final after the barrier
  if (tid < TS_MAX_Q) { st->qcnt[tid] = 0; st->qoff[tid] = 0; }
  __syncthreads();
  for (uint32_t e = tid; e < n; e += SCAN_THREADS) atomicAdd(&st->qcnt[st->q[e]], 1u);
  __syncthreads();
  if (tid < TS_MAX_Q && st->qcnt[tid] > 0)
    st->qbase[tid] = atomicAdd(&p.cand_cnt[tid], st->qcnt[tid]);
  __syncthreads();
  for (uint32_t e = tid; e < n; e += SCAN_THREADS) {
    const uint32_t q = st->q[e];
    const uint32_t slot = st->qbase[q] + atomicAdd(&st->qoff[q], 1u);
    if (slot < p.cand_cap) {
      p.cand_score[(size_t)q * p.cand_cap + slot] = st->score[e];
      p.cand_id[(size_t)q * p.cand_cap + slot] = st->id[e];
    }
  }
}

// ------------------------------------------------------------------ the ring scan
// Every per-pass stage-1 scan is one instantiation of scan_kernel<QH, MODE, OP, WALK> below: persistent waves, a
// TS_RING-deep register ring of non-temporal 1 KiB loads that stays full across row-block boundaries, the query image
// resident in LDS, a sched_barrier per step.  OP says how ring slots meet the image, WALK which row block a work
// item is; a masked WALK also keeps each lane's allow word of the current row block.
//
// OP:
//   Stage                    the survivor staging type
//   image_kib<QH>(kg)        1 KiB units of the query image
//   step<QH>(acc, ring, i, ql, g)   ring slot i (k group g of the row block) against the image
// WALK:
//   Params, kMasked
//   wave(tid)                the wave in the workgroup (masked walks: through readfirstlane, their loads are scalar)
//   nwork(p)                 work items of the launch
//   block(p, w), idle(p)     a work item's row block; the block whose address an idle wave forms and never loads
//   row_groups(p)            k groups between the starts of consecutive row blocks (p.kg groups of each are scanned: the
//                            prefix walks of ts_scan_prefix.hip scan fewer than a row block holds)
//   mask_init / mask_fetch / mask_advance (kMasked): the allow words of the first block; the request for the next
//                            block's, just before the tail's loads; next -> current, after the epilogue.  The state,
//                            per query half hq, is arrays of the kernel body:
//                              mrow[hq]   the lane's row of allow words
//                              mstep[hq]  words per row block in it (0 for an unmasked query: it keeps reading word 0)
//                              mor[hq]    ORed into every word read (all ones for an unmasked query)
//                              mw[hq]     the current block's allow word, what the epilogue tests
//                              mwn[hq]    the next block's word as fetched (mor not yet applied)
//   kBiased                  a masked walk that also carries the per-row bias of the current row block (WalkLiveBias,
//                            ts_scan_bias.hip): bias_init / bias_fetch / bias_advance beside the mask hooks, and an
//                            epilogue of its own that tests and stages score + bias
// OP::kScaled (optional; OpFp4 of ts_scan_fp4.hip, which needs TS_RING == 4): ring slots carry block-scaled elements
// whose scale bytes lie in units just before the row block's ring units.  scale_fetch(blk_ptr, kg, sc) requests a
// lane's scale bytes of a row block: for the first block just before its first ring loads, for the next one beside the
// mask words just before the tail's loads, unpredicated, so it is complete before that block's first slot is (vmcnt
// retires in order).  scale_word(sc, g0) picks the bytes of ring turn g0 .. g0 + 3 and step_scaled takes them.

template <class OP, class = void> struct ScanOpScaled { static constexpr bool value = false; };
template <class OP> struct ScanOpScaled<OP, decltype((void)OP::kScaled)> { static constexpr bool value = OP::kScaled; };

// 16-bit storage and the exact-f32 MFMA: one slot, one MFMA group per query half
template <int DT>
struct Op16 {
  typedef StageLds Stage;
  template <int QH> static __device__ __forceinline__ int image_kib(int kg) { return kg * QH; }
  template <int QH>
  static __device__ __forceinline__ void step(f32x16 (&acc)[QH], const u32x4 (&ring)[TS_RING], int i, const u32x4* ql, int g) {
#pragma unroll
    for (int hq = 0; hq < QH; ++hq) {
      const u32x4 b = ql[(size_t)g * (QH * 64) + hq * 64];   // (hq as a constant offset: one address per k group)
      mma_group<DT>(acc[hq], ring[i], b);
    }
  }
};

#if defined(TS_TUNING) && defined(DBG_NO_LDS)  // ablation builds only (wrong results): the B operand is the next ring slot
template <int DT>
struct OpNoLds : Op16<DT> {
  template <int QH>
  static __device__ __forceinline__ void step(f32x16 (&acc)[QH], const u32x4 (&ring)[TS_RING], int i, const u32x4*, int) {
#pragma unroll
    for (int hq = 0; hq < QH; ++hq) mma_group<DT>(acc[hq], ring[i], ring[(i + 1) % TS_RING]);
  }
};
#endif

typedef const uint32_t __attribute__((address_space(4)))* ts_sgpr_u32p;   // scalar loads: lgkmcnt, not vmcnt
typedef const int32_t __attribute__((address_space(4)))* ts_sgpr_i32p;

// work item w is row block blk0 + w * blk_stride
struct WalkStrided {
  typedef ScanParams Params;
  static constexpr bool kMasked = false;
  static constexpr bool kBiased = false;
  static __device__ __forceinline__ int wave(int tid) { return tid >> 6; }
  static __device__ __forceinline__ int64_t nwork(const Params& p) { return p.nwork; }
  static __device__ __forceinline__ int64_t block(const Params& p, int64_t i) { return p.blk0 + i * p.blk_stride; }
  static __device__ __forceinline__ int64_t idle(const Params& p) { return p.blk0; }
  static __device__ __forceinline__ int row_groups(const Params& p) { return p.kg; }
};

// Filtered searches: work item w is row block p.live[w], w < *p.nlive.  Both are read with scalar loads (constant
// address space, wave-uniform index): they count against lgkmcnt, not vmcnt, so fetching the next block's index never
// waits for the corpus ring.  Each lane's allow word of the NEXT block is requested just before that block's first
// ring loads, unpredicated (an unmasked query reads word 0 of mask 0 and ORs in all ones), and is complete by the
// time the block's epilogue reads it: vmcnt retires in order, and the ring loads issued after it have been consumed
// by then.
struct WalkLive {
  typedef MaskedScanParams Params;
  static constexpr bool kMasked = true;
  static constexpr bool kBiased = false;
  static __device__ __forceinline__ int wave(int tid) { return __builtin_amdgcn_readfirstlane(tid >> 6); }
  static __device__ __forceinline__ int64_t nwork(const Params& p) { return (int64_t)*(ts_sgpr_u32p)p.nlive; }
  static __device__ __forceinline__ int64_t block(const Params& p, int64_t i) {
    return (int64_t)((ts_sgpr_i32p)p.live)[i];
  }
  static __device__ __forceinline__ int64_t idle(const Params&) { return 0; }
  static __device__ __forceinline__ int row_groups(const Params& p) { return p.kg; }
  template <int QH>
  static __device__ __forceinline__ void mask_init(const Params& p, int64_t blk, int lane, const uint32_t* (&mrow)[QH],
                                                   int64_t (&mstep)[QH], uint32_t (&mor)[QH], uint32_t (&mw)[QH]) {
#pragma unroll
    for (int hq = 0; hq < QH; ++hq) {
      const int32_t qm = p.qmask[hq * 32 + (lane & 31)];
      mrow[hq] = p.allow_bits + (qm < 0 ? 0 : (int64_t)qm * p.allow_words);
      mstep[hq] = qm < 0 ? 0 : 1;
      mor[hq] = qm < 0 ? ~0u : 0u;
      mw[hq] = mrow[hq][blk * mstep[hq]] | mor[hq];
    }
  }
  template <int QH>
  static __device__ __forceinline__ void mask_fetch(const Params&, int64_t blkn, const uint32_t* const (&mrow)[QH],
                                                    const int64_t (&mstep)[QH], uint32_t (&mwn)[QH]) {
#pragma unroll
    for (int hq = 0; hq < QH; ++hq) mwn[hq] = mrow[hq][blkn * mstep[hq]];
  }
  template <int QH>
  static __device__ __forceinline__ void mask_advance(const uint32_t (&mor)[QH], const uint32_t (&mwn)[QH],
                                                      uint32_t (&mw)[QH]) {
#pragma unroll
    for (int hq = 0; hq < QH; ++hq) mw[hq] = mwn[hq] | mor[hq];
  }
};

// Q image global(L2) -> LDS, once per workgroup.  8 independent loads in flight per thread (a one-load-at-a-time copy
// of the 96 KiB image costs ~18 us of serial L2 latency per workgroup)
__device__ __forceinline__ void scan_load_image(u32x4* qlds, const uint4* qimg, int units, int tid) {
  const u32x4* src = reinterpret_cast<const u32x4*>(qimg);
  for (int i0 = tid; i0 < units; i0 += 8 * SCAN_THREADS) {
    u32x4 t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = i0 + j * SCAN_THREADS;
      t[j] = (i < units) ? src[i] : u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = i0 + j * SCAN_THREADS;
      if (i < units) qlds[i] = t[j];
    }
  }
}

// One persistent wave streams work items gw, gw+W, gw+2W, ... (W = waves in the grid).  No barrier after the prologue.
// The template is the __global__ function itself: a body inlined into named kernels allocates registers differently.
template <int QH, int MODE, class OP, class WALK>
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(typename WALK::Params p) {
  typedef typename OP::Stage Stage;
  constexpr bool MASKED = WALK::kMasked && MODE == SCAN_FILTER;
  constexpr bool BIASED = MASKED && WALK::kBiased;
  constexpr bool SCALED = ScanOpScaled<OP>::value;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* qlds = reinterpret_cast<u32x4*>(smem);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = WALK::wave(tid);
  const int kg = p.kg;

  // ---- the first corpus loads go out before anything else, so the HBM round trip
  // overlaps the Q-image copy below
  const int64_t nwaves = (int64_t)gridDim.x * SCAN_WAVES;
  int64_t w = (int64_t)blockIdx.x * SCAN_WAVES + wave;
  const int64_t nwork = WALK::nwork(p);
  const bool active = w < nwork;  // (waves without work still join the final flush)
  const u32x4* base = reinterpret_cast<const u32x4*>(p.corpus) + lane;
  const size_t blk_units = (size_t)WALK::row_groups(p) * 64;
  int64_t blk = active ? WALK::block(p, w) : WALK::idle(p);
  const u32x4* cur = base + (size_t)blk * blk_units;
  u32x4 ring[TS_RING];
  // the scale bytes of a scaled op: the current row block's, the next one's, the ring turn's.  The first block's are
  // requested ahead of its ring loads, as every later block's are: a request younger than the ring would make the
  // first use of them a wait for the whole ring, in every row block (the waits of a loop are those of its worst entry)
  u32x4 sc[2], scn[2];
  uint32_t sw = 0;
  if (active) {
    if constexpr (SCALED) OP::scale_fetch(cur, kg, sc);
#pragma unroll
    for (int i = 0; i < TS_RING; ++i) ring[i] = stream_load(cur + (size_t)i * 64);
  }

  // ---- prologue: Q image global(L2) -> LDS, once per workgroup
  const int image_kib = OP::template image_kib<QH>(kg);
  scan_load_image(qlds, p.qimg, image_kib * 64, tid);
  Stage* st = reinterpret_cast<Stage*>(smem + (size_t)image_kib * 1024);
  if constexpr (MODE == SCAN_FILTER) {
    if (tid == 0) st->cnt = 0;
  }
  __syncthreads();

  if (active) {
    float tau[QH];
    if constexpr (MODE == SCAN_FILTER) {
#pragma unroll
      for (int hq = 0; hq < QH; ++hq) tau[hq] = p.tau[hq * 32 + (lane & 31)];
    }
    // the allow-word state of a masked walk (plain arrays: held in a struct they change the register allocation)
    const uint32_t* mrow[QH];
    int64_t mstep[QH];
    uint32_t mor[QH], mw[QH];
    if constexpr (MASKED) WALK::template mask_init<QH>(p, blk, lane, mrow, mstep, mor, mw);
    // the bias state of a biased walk: bcur[r >> 2][r & 3] is the bias of the row of accumulator register r, bmax
    // the largest of the lane's 16
    f32x4 bcur[4];
    float bmax;
    if constexpr (BIASED) WALK::bias_init(p, blk, lane, bcur, bmax);

    const u32x4* ql = qlds + lane;

    while (true) {
      const int64_t wn = w + nwaves;
      const bool has_next = wn < nwork;
      const int64_t blkn = has_next ? WALK::block(p, wn) : blk;
      const u32x4* nxt = base + (size_t)blkn * blk_units;

      f32x16 acc[QH];
#pragma unroll
      for (int hq = 0; hq < QH; ++hq)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[hq][r] = 0.f;

      // main part: prefetch stays inside the current row block
      int g0 = 0;
      for (; g0 < kg - TS_RING; g0 += TS_RING) {
        if constexpr (SCALED) sw = OP::scale_word(sc, g0);
#pragma unroll
        for (int i = 0; i < TS_RING; ++i) {
          if constexpr (SCALED) OP::template step_scaled<QH>(acc, ring, i, ql, g0 + i, sw);
          else OP::template step<QH>(acc, ring, i, ql, g0 + i);
          // refill the slot just consumed; the barrier keeps the compiler from
          // clustering the ring's loads (which would drain vmcnt to 0 mid-loop)
          ring[i] = stream_load(cur + (size_t)(g0 + i + TS_RING) * 64);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // tail: (masked: the next block's allow words, then) the ring is refilled from the start of the wave's next
      // row block
      uint32_t mwn[QH];
      if constexpr (MASKED) WALK::template mask_fetch<QH>(p, blkn, mrow, mstep, mwn);
      f32x4 bnxt[4];
      if constexpr (BIASED) WALK::bias_fetch(p, blkn, lane, bnxt);
      if constexpr (SCALED) {
        sw = OP::scale_word(sc, g0);
        OP::scale_fetch(nxt, kg, scn);
      }
#pragma unroll
      for (int i = 0; i < TS_RING; ++i) {
        if constexpr (SCALED) OP::template step_scaled<QH>(acc, ring, i, ql, g0 + i, sw);
        else OP::template step<QH>(acc, ring, i, ql, g0 + i);
        ring[i] = stream_load(nxt + (size_t)i * 64);
        __builtin_amdgcn_sched_barrier(0);
      }

      if constexpr (MODE == SCAN_DENSE)
        epilogue_dense<QH>(p, acc, w, blk, lane);
      else if constexpr (BIASED)
        WALK::template epilogue<QH, Stage>(p, st, acc, tau, blk, lane, mw, bcur, bmax);
      else if constexpr (MASKED)
        epilogue_filter<QH, Stage, true>(p, st, acc, tau, blk, lane, mw);
      else
        epilogue_filter<QH>(p, st, acc, tau, blk, lane);

      if (!has_next) break;
      w = wn;
      blk = blkn;
      cur = nxt;
      if constexpr (MASKED) WALK::template mask_advance<QH>(mor, mwn, mw);
      if constexpr (BIASED) WALK::bias_advance(bnxt, bcur, bmax);
      if constexpr (SCALED) { sc[0] = scn[0]; sc[1] = scn[1]; }
    }
  }  // active
  if constexpr (MODE == SCAN_FILTER) flush_stage(p, st, tid);
}

// workgroups of a scan over nwork work items: one per SCAN_WAVES items, at most cap, at least one
static inline int ts_scan_grid(int64_t nwork, int64_t cap) {
  const int64_t want = (nwork + SCAN_WAVES - 1) / SCAN_WAVES;
  const int grid = (int)(want < cap ? want : cap);
  return grid < 1 ? 1 : grid;
}

// The launch rule of scan_kernel, in plain host arithmetic (no HIP call: tests/test_scan_launch_host.py runs it
// without a device).  kib: KiB of the query image per query half (32 queries); stage_bytes: sizeof(OP::Stage).
//   mode   a masked (or biased) walk is filter-only, whatever the caller asks for
//   LDS    the image, and behind it the survivor staging of a filter scan
//   admit  a pass of qh halves is taken where its filter form fits the LDS (each file's check, with its own text)
//   grid   the filter scan is HBM-bound with one 8-wave workgroup per CU (more waves measured slower: 16 waves/CU
//          -1.5 %); the short dense scans (sample, small corpora) are latency-bound and take a second workgroup per CU
//          when LDS allows
struct TsScanGeom {
  int mode;
  size_t lds;
  int grid;
};
static inline size_t ts_scan_lds(int kib, int qh, int mode, size_t stage_bytes) {
  return (size_t)kib * qh * 1024 + (mode == SCAN_FILTER ? stage_bytes : 0);
}
static inline bool ts_scan_admits(int kib, int qh, size_t stage_bytes) {
  return ts_scan_lds(kib, qh, SCAN_FILTER, stage_bytes) <= TS_LDS_BYTES;
}
static inline TsScanGeom ts_scan_geom(int kib, int qh, int mode, bool masked, size_t stage_bytes, int64_t nwork,
                                      int num_cus) {
  if (masked) mode = SCAN_FILTER;
  const size_t lds = ts_scan_lds(kib, qh, mode, stage_bytes);
  const int wg_per_cu = (mode == SCAN_DENSE && 2 * lds <= TS_LDS_BYTES) ? 2 : 1;
  return {mode, lds, ts_scan_grid(nwork, (int64_t)num_cus * wg_per_cu)};
}

template <int QH, int MODE, class OP, class WALK>
static int launch_scan_ring(const typename WALK::Params& p, size_t lds, int grid, hipStream_t stream) {
  auto kern = scan_kernel<QH, MODE, OP, WALK>;
  static TsDeviceOnce lds_attr;  // per instantiation, per device (ts_common.h)
  TS_CHECK(ts_allow_max_lds(lds_attr, reinterpret_cast<const void*>(kern)));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(SCAN_THREADS), lds, stream, p);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// Every launch of scan_kernel: run-time (qh, mode) -> <QH, MODE>, with the geometry above.  A masked walk has no dense
// instantiation, and its p.nwork is every row block (the live count is only known on the device; waves past it leave
// at once).  The caller has made its admission check.
template <class OP, class WALK>
static int launch_scan(int mode, int qh, int kib, const typename WALK::Params& p, int num_cus, hipStream_t stream) {
  const TsScanGeom g = ts_scan_geom(kib, qh, mode, WALK::kMasked, sizeof(typename OP::Stage), p.nwork, num_cus);
  if constexpr (!WALK::kMasked) {
    if (g.mode == SCAN_DENSE)
      return qh == 1 ? launch_scan_ring<1, SCAN_DENSE, OP, WALK>(p, g.lds, g.grid, stream)
                     : launch_scan_ring<2, SCAN_DENSE, OP, WALK>(p, g.lds, g.grid, stream);
  }
  return qh == 1 ? launch_scan_ring<1, SCAN_FILTER, OP, WALK>(p, g.lds, g.grid, stream)
                 : launch_scan_ring<2, SCAN_FILTER, OP, WALK>(p, g.lds, g.grid, stream);
}

// ------------------------------------------------------------------ layout
template <typename T> struct ElemIO;
template <> struct ElemIO<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
};
template <> struct ElemIO<_Float16> {
  static __device__ __forceinline__ float ld(const _Float16* p) { return (float)*p; }
};
template <> struct ElemIO<__bf16> {
  static __device__ __forceinline__ float ld(const __bf16* p) {
    uint32_t u = (uint32_t)(*reinterpret_cast<const uint16_t*>(p)) << 16;
    return __builtin_bit_cast(float, u);
  }
};

// 8 consecutive elements as floats (p 16-byte aligned for 16-bit types, 32 for float rows
// whose dim is a multiple of 8)
template <typename T> __device__ __forceinline__ void ld8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void ld8<float>(const float* p, float (&v)[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <> __device__ __forceinline__ void ld8<_Float16>(const _Float16* p, float (&v)[8]) {
  const h8 x = *reinterpret_cast<const h8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)x[i];
}
template <> __device__ __forceinline__ void ld8<__bf16>(const __bf16* p, float (&v)[8]) {
  const uint4 x = *reinterpret_cast<const uint4*>(p);
  v[0] = __uint_as_float(x.x << 16); v[1] = __uint_as_float(x.x & 0xffff0000u);
  v[2] = __uint_as_float(x.y << 16); v[3] = __uint_as_float(x.y & 0xffff0000u);
  v[4] = __uint_as_float(x.z << 16); v[5] = __uint_as_float(x.z & 0xffff0000u);
  v[6] = __uint_as_float(x.w << 16); v[7] = __uint_as_float(x.w & 0xffff0000u);
}

__device__ __forceinline__ uint16_t f32_to_storage16(float f, int dt) {
  if (dt == TS_F16) {
    _Float16 h = (_Float16)f;
    return __builtin_bit_cast(uint16_t, h);
  }
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(uint16_t, b);
}

// k index of element e (0..epl-1) of lane half h in group g
__device__ __forceinline__ int frag_k(int dt, int g, int h, int e) {
  // f32: two consecutive units (g even, g odd) hold 8 consecutive k of a lane's row — k = 16(g/2) + 8h + 4(g&1) + e —
  // so that a pair of units is the A operand of one 16-wide k step of the bf16x3 split scan (ts_scan_f32s.hip);
  // the exact-f32 MFMA path does not care about the order (the query image uses the same map)
  return (dt == TS_F32) ? (16 * (g >> 1) + 8 * h + 4 * (g & 1) + e) : (16 * g + 8 * h + e);
}

// What every relayout kernel walks: one wave per (row block, unit) of the row blocks that rows [row0, row0 + n) touch,
// `units` units of each, four waves per workgroup.  vec: the 8-element loads of ld8 may be used (rows of whole
// 8-element groups from a base aligned to 16 bytes, 32 for float rows).
struct TsRelayoutGeom {
  int64_t blk_first, nwave;
  unsigned blocks;
  int vec;
};
static inline int ts_relayout_geom(int dim, int units, const void* rows, size_t elem_bytes, int64_t row0, int64_t n,
                                   TsRelayoutGeom& g) {
  g.blk_first = row0 / TS_ROWS_PER_BLOCK;
  const int64_t blk_last = (row0 + n - 1) / TS_ROWS_PER_BLOCK;
  g.nwave = (blk_last - g.blk_first + 1) * units;
  const int64_t blocks = (g.nwave + 3) / 4;
  if (blocks > 0x7fffffffLL) {
    ts_set_error("add: too many rows in one call");
    return TS_ERR_INVALID;
  }
  g.blocks = (unsigned)blocks;
  g.vec = (int)((dim % 8) == 0 && (reinterpret_cast<uintptr_t>(rows) % (4 * elem_bytes >= 16 ? 32 : 16)) == 0);
  return TS_OK;
}

// workgroups of a reconstruct kernel: a thread per (row, unit, lane half) of n rows
static inline int ts_reconstruct_blocks(int64_t n, int units, unsigned& blocks) {
  const int64_t b = (n * units * 2 + 255) / 256;
  if (b > 0x7fffffffLL) {
    ts_set_error("reconstruct: range too large");
    return TS_ERR_INVALID;
  }
  blocks = (unsigned)b;
  return TS_OK;
}

