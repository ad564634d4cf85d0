// Query-stationary coalesced passes (scan_qstat_kernel<DT, NWIN>): the wide pass turned round.
//
// scan_wide_kernel keeps the corpus in registers and re-gathers a window of every group's query image from L2 into LDS
// for every window of every row block: 48 KiB of image beside 64 KiB of corpus per window at G = 6.  Here the queries
// stay put and the corpus moves through LDS:
//   * one 8-wave workgroup per CU; wave g owns group g of the pass (G <= 8, a run-time argument) and holds the group's
//     whole image in registers, u32x4 q[kg] (192 VGPRs at padded d = 768): loaded once, in the prologue;
//   * the corpus goes from HBM into a ring of 8 KiB windows in LDS by LDS-DMA, each byte once per CU, shared by the
//     eight waves; wave w requests k group w of every window (one 1 KiB piece).  The tiled corpus is in A-fragment
//     order, so a piece lands lane-linear and a ds_read_b128 at lane * 16 is the operand stream_load delivers;
//   * per 32-row block a wave runs kg MFMAs (A from LDS, a few slots ahead; B = q[i]; one accumulator, the first MFMA on
//     a literal zero), the ballot epilogue of epilogue_multi for its one group, and meets the others at ONE barrier.
// The MFMA chain of a score is scan_kernel's (A the corpus, B the query, k groups in order, zeroed start), so its bits do
// not depend on which kernel scored it.
//
// Ring and counted waits.  The ring is `depth` = qstat_depth(NWIN) windows (ts_scan_qstat_ring.h: a compile-time
// constant, 15 at both widths; the host sizes the LDS from the same function), counted across row blocks (workgroup b walks row blocks
// b, b + grid, ...; window W of its walk is k window W % NWIN of its row block W / NWIN and lives in slot W % depth).
// The prologue requests windows 0 .. depth-1 and drains them.  Step s then
//     computes block s out of its NWIN slots,
//     waits vmcnt(depth - 2 * NWIN): requests are retired in order, a wave has issued windows 0 .. depth + s*NWIN - 1, so
//       at most that many outstanding means windows .. (s + 2) * NWIN - 1, block s + 1's, have landed (its own pieces),
//     meets the others (lgkmcnt(0) + s_barrier: the DMA stays in flight; every wave's reads of block s are retired),
//     requests windows depth + s*NWIN .. + NWIN - 1 into the slots block s freed.
// So a window is read one barrier after the wait that retired it, and restaged one barrier after its last read was
// waited for; depth - NWIN windows are in flight while a block computes.  Past the end of the walk the requests read the
// first 8 KiB of group 0's image instead (in bounds, L2-resident, never consumed), as scan_wide_kernel's refills do, so
// every step issues NWIN requests and the one count holds in the prologue, in walks shorter than the ring and in the tail.
//
// The step's tail is straight-line.  Everything the requests need is known at compile time (which of two row blocks
// and which k window request kw of a step belongs to, the wait's count) or moves by a constant per step (two source
// pointers, NWIN slot offsets: scalar additions, QstatRingState).  The walk is split: a main loop over the steps whose
// NWIN requests all lie inside the walk (s + 3 < steps at both widths) issues them in ONE statement with no live / dead
// select, M0 saved and restored once; a tail loop over the last three steps, and the prologue, choose per request
// between its source and the dead address.  tests/qstat_ring.hip walks this arithmetic on the host;
// tests/test_qstat_tail_build.py counts the compiled main loop.
#include "ts_scan_dev.h"
#include "ts_linear_dev.h"   // fs_barrier
#include "ts_scan_qstat_ring.h"
#include <algorithm>
#include <type_traits>

struct StageQstatHdr {
  uint32_t cnt;
  uint32_t pad[3];
  uint32_t qcnt[TS_MAX_WIDE_GROUPS * 32];
  uint32_t qbase[TS_MAX_WIDE_GROUPS * 32];
  uint32_t qoff[TS_MAX_WIDE_GROUPS * 32];
  // followed by float score[stage_cap], uint32_t key[stage_cap]
};
static_assert(SCAN_WAVES == 8 && TS_MAX_WIDE_GROUPS == SCAN_WAVES, "one group per wave");
static_assert(TS_RING == SCAN_WAVES, "a window is one piece per wave");
#define TS_QSTAT_GROUPS 8
#define TS_QSTAT_MAX_STEPS (1 << 16)   // survivor key: (step << 16) | (row in block << 8) | query of the pass
#define TS_QSTAT_MIN_STAGE 4096u       // entries (TS_WIDE_MIN_STAGE): about 3 k survivors per workgroup and pass of 8
#define TS_QSTAT_AHEAD 4               // A operands read ahead of their MFMA (6 and 8 measured the same)

// a[g] for a wave-uniform run-time g, without a dynamically indexed kernel argument (that would go through scratch)
template <class T>
__device__ __forceinline__ T qstat_pick(const T (&a)[TS_MAX_WIDE_GROUPS], int g) {
  T r = a[0];
#pragma unroll
  for (int i = 1; i < TS_MAX_WIDE_GROUPS; ++i) r = (g == i) ? a[i] : r;
  return r;
}

template <int N, int I = 0, class F>
__device__ __forceinline__ void qstat_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    qstat_static_for<N, I + 1>(f);
  }
}

// One request of the ring: 1 KiB (this wave's piece of a window) from src + voff (per lane) to the LDS address dst.
// s_nop 4: a VMEM instruction may read an SGPR only 5 wait states after a VALU wrote it.  s_nop 0: an LDS-DMA may read
// M0 one wait state after an SALU wrote it.  M0 is saved and restored: the compiler reserves it.
// nt: the corpus is read once per pass (measured against the default policy: 3.93-3.94 against 3.97-4.01 ms)
__device__ __forceinline__ void qstat_request(uint32_t dst, uint32_t voff, const unsigned char* src) {
  uint32_t keep;
  __asm__ volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                   "global_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(voff), "s"(src), "s"(dst) : "memory");
}
#define TS_QSTAT_REQ(d, v, s) "s_mov_b32 m0, " d "\n\ts_nop 0\n\tglobal_load_lds_dwordx4 " v ", " s " nt\n\t"

// The ring of a wave: its request state (QstatRingState, ts_scan_qstat_ring.h) lives in scalar registers and moves by
// additions only; voff[k] is the per-lane offset of k window k inside a row block.
template <int NWIN>
struct QstatWalk {
  using R = QstatRing<NWIN>;
  using State = QstatRingState<NWIN, const unsigned char*>;
  State st;
  uint32_t ring_lds, loff;
  uint32_t voff[NWIN];
  const unsigned char* dead;

  // `first`: this wave's piece of k window 0 of the walk's block 0.  Requests windows 0 .. DEPTH-1; a walk shorter than
  // the ring reads `dead` for the rest.
  __device__ __forceinline__ void prologue(uint32_t smem_lds, int wave, int lane, const unsigned char* first,
                                           int64_t step_bytes, const unsigned char* dead_, int steps) {
    ring_lds = smem_lds + (uint32_t)wave * 1024u;
    loff = (uint32_t)lane * 16;
    dead = dead_;
#pragma unroll
    for (int k = 0; k < NWIN; ++k) voff[k] = loff + (uint32_t)k * TS_QSTAT_WINDOW;
    qstat_static_for<R::DEPTH>([&](auto w) {
      constexpr int W = decltype(w)::value;
      const bool live = State::prologue_live(W, steps);
      qstat_request(ring_lds + (uint32_t)W * TS_QSTAT_WINDOW, live ? voff[W % NWIN] : loff,
                    live ? State::prologue_block(first, step_bytes, W) : dead);
    });
    st.start(first, step_bytes);
  }

  // LDS byte offset of this lane's 16 bytes of window kw's k group 0, for the block the step computes
  __device__ __forceinline__ uint32_t read_off(int kw) const { return st.slot[kw] + loff; }

  // the NWIN requests of a step whose requests all lie inside the walk: one statement, M0 saved and restored once
  __device__ __forceinline__ void requests_main() const {
    uint32_t keep;
    uint32_t d[NWIN], v[NWIN];
#pragma unroll
    for (int kw = 0; kw < NWIN; ++kw) {
      d[kw] = ring_lds + st.slot[kw];
      v[kw] = voff[R::req_kwin(kw)];
    }
    if constexpr (NWIN == 6) {
      static_assert(NWIN != 6 || R::SPLIT == 3, "the statement below: request kw takes src0 iff kw < SPLIT");
      __asm__ volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\t"
                       TS_QSTAT_REQ("%1", "%7", "%13") TS_QSTAT_REQ("%2", "%8", "%13") TS_QSTAT_REQ("%3", "%9", "%13")
                       TS_QSTAT_REQ("%4", "%10", "%14") TS_QSTAT_REQ("%5", "%11", "%14") TS_QSTAT_REQ("%6", "%12", "%14")
                       "s_mov_b32 m0, %0"
                       : "=&s"(keep)
                       : "s"(d[0]), "s"(d[1]), "s"(d[2]), "s"(d[3]), "s"(d[4]), "s"(d[5]),
                         "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "s"(st.src0), "s"(st.src1)
                       : "memory");
    } else {
      static_assert(NWIN == 6 || (NWIN == 5 && R::SPLIT == 5), "the statement below");
      __asm__ volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\t"
                       TS_QSTAT_REQ("%1", "%6", "%11") TS_QSTAT_REQ("%2", "%7", "%11") TS_QSTAT_REQ("%3", "%8", "%11")
                       TS_QSTAT_REQ("%4", "%9", "%11") TS_QSTAT_REQ("%5", "%10", "%11")
                       "s_mov_b32 m0, %0"
                       : "=&s"(keep)
                       : "s"(d[0]), "s"(d[1]), "s"(d[2]), "s"(d[3]), "s"(d[4]),
                         "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "s"(st.src0)
                       : "memory");
    }
  }

  // the NWIN requests of one of the walk's last steps: each chooses between its source and `dead`
  __device__ __forceinline__ void requests_tail(int s, int steps) const {
    qstat_static_for<NWIN>([&](auto k) {
      constexpr int KW = decltype(k)::value;
      const bool live = State::req_live(KW, s, steps);
      qstat_request(ring_lds + st.slot[KW], live ? voff[R::req_kwin(KW)] : loff, live ? st.req_block(KW) : dead);
    });
  }

  // to the next step
  __device__ __forceinline__ void advance() { st.advance(); }

  // at most LEAD requests outstanding: this wave's pieces of the next block have landed
  __device__ __forceinline__ static void wait_next_block() { __builtin_amdgcn_s_waitcnt(0x3F70 | R::LEAD); }
};

#if defined(TS_TUNING) && defined(QSTAT_TRACE)   // diagnostic builds only: per-wave phase sums of the walk, tools/trace_qstat.py
// Row (workgroup * SCAN_WAVES + wave) of the last scan_qstat_kernel launch: 100 MHz ticks summed over the wave's steps
// for 0 the step's start to its first MFMA (offsets, the first operand reads), 1 first to last MFMA, 2 the survivor
// test, 3 the counted wait, 4 the barrier, 5 the step's requests; then 6 the walk's ticks, 7 its s_memtime counts,
// 8 the wave's steps.  A stamp is a scalar memory read, so it waits lgkmcnt(0) itself: none inside the MFMA slots.
#define QSTAT_TRACE_ROW 10
__device__ uint32_t qstat_trace_buf[256 * SCAN_WAVES * QSTAT_TRACE_ROW];
extern "C" int ts_debug_qstat_trace(uint32_t* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(qstat_trace_buf), sizeof(qstat_trace_buf)) == hipSuccess ? 0 : -2;
}
struct QstatTrace {
  uint32_t sum[6], c0, t0, last;
  __device__ __forceinline__ void begin() {
    for (int k = 0; k < 6; ++k) sum[k] = 0;
    c0 = (uint32_t)__builtin_amdgcn_s_memtime();
    t0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
    last = t0;
  }
  __device__ __forceinline__ void stamp(int k) {
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t now = (uint32_t)__builtin_amdgcn_s_memrealtime();
    sum[k] += now - last;
    last = now;
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void end(int lane, int wave, int steps) {
    const uint32_t ticks = (uint32_t)__builtin_amdgcn_s_memrealtime() - t0;
    const uint32_t counts = (uint32_t)__builtin_amdgcn_s_memtime() - c0;
    if (lane == 0 && blockIdx.x < 256) {
      uint32_t* row = qstat_trace_buf + ((size_t)blockIdx.x * SCAN_WAVES + wave) * QSTAT_TRACE_ROW;
      for (int k = 0; k < 6; ++k) row[k] = sum[k];
      row[6] = ticks;
      row[7] = counts;
      row[8] = (uint32_t)steps;
    }
  }
};
#else
struct QstatTrace {
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void stamp(int) {}
  __device__ __forceinline__ void end(int, int, int) {}
};
#endif

// One block's scores for one group: KG MFMAs, A from the block's NWIN slots (rolling, TS_QSTAT_AHEAD operands ahead),
// B = q[i], one accumulator, the first MFMA on a literal zero.
template <int DT, int NWIN>
__device__ __forceinline__ f32x16 qstat_block(const unsigned char* smem, const QstatWalk<NWIN>& ring,
                                              const u32x4 (&q)[NWIN * TS_RING], QstatTrace& trace) {
  constexpr int KG = NWIN * TS_RING;
  // the block's windows: LDS byte offsets of this lane's 16 bytes of each window's k group 0
  uint32_t woff[NWIN];
#pragma unroll
  for (int kw = 0; kw < NWIN; ++kw) woff[kw] = ring.read_off(kw);
  auto a_read = [&](auto i) {
    constexpr int I = decltype(i)::value;
    return *reinterpret_cast<const u32x4*>(smem + woff[I / TS_RING] + (I % TS_RING) * 1024);
  };
  u32x4 a[TS_QSTAT_AHEAD];
  qstat_static_for<TS_QSTAT_AHEAD>([&](auto i) { a[decltype(i)::value] = a_read(i); });
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;   // (folds into the first MFMA's C operand: a literal 0)
  trace.stamp(0);
  // rolling A operands: a register set is re-read with the operand TS_QSTAT_AHEAD slots on as soon as its MFMA has
  // issued (lgkmcnt(TS_QSTAT_AHEAD - 1) before each MFMA, counted by the compiler).  The sched_barriers pin that
  // order: left alone the scheduler puts each read right in front of its MFMA.
  __builtin_amdgcn_sched_barrier(0);
  qstat_static_for<KG>([&](auto i) {
    constexpr int I = decltype(i)::value;
    mma_group<DT>(acc, a[I % TS_QSTAT_AHEAD], q[I]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (I + TS_QSTAT_AHEAD < KG) {
      a[I % TS_QSTAT_AHEAD] = a_read(std::integral_constant<int, I + TS_QSTAT_AHEAD>{});
      __builtin_amdgcn_sched_barrier(0);
    }
  });
  trace.stamp(1);
  return acc;
}

template <int DT, int NWIN>
__global__ __launch_bounds__(SCAN_THREADS) void scan_qstat_kernel(WideScanParams p, int G) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using R = QstatRing<NWIN>;
  constexpr int KG = NWIN * TS_RING;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool owner = wave < G;   // a wave without a group still requests its pieces and meets the barriers
  const int grid = (int)gridDim.x;
  // this workgroup's walk: row blocks blockIdx.x + s * grid, s < steps (the launcher keeps grid <= nwork)
  const int steps = (int)((p.nwork - 1 - (int64_t)blockIdx.x) / grid) + 1;

  StageQstatHdr* st = reinterpret_cast<StageQstatHdr*>(smem + R::RING_BYTES);
  float* sscore = reinterpret_cast<float*>(st + 1);
  uint32_t* skey = reinterpret_cast<uint32_t*>(sscore + p.stage_cap);
  if (tid == 0) st->cnt = 0;

  // ---- the ring's requests: this wave's piece (k group `wave` of the window) of the next windows of the walk
  const int64_t blk_step = (int64_t)grid * p.blk_stride;   // row blocks from one step's block to the next
  QstatWalk<NWIN> ring;
  ring.prologue((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem, wave, lane,
                reinterpret_cast<const unsigned char*>(p.corpus) +
                    qstat_first_byte(p.blk0, blockIdx.x, p.blk_stride, R::BLOCK_BYTES) + (size_t)wave * 1024,
                qstat_step_bytes(grid, p.blk_stride, R::BLOCK_BYTES),
                reinterpret_cast<const unsigned char*>(p.gimg[0]) + (size_t)wave * 1024, steps);

  // ---- the wave's group: its image into registers, its thresholds.  These loads follow the ring's requests, so the
  // compiler's own counts for them (it does not see the requests) only wait for more than it thinks.
  const int gqh = qstat_pick(p.gqh, wave), ghalf = qstat_pick(p.ghalf, wave);
  u32x4 q[KG];
  float tau = __builtin_huge_valf();
  if (owner) {
    const u32x4* img = reinterpret_cast<const u32x4*>(qstat_pick(p.gimg, wave)) + (size_t)ghalf * 64 + lane;
#pragma unroll
    for (int i = 0; i < KG; ++i) q[i] = img[(size_t)i * gqh * 64];
    tau = qstat_pick(p.gtau, wave)[lane & 31];
  } else {
#pragma unroll
    for (int i = 0; i < KG; ++i) q[i] = u32x4{0u, 0u, 0u, 0u};
  }
  // (loaded here, not sunk into the walk, where a compiler-counted load would wait for the ring's requests too)
#pragma unroll
  for (int i = 0; i < KG; ++i) __asm__ volatile("" : "+v"(q[i]));
  __asm__ volatile("" : "+v"(tau));
  __builtin_amdgcn_s_waitcnt(0x3F70);   // vmcnt(0): the first depth windows have landed (this wave's pieces)
  fs_barrier();

  int64_t row_base = (p.blk0 + (int64_t)blockIdx.x * p.blk_stride) * TS_ROWS_PER_BLOCK;   // of the step's block
  const int64_t row_step = blk_step * TS_ROWS_PER_BLOCK;

  // epilogue_multi's ballot epilogue for one group, block `sb` of the walk: the group's maximum against tau, then one
  // ballot per accumulator register, the staging code under the execution mask of the lanes that hit
  auto survivors = [&](const f32x16& acc, int sb) __attribute__((always_inline)) {
    if (__builtin_amdgcn_ballot_w64(acc_max(acc) >= tau) == 0ull) return;   // the common case
    const bool partial = row_base + TS_ROWS_PER_BLOCK > p.ntotal;   // the corpus's last row block, wave-uniform
    const int rows_left = (int)(p.ntotal - row_base);
    const uint32_t keyhi = (uint32_t)sb << 16;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool ok = acc[r] >= tau;
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(ok) == 0ull, 1)) continue;
      if (!ok) continue;
      int ln = lane;
      __asm__ volatile("" : "+v"(ln));
      const int row = acc_row(r, ln), j = ln & 31;
      if (!partial || row < rows_left) {
        const uint32_t slot = atomicAdd(&st->cnt, 1u);  // LDS
        if (slot < p.stage_cap) {
          sscore[slot] = acc[r];
          skey[slot] = keyhi | ((uint32_t)row << 8) | (uint32_t)(wave * 32 + j);
        } else {
          // staging area full: append directly
          const uint32_t g = atomicAdd(&qstat_pick(p.gcnt, wave)[j], 1u);
          if (g < p.cand_cap) {
            qstat_pick(p.gscore, wave)[(size_t)j * p.cand_cap + g] = acc[r];
            qstat_pick(p.gid, wave)[(size_t)j * p.cand_cap + g] = (int32_t)(row_base + row);
          }
        }
      }
    }
  };

  // a step up to its requests: block s out of its slots, then this wave's pieces of block s + 1 have landed and every
  // wave is done reading block s
  QstatTrace trace;
  trace.begin();
  auto step = [&](int s) __attribute__((always_inline)) {
    if (owner) {
      survivors(qstat_block<DT, NWIN>(smem, ring, q, trace), s);
      trace.stamp(2);
    }
    ring.wait_next_block();
    trace.stamp(3);
    fs_barrier();
    trace.stamp(4);
  };
  // the steps whose refills all lie inside the walk, then the last few, whose refills may read `dead`
  const int nmain = R::main_steps(steps);
  int s = 0;
  for (; s < nmain; ++s) {
    step(s);
    ring.requests_main();
    ring.advance();
    row_base += row_step;
    trace.stamp(5);
  }
  for (; s < steps; ++s) {
    step(s);
    ring.requests_tail(s, steps);
    ring.advance();
    row_base += row_step;
    trace.stamp(5);
  }
  trace.end(lane, wave, steps);
  // the tail's requests (never consumed) are still landing in the ring
  __builtin_amdgcn_s_waitcnt(0x3F70);   // vmcnt(0)

  // ---- flush (scan_wide_kernel's): one global atomic per (workgroup, query) reserves the slots
  __syncthreads();
  const uint32_t n = st->cnt < p.stage_cap ? st->cnt : p.stage_cap;
  if (n == 0) return;  // uniform: cnt is final after the barrier
  for (int t = tid; t < TS_QSTAT_GROUPS * 32; t += SCAN_THREADS) { st->qcnt[t] = 0; st->qoff[t] = 0; }
  __syncthreads();
  for (uint32_t e = tid; e < n; e += SCAN_THREADS) atomicAdd(&st->qcnt[skey[e] & 255u], 1u);
  __syncthreads();
  for (int t = tid; t < TS_QSTAT_GROUPS * 32; t += SCAN_THREADS)
    if (st->qcnt[t] > 0) st->qbase[t] = atomicAdd(qstat_pick(p.gcnt, t >> 5) + (t & 31), st->qcnt[t]);
  __syncthreads();
  for (uint32_t e = tid; e < n; e += SCAN_THREADS) {
    const uint32_t key = skey[e];
    const uint32_t qi = key & 255u;
    const uint32_t slot = st->qbase[qi] + atomicAdd(&st->qoff[qi], 1u);
    if (slot < p.cand_cap) {
      const int g = (int)(qi >> 5);
      const size_t at = (size_t)(qi & 31u) * p.cand_cap + slot;
      const int64_t wi = (int64_t)blockIdx.x + (int64_t)(key >> 16) * grid;
      qstat_pick(p.gscore, g)[at] = sscore[e];
      qstat_pick(p.gid, g)[at] = (int32_t)((p.blk0 + wi * p.blk_stride) * TS_ROWS_PER_BLOCK + ((key >> 8) & 31u));
    }
  }
}

// Sample mode: the dense scan of a strided sample of the corpus for the groups of several batches at once, in place of
// one scan_kernel dense launch per batch (coalesced passes, DESIGN.md 4.2c "pass prologue").  A sibling of
// scan_qstat_kernel on the same ring (QstatWalk) and the same block (qstat_block: the rolling A operands and the
// one-accumulator MFMA chain, so a score has scan_kernel's bits).  What differs: no thresholds, no staging, no flush;
// the LDS is the ring only, and a wave's accumulator goes to its group's lines of its batch's sample buffer as
// epilogue_dense writes them.  Those stores share vmcnt with the ring's requests and are younger than the requests a
// counted wait is for, so the wait only waits for more.
template <int DT, int NWIN>
__global__ __launch_bounds__(SCAN_THREADS) void scan_qstat_sample_kernel(QstatSampleParams p, int G) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using R = QstatRing<NWIN>;
  constexpr int KG = NWIN * TS_RING;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool owner = wave < G;
  const int grid = (int)gridDim.x;
  const int steps = (int)((p.nwork - 1 - (int64_t)blockIdx.x) / grid) + 1;

  const int64_t blk_step = (int64_t)grid * p.blk_stride;
  QstatWalk<NWIN> ring;
  ring.prologue((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem, wave, lane,
                reinterpret_cast<const unsigned char*>(p.corpus) +
                    qstat_first_byte(p.blk0, blockIdx.x, p.blk_stride, R::BLOCK_BYTES) + (size_t)wave * 1024,
                qstat_step_bytes(grid, p.blk_stride, R::BLOCK_BYTES),
                reinterpret_cast<const unsigned char*>(p.gimg[0]) + (size_t)wave * 1024, steps);

  // ---- the wave's group: its image into registers; its valid queries and this lane's line of the sample buffer
  const int gqh = qstat_pick(p.gqh, wave), ghalf = qstat_pick(p.ghalf, wave);
  u32x4 q[KG];
  int snq = 0;
  float* sdst = nullptr;   // this lane's line, at the step's work item
  if (owner) {
    const u32x4* img = reinterpret_cast<const u32x4*>(qstat_pick(p.gimg, wave)) + (size_t)ghalf * 64 + lane;
#pragma unroll
    for (int i = 0; i < KG; ++i) q[i] = img[(size_t)i * gqh * 64];
    snq = qstat_pick(p.gnq, wave);
    sdst = qstat_pick(p.gdense, wave) + (int64_t)(ghalf * 32 + (lane & 31)) * p.dense_ld +
           (int64_t)blockIdx.x * TS_ROWS_PER_BLOCK;
  } else {
#pragma unroll
    for (int i = 0; i < KG; ++i) q[i] = u32x4{0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int i = 0; i < KG; ++i) __asm__ volatile("" : "+v"(q[i]));
  __builtin_amdgcn_s_waitcnt(0x3F70);   // vmcnt(0): the first depth windows have landed (this wave's pieces)
  fs_barrier();

  int64_t row_base = (p.blk0 + (int64_t)blockIdx.x * p.blk_stride) * TS_ROWS_PER_BLOCK;   // of the step's block
  const int64_t row_step = blk_step * TS_ROWS_PER_BLOCK;
  const int64_t dst_step = (int64_t)grid * TS_ROWS_PER_BLOCK;   // work item blockIdx.x + s * grid

  auto step = [&]() __attribute__((always_inline)) {
    if (owner) {
      QstatTrace none;   // (the stamps are scan_qstat_kernel's)
      const f32x16 acc = qstat_block<DT, NWIN>(smem, ring, q, none);
      // epilogue_dense for one group: rows past the corpus's end get -FLT_MAX
      if ((lane & 31) < snq) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int i0 = 8 * r4 + 4 * (lane >> 5);
          float4 v;
          v.x = (row_base + i0 + 0 < p.ntotal) ? acc[4 * r4 + 0] : -3.402823466e38f;
          v.y = (row_base + i0 + 1 < p.ntotal) ? acc[4 * r4 + 1] : -3.402823466e38f;
          v.z = (row_base + i0 + 2 < p.ntotal) ? acc[4 * r4 + 2] : -3.402823466e38f;
          v.w = (row_base + i0 + 3 < p.ntotal) ? acc[4 * r4 + 3] : -3.402823466e38f;
          *reinterpret_cast<float4*>(sdst + i0) = v;
        }
      }
    }
    // this wave's pieces of block s + 1 have landed; every wave is done reading block s
    ring.wait_next_block();
    fs_barrier();
  };
  const int nmain = R::main_steps(steps);
  int s = 0;
  for (; s < nmain; ++s) {
    step();
    ring.requests_main();
    ring.advance();
    row_base += row_step;
    sdst += dst_step;
  }
  for (; s < steps; ++s) {
    step();
    ring.requests_tail(s, steps);
    ring.advance();
    row_base += row_step;
    sdst += dst_step;
  }
  // the tail's requests (never consumed) are still landing in the ring
  __builtin_amdgcn_s_waitcnt(0x3F70);   // vmcnt(0)
}

// ---- host
static int qstat_nwin(const TsLayout& L) {
  if (L.dtype != TS_F16 && L.dtype != TS_BF16) return 0;
  const int nwin = L.kg / TS_RING;
  return (L.kg % TS_RING == 0 && (nwin == 5 || nwin == 6)) ? nwin : 0;   // padded d = 640 and 768
}

// windows of the ring (ts_scan_qstat_ring.h: the kernels take the same function of NWIN)
static int qstat_depth(const TsLayout& L) { return qstat_depth(qstat_nwin(L)); }

int ts_scan_qstat_groups(const TsLayout& L) {
  return qstat_nwin(L) > 0 && ts_scan_qstat_stage_cap(L) > 0 ? TS_QSTAT_GROUPS : 0;
}

uint32_t ts_scan_qstat_stage_cap(const TsLayout& L) {
  if (qstat_nwin(L) == 0) return 0;
  const size_t fixed = (size_t)qstat_depth(L) * TS_QSTAT_WINDOW + sizeof(StageQstatHdr);
  if (fixed + 8 * (size_t)TS_QSTAT_MIN_STAGE > TS_LDS_BYTES) return 0;
  return (uint32_t)((TS_LDS_BYTES - fixed) / 8);
}

bool ts_scan_qstat_fits(int64_t nblk, int num_cus) {
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(nblk, num_cus));
  return (nblk + grid - 1) / grid <= TS_QSTAT_MAX_STEPS;
}

template <int DT, int NWIN>
static int qstat_sample_t(const QstatSampleParams* p, int G, size_t lds, int grid, hipStream_t stream) {
  void (*kern)(QstatSampleParams, int) = scan_qstat_sample_kernel<DT, NWIN>;
  static TsDeviceOnce lds_attr;
  TS_CHECK(ts_allow_max_lds(lds_attr, reinterpret_cast<const void*>(kern)));
  if (!p) return TS_OK;   // ts_scan_qstat_prepare
  hipLaunchKernelGGL(kern, dim3(grid), dim3(SCAN_THREADS), lds, stream, *p, G);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

static int qstat_sample_dispatch(const TsLayout& L, const QstatSampleParams* p, int G, size_t lds, int grid,
                                 hipStream_t stream) {
  const int nwin = qstat_nwin(L);
  if (L.dtype == TS_F16 && nwin == 5) return qstat_sample_t<TS_F16, 5>(p, G, lds, grid, stream);
  if (L.dtype == TS_F16 && nwin == 6) return qstat_sample_t<TS_F16, 6>(p, G, lds, grid, stream);
  if (L.dtype == TS_BF16 && nwin == 5) return qstat_sample_t<TS_BF16, 5>(p, G, lds, grid, stream);
  if (L.dtype == TS_BF16 && nwin == 6) return qstat_sample_t<TS_BF16, 6>(p, G, lds, grid, stream);
  ts_set_error("stationary sample scan: no kernel for dtype %d at dimension %d", L.dtype, L.dim);
  return TS_ERR_UNSUPPORTED;
}

template <int DT, int NWIN>
static int qstat_kernel_t(const WideScanParams* p, int G, size_t lds, int grid, hipStream_t stream) {
  void (*kern)(WideScanParams, int) = scan_qstat_kernel<DT, NWIN>;
  static TsDeviceOnce lds_attr;
  TS_CHECK(ts_allow_max_lds(lds_attr, reinterpret_cast<const void*>(kern)));
  if (!p) return TS_OK;   // ts_scan_qstat_prepare
  hipLaunchKernelGGL(kern, dim3(grid), dim3(SCAN_THREADS), lds, stream, *p, G);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

static int qstat_dispatch(const TsLayout& L, const WideScanParams* p, int G, size_t lds, int grid,
                          hipStream_t stream) {
  const int nwin = qstat_nwin(L);
  if (L.dtype == TS_F16 && nwin == 5) return qstat_kernel_t<TS_F16, 5>(p, G, lds, grid, stream);
  if (L.dtype == TS_F16 && nwin == 6) return qstat_kernel_t<TS_F16, 6>(p, G, lds, grid, stream);
  if (L.dtype == TS_BF16 && nwin == 5) return qstat_kernel_t<TS_BF16, 5>(p, G, lds, grid, stream);
  if (L.dtype == TS_BF16 && nwin == 6) return qstat_kernel_t<TS_BF16, 6>(p, G, lds, grid, stream);
  ts_set_error("stationary scan: no kernel for dtype %d at dimension %d", L.dtype, L.dim);
  return TS_ERR_UNSUPPORTED;
}

int ts_scan_qstat_prepare(const TsLayout& L) {
  if (ts_scan_qstat_groups(L) == 0) return TS_OK;
  TS_CHECK(qstat_sample_dispatch(L, nullptr, 0, 0, 0, nullptr));
  return qstat_dispatch(L, nullptr, 0, 0, 0, nullptr);
}

int ts_launch_scan_qstat_sample(const TsLayout& L, int G, const QstatSampleParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  // every sampled block lies inside the corpus, every line inside its buffer (the caller sizes it nq x dense_ld)
  bool ok = G >= 1 && G <= TS_QSTAT_GROUPS && ts_scan_qstat_groups(L) > 0 && p.kg == L.kg && p.blk_stride >= 1 &&
            p.blk0 >= 0 && (p.blk0 + (p.nwork - 1) * p.blk_stride) * TS_ROWS_PER_BLOCK < p.ntotal &&
            p.dense_ld >= p.nwork * TS_ROWS_PER_BLOCK && p.dense_ld % 4 == 0;
  for (int g = 0; ok && g < G; ++g)
    ok = p.gimg[g] && p.gdense[g] && p.gqh[g] >= 1 && p.gqh[g] <= 2 && p.ghalf[g] >= 0 && p.ghalf[g] < p.gqh[g] &&
         p.gnq[g] >= 1 && p.gnq[g] <= 32;
  if (!ok) {
    ts_set_error("stationary sample scan: bad geometry for %d groups at dimension %d", G, L.dim);
    return TS_ERR_UNSUPPORTED;
  }
  const size_t lds = (size_t)qstat_depth(L) * TS_QSTAT_WINDOW;   // the ring only
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(p.nwork, num_cus));
  return qstat_sample_dispatch(L, &p, G, lds, grid, stream);
}

int ts_launch_scan_qstat(const TsLayout& L, int G, const WideScanParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (G < 1 || G > TS_QSTAT_GROUPS || ts_scan_qstat_groups(L) == 0 || p.kg != L.kg || p.stage_cap == 0 ||
      p.stage_cap > ts_scan_qstat_stage_cap(L) || !ts_scan_qstat_fits(p.nwork, num_cus)) {
    ts_set_error("stationary scan: %d groups do not fit at dimension %d", G, L.dim);
    return TS_ERR_UNSUPPORTED;
  }
  const size_t lds = (size_t)qstat_depth(L) * TS_QSTAT_WINDOW + sizeof(StageQstatHdr) + 8 * (size_t)p.stage_cap;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(p.nwork, num_cus));
  return qstat_dispatch(L, &p, G, lds, grid, stream);
}
