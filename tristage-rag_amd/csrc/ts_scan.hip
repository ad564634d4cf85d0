// Stage-1 brute-force inner-product scan for gfx950 (MI355X, CDNA4).
//
// Replaces the arithmetic the reference reaches through
// faiss.IndexFlatIP.add / .search (reference src/stage1_retriever.py:263-277,
// 313, 380): every query of a batch (<= 64) against every corpus row.
//
// Design:
//   * HBM-bound streaming kernel.  The corpus is stored pre-tiled in MFMA
//     A-fragment order (ts_common.h), so each wave-level load is one
//     contiguous 1 KiB global_load_dwordx4 straight into VGPRs; no LDS round
//     trip and no barrier for the streamed operand.
//   * The query batch (the stationary operand, <= 128 KiB) is staged once per
//     workgroup into LDS in B-fragment order; every ds_read_b128 is
//     lane-linear, hence bank-conflict free.
//   * Each wave owns a 32-row x 64-query score tile held in two 32x32 MFMA
//     accumulators; a TS_RING-deep register ring keeps 8 KiB of corpus loads in
//     flight per wave across row-block boundaries (persistent waves).
//   * Epilogue, dense mode: scores are written out (small corpora, the sample
//     that seeds the thresholds, fallback).  Filter mode: a score survives
//     only if it is >= the per-query threshold; survivors (a few thousand per
//     query out of millions) are appended to per-query candidate lists, so the
//     B x N score matrix is never materialised.
#include "ts_scan_dev.h"
#include "ts_linear_dev.h"   // fs_barrier: the wide scan's window barrier
#include <stdlib.h>

// Multi-group filter mode (coalesced passes, TS_FLAG_COALESCE): scan_kernel's SCAN_FILTER loop for G 32-query
// groups that may belong to different batches (MultiScanParams, ts_common.h).  The prologue gathers each group's
// columns from its batch's Q image into one G-group image laid out like scan_kernel's (unit (kg*G + g)*64 + lane);
// the hot loop is scan_kernel's ring with G reads and G MFMAs per k group.  Every group's pointers are indexed by
// a compile-time group number where it matters (the epilogue), so they stay scalar.
//
// Staging: with 3 groups at d = 768 the image leaves 16 KiB of LDS, so a survivor takes 8 bytes instead of
// StageLds's 9: its score and one key word, (iteration << 15) | (wave << 12) | (row in block << 7) | query of
// the pass.  The row id is rebuilt in the flush from the workgroup's fixed walk: work item
// w = blockIdx.x * SCAN_WAVES + wave + iteration * (waves in the grid).  ts_scan_multi_fits() keeps the
// iteration count below 2^17.
struct StageMultiHdr {
  uint32_t cnt;
  uint32_t pad[3];
  uint32_t qcnt[TS_MAX_GROUPS * 32];
  uint32_t qbase[TS_MAX_GROUPS * 32];
  uint32_t qoff[TS_MAX_GROUPS * 32];
  // followed by float score[stage_cap], uint32_t key[stage_cap]
};
static_assert(SCAN_WAVES <= 8 && TS_MAX_GROUPS * 32 <= 128, "survivor key fields");
#define TS_MULTI_MAX_ITERS (1 << 17)
#define TS_MULTI_MIN_STAGE 1024u     // entries: below this a group count is not offered (ts_scan_multi_groups)
#define TS_MULTI_MAX_STAGE 4096u     // entries: more LDS than this buys nothing (about 1.3 k survivors per pass)

// a[g] for a run-time g < G, without a dynamically indexed kernel argument (that would go through scratch)
template <int G, class T, int N>
__device__ __forceinline__ T pick_group(const T (&a)[N], int g) {
  T r = a[0];
#pragma unroll
  for (int i = 1; i < G; ++i) r = (g == i) ? a[i] : r;
  return r;
}

// QB: bits of the query field of the survivor key (7 for scan_multi_kernel, 8 for scan_wide_kernel); the row in the
// block sits right above it.
// TOMB (the tombstone passes of an index with removed rows): staged survivors are checked against the
// live words when the workgroup flushes them (tomb_live), after the walk; a survivor that finds the staging area full
// is not appended but makes its batch overflow (redone exactly).
// The tests are wave-uniform: one ballot per group of the lanes whose largest score reaches the threshold (in a wide
// pass of 192 queries about five row blocks in six have one), then in a group with a hit one ballot per accumulator
// register, so the staging code runs with the execution mask of the lanes that hit.  The hit is marked unlikely: the
// compiler then lays a group's 16 tests out as 16 x (v_cmp, s_cbranch_vccnz) in a row and the staging blocks behind
// the loop, so a score that misses costs two instructions and no taken branch.  The row bound matters only in the
// corpus's partial last row block (wave-uniform too).  The per-lane LDS atomicAdd of 1 compiles to one wave-aggregated
// ds_add_rtn.  (-DTS_TUNING -DDBG_EPILOGUE_MASKS: the per-lane 16-bit masks this replaced, for A/B.)
template <int G, int QB, bool TOMB, class P, class H>
__device__ __forceinline__ void epilogue_multi(const P& p, H* st, float* sscore,
                                               uint32_t* skey, const f32x16 (&acc)[G], const float (&tau)[G],
                                               int64_t blk, uint32_t keyhi, int lane) {
#if defined(TS_TUNING) && defined(DBG_EPILOGUE_MASKS)   // A/B only: per-lane masks, then 16 x G divergent blocks
  bool hit = false;
#pragma unroll
  for (int hq = 0; hq < G; ++hq) hit |= (acc_max(acc[hq]) >= tau[hq]);
  if (__builtin_amdgcn_ballot_w64(hit) == 0ull) return;  // the common case
  const int64_t row_base = blk * TS_ROWS_PER_BLOCK;
  const int j = lane & 31;
#pragma unroll
  for (int hq = 0; hq < G; ++hq) {
    uint32_t mask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool ok = (acc[hq][r] >= tau[hq]) && (row_base + acc_row(r, lane) < p.ntotal);
      mask |= ok ? (1u << r) : 0u;
    }
    if (mask) {
      uint32_t slot = atomicAdd(&st->cnt, (uint32_t)__builtin_popcount(mask));  // LDS
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (mask & (1u << r)) {
          if (slot < p.stage_cap) {
            sscore[slot] = acc[hq][r];
            skey[slot] = keyhi | ((uint32_t)acc_row(r, lane) << QB) | (uint32_t)(hq * 32 + j);
          } else {
            // staging area full: append directly
            // (TOMB: nothing here knows whether the row is live, so the count is pushed past the list's capacity:
            // the select reports an overflow and the batch is redone exactly)
            if constexpr (TOMB) {
              atomicMax(&p.gcnt[hq][j], p.cand_cap + 1u);
            } else {
              const uint32_t g = atomicAdd(&p.gcnt[hq][j], 1u);
              if (g < p.cand_cap) {
                p.gscore[hq][(size_t)j * p.cand_cap + g] = acc[hq][r];
                p.gid[hq][(size_t)j * p.cand_cap + g] = (int32_t)(row_base + acc_row(r, lane));
              }
            }
          }
          ++slot;
        }
      }
    }
  }
#else
  uint64_t gm[G], any = 0;
#pragma unroll
  for (int hq = 0; hq < G; ++hq) {
    gm[hq] = __builtin_amdgcn_ballot_w64(acc_max(acc[hq]) >= tau[hq]);
    any |= gm[hq];
  }
  if (any == 0ull) return;
  const int64_t row_base = blk * TS_ROWS_PER_BLOCK;
  const bool partial = row_base + TS_ROWS_PER_BLOCK > p.ntotal;   // the corpus's last row block, wave-uniform
  const int rows_left = (int)(p.ntotal - row_base);                // (its rows: read only if partial)
#pragma unroll
  for (int hq = 0; hq < G; ++hq) {
    if (gm[hq] == 0ull) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool ok = acc[hq][r] >= tau[hq];
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(ok) == 0ull, 1)) continue;
      if (!ok) continue;
      // (the lane as the staging code's own value: what is computed from it, rows and the lists' addresses, is then
      // computed here and not kept in registers across the walk)
      int ln = lane;
      __asm__ volatile("" : "+v"(ln));
      const int row = acc_row(r, ln), j = ln & 31;
      if (!partial || row < rows_left) {
        const uint32_t slot = atomicAdd(&st->cnt, 1u);  // LDS
        if (slot < p.stage_cap) {
          sscore[slot] = acc[hq][r];
          skey[slot] = keyhi | ((uint32_t)row << QB) | (uint32_t)(hq * 32 + j);
        } else {
          // staging area full: append directly
          // (TOMB: nothing here knows whether the row is live, so the count is pushed past the list's capacity:
          // the select reports an overflow and the batch is redone exactly)
          if constexpr (TOMB) {
            atomicMax(&p.gcnt[hq][j], p.cand_cap + 1u);
          } else {
            const uint32_t g = atomicAdd(&p.gcnt[hq][j], 1u);
            if (g < p.cand_cap) {
              p.gscore[hq][(size_t)j * p.cand_cap + g] = acc[hq][r];
              p.gid[hq][(size_t)j * p.cand_cap + g] = (int32_t)(row_base + row);
            }
          }
        }
      }
    }
  }
#endif
}

// a staged survivor's row is live (after the walk: a plain load)
template <bool TOMB, class P>
__device__ __forceinline__ bool tomb_live(const P& p, int64_t row) {
  if constexpr (TOMB) return (p.live[row >> 5] >> (row & 31)) & 1u;
  return true;
}

// One kernel template for the plain passes (TOMB = false, MultiScanParams) and the tombstone passes of an index with
// removed rows (TOMB = true, MultiTombParams): the same walk, with removed rows dropped at the flush.  The kernel itself
// carries TOMB and takes its parameter block as the kernel argument; a __global__ wrapper around an inlined body that
// receives the block by reference is what changes the plain instantiations' code, so there is none.
template <int DT, int G, bool TOMB>
__global__ __launch_bounds__(SCAN_THREADS) void scan_multi_kernel(
    std::conditional_t<TOMB, MultiTombParams, MultiScanParams> p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* qlds = reinterpret_cast<u32x4*>(smem);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kg = p.kg;

  const int64_t nwaves = (int64_t)gridDim.x * SCAN_WAVES;
  int64_t w = (int64_t)blockIdx.x * SCAN_WAVES + wave;
  const bool active = w < p.nwork;  // (waves without work still join the final flush)
  const u32x4* base = reinterpret_cast<const u32x4*>(p.corpus) + lane;
  const size_t blk_units = (size_t)kg * 64;
  int64_t blk = active ? p.blk0 + w * p.blk_stride : p.blk0;
  const u32x4* cur = base + (size_t)blk * blk_units;
  u32x4 ring[TS_RING];
  if (active) {
#pragma unroll
    for (int i = 0; i < TS_RING; ++i) ring[i] = stream_load(cur + (size_t)i * 64);
  }

  // ---- prologue: gather the groups' columns (global/L2) into one G-group image in LDS, once per workgroup
  {
    const int units = kg * G * 64;
    for (int i0 = tid; i0 < units; i0 += 8 * SCAN_THREADS) {
      u32x4 t[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int i = i0 + jj * SCAN_THREADS;
        t[jj] = u32x4{0, 0, 0, 0};
        if (i < units) {
          const int u = i >> 6, gk = u / G, g = u - gk * G;
          const u32x4* src = reinterpret_cast<const u32x4*>(pick_group<G>(p.gimg, g));
          t[jj] = src[(size_t)(gk * pick_group<G>(p.gqh, g) + pick_group<G>(p.ghalf, g)) * 64 + (i & 63)];
        }
      }
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int i = i0 + jj * SCAN_THREADS;
        if (i < units) qlds[i] = t[jj];
      }
    }
  }
  StageMultiHdr* st = reinterpret_cast<StageMultiHdr*>(smem + (size_t)kg * G * 1024);
  float* sscore = reinterpret_cast<float*>(st + 1);
  uint32_t* skey = reinterpret_cast<uint32_t*>(sscore + p.stage_cap);
  if (tid == 0) st->cnt = 0;
  __syncthreads();

  if (active) {

  float tau[G];
#pragma unroll
  for (int hq = 0; hq < G; ++hq) tau[hq] = p.gtau[hq][lane & 31];

  const u32x4* ql = qlds + lane;
  uint32_t keyhi = (uint32_t)wave << 12;   // + (iteration << 15)

  while (true) {
    const int64_t wn = w + nwaves;
    const bool has_next = wn < p.nwork;
    const int64_t blkn = has_next ? (p.blk0 + wn * p.blk_stride) : blk;
    const u32x4* nxt = base + (size_t)blkn * blk_units;

    f32x16 acc[G];
#pragma unroll
    for (int hq = 0; hq < G; ++hq)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[hq][r] = 0.f;

    // main part: prefetch stays inside the current row block
    int g0 = 0;
    for (; g0 < kg - TS_RING; g0 += TS_RING) {
#pragma unroll
      for (int i = 0; i < TS_RING; ++i) {
#pragma unroll
        for (int hq = 0; hq < G; ++hq) {
          const u32x4 b = ql[(size_t)((g0 + i) * G + hq) * 64];
          mma_group<DT>(acc[hq], ring[i], b);
        }
        ring[i] = stream_load(cur + (size_t)(g0 + i + TS_RING) * 64);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // tail: the ring is refilled from the start of the wave's next row block
#pragma unroll
    for (int i = 0; i < TS_RING; ++i) {
#pragma unroll
      for (int hq = 0; hq < G; ++hq) {
        const u32x4 b = ql[(size_t)((g0 + i) * G + hq) * 64];
        mma_group<DT>(acc[hq], ring[i], b);
      }
      ring[i] = stream_load(nxt + (size_t)i * 64);
      __builtin_amdgcn_sched_barrier(0);
    }

    epilogue_multi<G, 7, TOMB>(p, st, sscore, skey, acc, tau, blk, keyhi, lane);

    if (!has_next) break;
    w = wn;
    blk = blkn;
    cur = nxt;
    keyhi += 1u << 15;
  }
  }  // active

  // ---- flush: one global atomic per (workgroup, query) reserves the slots
  __syncthreads();
  const uint32_t n = st->cnt < p.stage_cap ? st->cnt : p.stage_cap;
  if (n == 0) return;  // uniform: cnt is final after the barrier
  if (tid < G * 32) { st->qcnt[tid] = 0; st->qoff[tid] = 0; }
  __syncthreads();
  // (TOMB: the global row of a staged key, to drop removed rows from both loops alike)
  auto key_row = [&](uint32_t key) {
    const int64_t wi = (int64_t)blockIdx.x * SCAN_WAVES + ((key >> 12) & 7u) + (int64_t)(key >> 15) * nwaves;
    return (p.blk0 + wi * p.blk_stride) * TS_ROWS_PER_BLOCK + ((key >> 7) & 31u);
  };
  for (uint32_t e = tid; e < n; e += SCAN_THREADS) {
    if constexpr (TOMB)
      if (!tomb_live<TOMB>(p, key_row(skey[e]))) continue;
    atomicAdd(&st->qcnt[skey[e] & 127u], 1u);
  }
  __syncthreads();
  if (tid < G * 32 && st->qcnt[tid] > 0)
    st->qbase[tid] = atomicAdd(pick_group<G>(p.gcnt, tid >> 5) + (tid & 31), st->qcnt[tid]);
  __syncthreads();
  for (uint32_t e = tid; e < n; e += SCAN_THREADS) {
    const uint32_t key = skey[e];
    if constexpr (TOMB)
      if (!tomb_live<TOMB>(p, key_row(key))) continue;
    const uint32_t q = key & 127u;
    const uint32_t slot = st->qbase[q] + atomicAdd(&st->qoff[q], 1u);
    if (slot < p.cand_cap) {
      const int g = (int)(q >> 5);
      const size_t at = (size_t)(q & 31u) * p.cand_cap + slot;
      const int64_t wi = (int64_t)blockIdx.x * SCAN_WAVES + ((key >> 12) & 7u) + (int64_t)(key >> 15) * nwaves;
      pick_group<G>(p.gscore, g)[at] = sscore[e];
      pick_group<G>(p.gid, g)[at] = (int32_t)((p.blk0 + wi * p.blk_stride) * TS_ROWS_PER_BLOCK + ((key >> 7) & 31u));
    }
  }
}

int ts_scan_multi_groups(const TsLayout& L) {
  if (L.dtype != TS_F16 && L.dtype != TS_BF16) return 0;
  for (int G = TS_MAX_GROUPS; G >= 1; --G)
    if (ts_scan_multi_stage_cap(L, G) > 0) return G;
  return 0;
}

uint32_t ts_scan_multi_stage_cap(const TsLayout& L, int G) {
  const size_t fixed = (size_t)L.kg * G * 1024 + sizeof(StageMultiHdr);
  if (G < 1 || G > TS_MAX_GROUPS || fixed + 8 * (size_t)TS_MULTI_MIN_STAGE > TS_LDS_BYTES) return 0;
  return (uint32_t)std::min<size_t>(TS_MULTI_MAX_STAGE, (TS_LDS_BYTES - fixed) / 8);
}

// the grid of ts_launch_scan_multi: at most num_cus workgroups of SCAN_WAVES waves
bool ts_scan_multi_fits(int64_t nblk, int num_cus) {
  const int64_t want = (nblk + SCAN_WAVES - 1) / SCAN_WAVES;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(want, num_cus));
  const int64_t nwaves = grid * SCAN_WAVES;
  return (nblk + nwaves - 1) / nwaves <= TS_MULTI_MAX_ITERS;
}

template <int DT, int G, class P = MultiScanParams>
static int launch_scan_multi_t(const TsLayout& L, const P& p, int num_cus, hipStream_t stream) {
  const size_t lds = (size_t)L.kg * G * 1024 + sizeof(StageMultiHdr) + 8 * (size_t)p.stage_cap;
  void (*kern)(P) = scan_multi_kernel<DT, G, std::is_same<P, MultiTombParams>::value>;
  static TsDeviceOnce lds_attr;
  TS_CHECK(ts_allow_max_lds(lds_attr, reinterpret_cast<const void*>(kern)));
  const int64_t want = (p.nwork + SCAN_WAVES - 1) / SCAN_WAVES;
  int grid = (int)(want < num_cus ? want : num_cus);
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(SCAN_THREADS), lds, stream, p);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

template <class P>
static int launch_scan_multi_any(const TsLayout& L, int G, const P& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (p.stage_cap == 0 || p.stage_cap > ts_scan_multi_stage_cap(L, G) || !ts_scan_multi_fits(p.nwork, num_cus)) {
    ts_set_error("multi-group scan: %d groups do not fit at dimension %d", G, L.dim);
    return TS_ERR_UNSUPPORTED;
  }
#define TS_MULTI_G(DT)                                                      \
  switch (G) {                                                              \
    case 1: return launch_scan_multi_t<DT, 1, P>(L, p, num_cus, stream);    \
    case 2: return launch_scan_multi_t<DT, 2, P>(L, p, num_cus, stream);    \
    case 3: return launch_scan_multi_t<DT, 3, P>(L, p, num_cus, stream);    \
    case 4: return launch_scan_multi_t<DT, 4, P>(L, p, num_cus, stream);    \
  }
  switch (L.dtype) {
    case TS_F16: TS_MULTI_G(TS_F16); break;
    case TS_BF16: TS_MULTI_G(TS_BF16); break;
  }
#undef TS_MULTI_G
  ts_set_error("multi-group scan: bad dtype %d or group count %d", L.dtype, G);
  return TS_ERR_UNSUPPORTED;
}

int ts_launch_scan_multi(const TsLayout& L, int G, const MultiScanParams& p, int num_cus, hipStream_t stream) {
  return launch_scan_multi_any(L, G, p, num_cus, stream);
}

int ts_launch_scan_multi_tomb(const TsLayout& L, int G, const MultiTombParams& p, int num_cus, hipStream_t stream) {
  return launch_scan_multi_any(L, G, p, num_cus, stream);
}

// Wide coalesced passes (scan_wide_kernel<DT, G>, WideScanParams): scan_multi_kernel for more groups than their
// query images can keep resident in LDS.  The corpus path is scan_kernel's persistent waves, row blocks and order of
// non-temporal loads, with a register ring two windows (2 * TS_RING units) deep.  The query side is a double-buffered
// window in LDS: TS_RING k groups of all G groups (G * TS_RING KiB; unit (i*G + g)*64 + lane for k group g0 + i of
// group g, the resident image's order), so G no longer depends on the dimension.  The k groups of a row block are
// walked in windows of TS_RING — the g0 += TS_RING steps of scan_kernel — and every row block walks the same
// windows, so the workgroup's waves meet at one barrier per window:
//   * at the start of window t each wave requests its G units of window t + 1 from the batches' Q images (L2: a pass
//     reads at most a few hundred KiB of images, and FETCH_SIZE stays one corpus read) by LDS-DMA into the other
//     buffer;
//   * it runs the window's TS_RING x G MFMAs out of the current buffer and refills that ring half with window t + 2;
//     the B operands roll through G register sets, each re-read for the next slot right after its MFMA;
//   * it waits for the units (vmcnt(TS_RING): the ring loads issued in this window stay in flight) and meets the
//     others at lgkmcnt(0) + s_barrier.
// The other buffer was last read in window t - 1, before the previous barrier.  A window's corpus units are thus
// requested a full window before it starts, where a one-window ring requested them during the window before: with
// 48 MFMAs per window the loads then arrived late and the workgroup waited at the barrier for its slowest wave
// (DESIGN.md 4.2c).  Waves whose walk is shorter than the workgroup's longest (one iteration less, or no work at
// all) keep requesting windows and meeting the barrier until that walk ends.  Each group's MFMA chain is
// scan_kernel's for it (same operands, k order, zeroed start), so a query's score bits do not depend on G or on which
// groups share its pass.
//
// Survivor keys need 8 query bits at G > 4: (iteration << 16) | (wave << 13) | (row in block << 8) | query of the
// pass; ts_scan_wide_fits() keeps the iteration count below 2^16.  Staging gets the LDS the two windows leave.
struct StageWideHdr {
  uint32_t cnt;
  uint32_t pad[3];
  uint32_t qcnt[TS_MAX_WIDE_GROUPS * 32];
  uint32_t qbase[TS_MAX_WIDE_GROUPS * 32];
  uint32_t qoff[TS_MAX_WIDE_GROUPS * 32];
  // followed by float score[stage_cap], uint32_t key[stage_cap]
};
static_assert(SCAN_WAVES <= 8 && TS_MAX_WIDE_GROUPS * 32 <= 256, "wide survivor key fields");
static_assert(SCAN_THREADS == TS_RING * 64, "a window is G units per thread");
#define TS_WIDE_GROUPS 6             // groups per wide pass: three 64-query batches
#define TS_WIDE_MAX_ITERS (1 << 16)
#define TS_WIDE_MIN_STAGE 4096u      // entries
#define TS_WIDE_MAX_STAGE 8192u      // entries: about 2.6 k survivors per workgroup and pass at G = 6

// f(std::integral_constant<int, i>) for i = 0 .. N-1: unrolled with i usable as an inline-asm immediate
template <int N, int I = 0, class F>
__device__ __forceinline__ void ts_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    ts_static_for<N, I + 1>(f);
  }
}

// ring slot I of the wide scan: fill (wave-uniform) + the lane's 16-byte offset + I KiB, as the lane offset and an
// immediate of (I % 4) KiB from fill or fill + 4 KiB (no offset registers); non-temporal like stream_load.
// (s_nop 4: a VMEM instruction may read an SGPR only 5 wait states after a VALU wrote it (v_readfirstlane), and
// the compiler pads nothing inside an asm statement; the base is SALU arithmetic today, which needs none, but that is
// the compiler's choice.  Issue cost only: the MFMAs in flight keep running.)
// The destination is written when the load lands, up to two windows after the statement, while the compiler takes it
// as written at once: the kernel is correct only if the compiler neither copies nor spills a ring register in between.
// It does neither while the kernel uses no scratch (every instantiation, tests/test_wide_prefetch_build.py).  A
// TS_TUNING build without MFMAs spills, so there the loads are plain ones the compiler waits for.
template <int I>
__device__ __forceinline__ void wide_ring_load(u32x4& r, uint32_t loff, const unsigned char* fill) {
#if defined(TS_TUNING) && defined(DBG_NO_MFMA)
  r = stream_load(reinterpret_cast<const u32x4*>(fill + loff + I * 1024));
#else
  __asm__ volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3 nt"
                   : "=v"(r) : "v"(loff), "s"(fill + (I / 4) * 4096), "i"((I % 4) * 1024) : "memory");
#endif
}

#if defined(TS_TUNING) && defined(WIDE_TRACE)   // diagnostic builds only: per-wave phase sums of the wide walk, tools/trace_wide.py
// Row (workgroup * SCAN_WAVES + wave) of the last wide launch: 100 MHz ticks summed over the wave's windows for
// 0 gather requests, 1 the window's first-slot operand reads (issued and waited for: lgkmcnt(0), which the untraced
// walk does not wait for in one piece), 2 the TS_RING slots (MFMAs, re-reads, refills), 3 fill pointer + epilogue,
// 4 the vmcnt wait for the next window's units, 5 the barrier; then 6 the walk's ticks, 7 its s_memtime counts,
// 8 the wave's windows.  A stamp is a scalar memory read, so it waits lgkmcnt(0) itself: none inside the slots.
#define WIDE_TRACE_ROW 10
__device__ uint32_t wide_trace_buf[256 * SCAN_WAVES * WIDE_TRACE_ROW];
extern "C" int ts_debug_wide_trace(uint32_t* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(wide_trace_buf), sizeof(wide_trace_buf)) == hipSuccess ? 0 : -2;
}
#define WIDE_TRACE_BEGIN()                                              \
  uint32_t wt_sum[6] = {0, 0, 0, 0, 0, 0};                              \
  const uint32_t wt_c0 = (uint32_t)__builtin_readcyclecounter();        \
  const uint32_t wt_t0 = (uint32_t)__builtin_amdgcn_s_memrealtime();    \
  uint32_t wt_last = wt_t0
#define WIDE_STAMP(k)                                                   \
  do {                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                  \
    const uint32_t now_ = (uint32_t)__builtin_amdgcn_s_memrealtime();   \
    wt_sum[k] += now_ - wt_last;                                        \
    wt_last = now_;                                                     \
    __builtin_amdgcn_sched_barrier(0);                                  \
  } while (0)
#define WIDE_STAMP_READS(k)                                             \
  do {                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                  \
    __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0) */                \
    WIDE_STAMP(k);                                                      \
  } while (0)
#define WIDE_TRACE_END(nwindows)                                                                     \
  do {                                                                                               \
    if (lane == 0 && blockIdx.x < 256) {                                                             \
      uint32_t* row_ = wide_trace_buf + ((size_t)blockIdx.x * SCAN_WAVES + wave) * WIDE_TRACE_ROW;   \
      for (int k_ = 0; k_ < 6; ++k_) row_[k_] = wt_sum[k_];                                          \
      row_[6] = (uint32_t)__builtin_amdgcn_s_memrealtime() - wt_t0;                                  \
      row_[7] = (uint32_t)__builtin_readcyclecounter() - wt_c0;                                      \
      row_[8] = (uint32_t)(nwindows);                                                                \
    }                                                                                                \
  } while (0)
#else
#define WIDE_TRACE_BEGIN() do { } while (0)
#define WIDE_STAMP(k) do { } while (0)
#define WIDE_STAMP_READS(k) do { } while (0)
#define WIDE_TRACE_END(nwindows) do { } while (0)
#endif

// Staggered requests: the slots whose MFMAs the second half of a workgroup's waves runs before it
// requests the next window's units; -1: every wave requests right after the barrier.  Kept as an A/B switch only:
// S = 1 .. 3 measured no gain at 10 M x 768 (the late waves are the window's critical path wherever their requests
// stand), so the default build has none of it.
#if defined(TS_TUNING) && defined(DBG_WIDE_STAGGER)   // A/B only
#define TS_WIDE_STAGGER DBG_WIDE_STAGGER
#else
#define TS_WIDE_STAGGER (-1)
#endif
static_assert(TS_WIDE_STAGGER >= -1 && TS_WIDE_STAGGER < TS_RING - 1, "stagger slots");

// One kernel template, like scan_multi_kernel: TOMB = false takes WideScanParams, TOMB = true WideTombParams.  In a
// tombstone pass removed rows are dropped from the staged survivors at the flush (tomb_live), after the ring, so no
// load enters the walk; only a survivor that finds the staging area full makes its batch overflow and be redone.
template <int DT, int G, bool TOMB>
__global__ __launch_bounds__(SCAN_THREADS) void scan_wide_kernel(
    std::conditional_t<TOMB, WideTombParams, WideScanParams> p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int WU = G * TS_RING * 64;   // 16-byte units per window buffer
  u32x4* win = reinterpret_cast<u32x4*>(smem);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kg = p.kg;
  const int nwin = kg / TS_RING;   // (ts_make_layout: kg is a multiple of TS_RING)

  const int64_t nwaves = (int64_t)gridDim.x * SCAN_WAVES;
  const int64_t w0 = (int64_t)blockIdx.x * SCAN_WAVES;
  int64_t w = w0 + wave;
  const bool active = w < p.nwork;
  const size_t blk_units = (size_t)kg * 64;
  int64_t blk = active ? p.blk0 + w * p.blk_stride : p.blk0;

  // walks, in windows: this wave's (its row blocks x nwin) and the workgroup's longest (its wave 0's)
  const int64_t my_iters = active ? (p.nwork - 1 - w) / nwaves + 1 : 0;
  const int64_t wg_iters = w0 < p.nwork ? (p.nwork - 1 - w0) / nwaves + 1 : 0;
  const int64_t tw_mine = my_iters * nwin, tw_all = wg_iters * nwin;

  // The ring is two windows deep: window t of the walk computes from slots (t & 1) * TS_RING + i and refills them
  // with window t + 2, so every corpus unit is requested a full window before the window that needs it starts.
  // `fill` (wave-uniform, scalar) is the first byte of the window the next refill requests, `fwin` its window in the
  // row block.  A lane adds its 16 bytes as a 32-bit offset.
  const unsigned char* corpus = reinterpret_cast<const unsigned char*>(p.corpus);
  const uint32_t loff = (uint32_t)lane * 16;
  int64_t fw = w;
  const unsigned char* fill = corpus + (size_t)blk * blk_units * 16;
  // past the end of the walk the refills (two windows per wave, never consumed) read the first 8 KiB of group 0's
  // query image instead: in bounds (an image holds kg >= TS_RING KiB per 32 queries), L2-resident (every window's
  // requests read it), so no corpus bytes are fetched twice, and every window still issues TS_RING ring loads
  const unsigned char* const fill_dead = reinterpret_cast<const unsigned char*>(p.gimg[0]);
  bool fill_done = false;
  int fwin = 0;
  auto advance_fill = [&]() {
    if (fill_done) return;
    if (++fwin < nwin) {
      fill += TS_RING * 1024;
    } else if (fw + nwaves < p.nwork) {
      fwin = 0;
      fw += nwaves;
      fill = corpus + (size_t)(p.blk0 + fw * p.blk_stride) * blk_units * 16;
    } else {
      fill_done = true;
      fill = fill_dead;
    }
  };
#if defined(TS_TUNING) && defined(DBG_WIDE_L2_RING)   // ablation builds only (wrong results): the ring reads one L2-resident 8 KiB
  fill = fill_dead;
  fill_done = true;
#endif
  // The ring's loads are inline asm too, and the walk waits for them itself (ring_wait): the compiler's waitcnt pass
  // does not count the units' LDS-DMA, and for loads it counts it waits as if the ring were one window deep.
  // Requests per wave, oldest first: the units of window t + 1 (G), then the ring loads of window t + 2 (TS_RING)
  // at window t; so a slot's load is followed by (TS_RING - 1) + 2 * G + TS_RING younger ones when it is consumed.
  auto refill = [&](u32x4& r, auto slot) { wide_ring_load<decltype(slot)::value>(r, loff, fill); };
  // (staggered requests, TS_WIDE_STAGGER = S >= 0: slots 0 .. S are consumed before the workgroup's late half of waves
  // has requested anything in this window, so their loads have only 2 * TS_RING - 1 + G - slot younger ones there; the
  // early half uses the same count, which makes it wait in addition only for ring loads two windows old and for units
  // the last barrier already waited for)
  auto ring_wait = [&](u32x4& r, auto slot) {
    constexpr int I = decltype(slot)::value;
    __asm__ volatile("s_waitcnt vmcnt(%1)" : "+v"(r)
                     : "i"(I <= TS_WIDE_STAGGER ? 2 * TS_RING - 1 + G - I : 2 * TS_RING - 1 + 2 * G));
  };

  // this thread's share of every window: units tid + j*SCAN_THREADS (j < G) = k group v / G of the window, group
  // v % G, v = wave + SCAN_WAVES*j (wave-uniform).  A wave's 64 lanes fill 64 consecutive units, so each share is
  // one LDS-DMA (global_load_lds_dwordx4: per-lane source, LDS destination = wave-uniform base + lane * 16) from a
  // wave-uniform source base plus the lane's 16 bytes: no registers hold the units, no ds_write copies them.
  // (Inline asm, not the builtin: DESIGN.md §8.  The requests are invisible to the compiler's waitcnt pass, so its
  // waits for the ring can only come out stricter; their own completion is the explicit vmcnt before each barrier.)
  const unsigned char* qsrc[G];
  int64_t qstep[G];   // bytes between windows
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const int v = wave + SCAN_WAVES * j, i = v / G, g = v - i * G;
    const int gqh = pick_group<G>(p.gqh, g);
    qsrc[j] = reinterpret_cast<const unsigned char*>(pick_group<G>(p.gimg, g)) +
              (size_t)(i * gqh + pick_group<G>(p.ghalf, g)) * 1024;
    qstep[j] = (int64_t)gqh * TS_RING * 1024;
  }
  const uint32_t win_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(win + wave * 64);
  // request window wi's units into buffer b
  auto gather = [&](int wi, int b) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const unsigned char* src = qsrc[j] + wi * qstep[j];
      const uint32_t dst = win_lds + (uint32_t)(b * WU + j * SCAN_THREADS) * 16;
      // s_nop 4: the SGPR-base hazard of wide_ring_load.  s_nop 0: an LDS-DMA may read M0 one wait state after an
      // SALU wrote it.  M0 is saved and restored: the compiler reserves it, and a clobber would not make it do so.
      uint32_t keep;
      __asm__ volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                       "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                       : "=&s"(keep) : "v"(loff), "s"(src), "s"(dst) : "memory");
    }
  };

  StageWideHdr* st = reinterpret_cast<StageWideHdr*>(smem + (size_t)2 * WU * 16);
  float* sscore = reinterpret_cast<float*>(st + 1);
  uint32_t* skey = reinterpret_cast<uint32_t*>(sscore + p.stage_cap);
  if (tid == 0) st->cnt = 0;

  // (the thresholds are loaded before the ring: no load issued ahead of the walk is still pending inside it)
  float tau[G];
#pragma unroll
  for (int hq = 0; hq < G; ++hq) tau[hq] = p.gtau[hq][lane & 31];
#pragma unroll
  for (int hq = 0; hq < G; ++hq) __asm__ volatile("" : "+v"(tau[hq]));   // (loaded here, not sunk into the walk)
  // the ring's first window, window 0's query units, the ring's second window: the same order of requests as
  // every later window's
  u32x4 ring[2 * TS_RING];
  if (active) {
    ts_static_for<TS_RING>([&](auto i) { refill(ring[i], i); });
    advance_fill();
  }
  gather(0, 0);
  if (active) {
    ts_static_for<TS_RING>([&](auto i) { refill(ring[TS_RING + i], i); });
    advance_fill();
    __builtin_amdgcn_s_waitcnt(0x3F70 | TS_RING);   // vmcnt(TS_RING)
  } else {
    __builtin_amdgcn_s_waitcnt(0x3F70);   // vmcnt(0)
  }
  fs_barrier();

  uint32_t keyhi = (uint32_t)wave << 13;   // + (iteration << 16)

  f32x16 acc[G];
#pragma unroll
  for (int hq = 0; hq < G; ++hq)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[hq][r] = 0.f;

  // the walk's window barrier (fs_barrier: vmcnt untouched)
  auto walk_barrier = [&]() {
#if defined(TS_TUNING) && defined(DBG_WIDE_NO_BARRIER)   // ablation builds only (wrong results; with TS_DEBUG_TAU_INF=1)
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
#else
    fs_barrier();
#endif
  };
  // Window t of the wave's walk (k window qw of a row block), ring half and LDS buffer P = t & 1: request the next
  // window's query units into the other buffer, run the window's TS_RING x G MFMAs and refill the ring half with
  // window t + 2, wait for the units (vmcnt(TS_RING): this window's ring loads stay in flight) and meet the others
  // at lgkmcnt(0) + s_barrier.  The other buffer was last read in window t - 1, before the previous barrier.
  int qw = 0;
  WIDE_TRACE_BEGIN();
  auto window = [&](auto half) {
    constexpr int P = decltype(half)::value;
    const int qn = qw + 1 < nwin ? qw + 1 : 0;
    // Nothing is pending here after a window barrier; ahead of the first window the compiler may have started scalar
    // loads of loop-invariant kernel arguments (the epilogue's) that it waits for only at their use.  With one of
    // those counted as in flight it waits lgkmcnt(0) before slot 0's first MFMA in every window, for all G operand
    // reads at once.
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
    // staggered requests: the waves of the workgroup's second half (w and w + SCAN_WAVES / 2 share a SIMD) run the
    // MFMAs of slots 0 .. S before they request the units, while their SIMD partners request first.  Every wave defers
    // the refills of slots 0 .. S until then, so a wave's requests keep their order: G units, then refills 0 .. 7.
    const bool late = TS_WIDE_STAGGER >= 0 && wave >= SCAN_WAVES / 2;
    if (!late) gather(qn, P ^ 1);
    WIDE_STAMP(0);
    const u32x4* ql = win + P * WU + lane;
#if !(defined(TS_TUNING) && defined(DBG_WIDE_SERIAL_B))
    // slot 0's operands: the buffer is valid since the barrier that ended the window before
    u32x4 bb[G];
#pragma unroll
    for (int hq = 0; hq < G; ++hq) bb[hq] = ql[hq * 64];
#endif
    WIDE_STAMP_READS(1);
    ts_static_for<TS_RING>([&](auto i) {
#if defined(TS_TUNING) && defined(DBG_WIDE_SERIAL_B)   // A/B only: one B register set, every MFMA waits for its own read
      ring_wait(ring[P * TS_RING + i], i);
#pragma unroll
      for (int hq = 0; hq < G; ++hq) {
        const u32x4 b = ql[(i * G + hq) * 64];
        mma_group<DT>(acc[hq], ring[P * TS_RING + i], b);
      }
#else
      // rolling B operands: group hq's register set is re-read with the next slot's operand as soon as its MFMA has
      // issued, so every read is G - 1 MFMAs ahead of its use (lgkmcnt(G - 1) before each MFMA, counted by the
      // compiler; it counts down to 0 only in the window's last slot).  The sched_barriers pin that order: left
      // alone the scheduler puts each read back in front of its MFMA.
      __builtin_amdgcn_sched_barrier(0);
      ring_wait(ring[P * TS_RING + i], i);
#pragma unroll
      for (int hq = 0; hq < G; ++hq) {
        mma_group<DT>(acc[hq], ring[P * TS_RING + i], bb[hq]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (decltype(i)::value + 1 < TS_RING) {
          bb[hq] = ql[((i + 1) * G + hq) * 64];
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#endif
      if constexpr (decltype(i)::value == TS_WIDE_STAGGER) {
        if (late) gather(qn, P ^ 1);
        ts_static_for<TS_WIDE_STAGGER + 1>([&](auto k) { refill(ring[P * TS_RING + k], k); });
      } else if constexpr (decltype(i)::value > TS_WIDE_STAGGER) {
        refill(ring[P * TS_RING + i], i);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    WIDE_STAMP(2);
    advance_fill();
    if (qw == nwin - 1) {   // the row block's last window
      epilogue_multi<G, 8, TOMB>(p, st, sscore, skey, acc, tau, blk, keyhi, lane);
#pragma unroll
      for (int hq = 0; hq < G; ++hq)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[hq][r] = 0.f;
      w += nwaves;
      blk = p.blk0 + w * p.blk_stride;
      keyhi += 1u << 16;
    }
    WIDE_STAMP(3);
    __builtin_amdgcn_s_waitcnt(0x3F70 | TS_RING);   // vmcnt(TS_RING)
    WIDE_STAMP(4);
    walk_barrier();
    WIDE_STAMP(5);
    qw = qn;
  };
  // Ring slots and buffers are compile-time, so the walk goes in pairs of windows (nwin may be odd).  The walk has
  // no branch between a wave's computing windows: every window's waits see the same two windows of ring loads.
  int64_t t = 0;
  for (; t < tw_mine; t += 2) {
    window(std::integral_constant<int, 0>{});
    if (t + 1 == tw_mine) { ++t; break; }
    window(std::integral_constant<int, 1>{});
  }
  // The last window's ring loads are still in flight, into registers the compiler now takes as free: nothing that
  // follows may be written before they land.
  __builtin_amdgcn_s_waitcnt(0x3F70);   // vmcnt(0)
  // the workgroup's other waves are still walking: keep filling windows with them
  for (; t < tw_all; ++t) {
    const int qn = qw + 1 < nwin ? qw + 1 : 0;
    gather(qn, (int)(t & 1) ^ 1);
    __builtin_amdgcn_s_waitcnt(0x3F70);   // vmcnt(0)
    walk_barrier();
    qw = qn;
  }
  WIDE_TRACE_END(tw_mine);

  // ---- flush: one global atomic per (workgroup, query) reserves the slots
  __syncthreads();
  const uint32_t n = st->cnt < p.stage_cap ? st->cnt : p.stage_cap;
  if (n == 0) return;  // uniform: cnt is final after the barrier
  for (int t = tid; t < G * 32; t += SCAN_THREADS) { st->qcnt[t] = 0; st->qoff[t] = 0; }
  __syncthreads();
  // (TOMB: the global row of a staged key, to drop removed rows from both loops alike)
  auto key_row = [&](uint32_t key) {
    const int64_t wi = (int64_t)blockIdx.x * SCAN_WAVES + ((key >> 13) & 7u) + (int64_t)(key >> 16) * nwaves;
    return (p.blk0 + wi * p.blk_stride) * TS_ROWS_PER_BLOCK + ((key >> 8) & 31u);
  };
  for (uint32_t e = tid; e < n; e += SCAN_THREADS) {
    if constexpr (TOMB)
      if (!tomb_live<TOMB>(p, key_row(skey[e]))) continue;
    atomicAdd(&st->qcnt[skey[e] & 255u], 1u);
  }
  __syncthreads();
  for (int t = tid; t < G * 32; t += SCAN_THREADS)
    if (st->qcnt[t] > 0) st->qbase[t] = atomicAdd(pick_group<G>(p.gcnt, t >> 5) + (t & 31), st->qcnt[t]);
  __syncthreads();
  for (uint32_t e = tid; e < n; e += SCAN_THREADS) {
    const uint32_t key = skey[e];
    if constexpr (TOMB)
      if (!tomb_live<TOMB>(p, key_row(key))) continue;
    const uint32_t q = key & 255u;
    const uint32_t slot = st->qbase[q] + atomicAdd(&st->qoff[q], 1u);
    if (slot < p.cand_cap) {
      const int g = (int)(q >> 5);
      const size_t at = (size_t)(q & 31u) * p.cand_cap + slot;
      const int64_t wi = (int64_t)blockIdx.x * SCAN_WAVES + ((key >> 13) & 7u) + (int64_t)(key >> 16) * nwaves;
      pick_group<G>(p.gscore, g)[at] = sscore[e];
      pick_group<G>(p.gid, g)[at] = (int32_t)((p.blk0 + wi * p.blk_stride) * TS_ROWS_PER_BLOCK + ((key >> 8) & 31u));
    }
  }
}

int ts_scan_wide_groups(const TsLayout& L) {
  if (L.dtype != TS_F16 && L.dtype != TS_BF16) return 0;
  return ts_scan_wide_stage_cap(L, TS_WIDE_GROUPS) > 0 ? TS_WIDE_GROUPS : 0;
}

uint32_t ts_scan_wide_stage_cap(const TsLayout& L, int G) {
  (void)L;   // the windows do not depend on the dimension
  const size_t fixed = (size_t)2 * G * TS_RING * 1024 + sizeof(StageWideHdr);
  if (G < 2 || G > TS_WIDE_GROUPS || fixed + 8 * (size_t)TS_WIDE_MIN_STAGE > TS_LDS_BYTES) return 0;
  return (uint32_t)std::min<size_t>(TS_WIDE_MAX_STAGE, (TS_LDS_BYTES - fixed) / 8);
}

bool ts_scan_wide_fits(int64_t nblk, int num_cus) {
  const int64_t want = (nblk + SCAN_WAVES - 1) / SCAN_WAVES;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(want, num_cus));
  const int64_t nwaves = grid * SCAN_WAVES;
  return (nblk + nwaves - 1) / nwaves <= TS_WIDE_MAX_ITERS;
}

template <int DT, int G, class P = WideScanParams>
static int launch_scan_wide_t(const P& p, int num_cus, hipStream_t stream) {
  const size_t lds = (size_t)2 * G * TS_RING * 1024 + sizeof(StageWideHdr) + 8 * (size_t)p.stage_cap;
  void (*kern)(P) = scan_wide_kernel<DT, G, std::is_same<P, WideTombParams>::value>;
  static TsDeviceOnce lds_attr;
  TS_CHECK(ts_allow_max_lds(lds_attr, reinterpret_cast<const void*>(kern)));
  const int64_t want = (p.nwork + SCAN_WAVES - 1) / SCAN_WAVES;
  int grid = (int)(want < num_cus ? want : num_cus);
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(SCAN_THREADS), lds, stream, p);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

template <class P>
static int launch_scan_wide_any(const TsLayout& L, int G, const P& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (p.stage_cap == 0 || p.stage_cap > ts_scan_wide_stage_cap(L, G) || !ts_scan_wide_fits(p.nwork, num_cus) ||
      L.kg % TS_RING != 0) {
    ts_set_error("wide scan: %d groups do not fit at dimension %d", G, L.dim);
    return TS_ERR_UNSUPPORTED;
  }
  // (G = 2..4: partial passes that the LDS-resident kernel cannot take at this dimension)
#define TS_WIDE_G(DT)                                                   \
  switch (G) {                                                          \
    case 2: return launch_scan_wide_t<DT, 2, P>(p, num_cus, stream);    \
    case 3: return launch_scan_wide_t<DT, 3, P>(p, num_cus, stream);    \
    case 4: return launch_scan_wide_t<DT, 4, P>(p, num_cus, stream);    \
    case 5: return launch_scan_wide_t<DT, 5, P>(p, num_cus, stream);    \
    case 6: return launch_scan_wide_t<DT, 6, P>(p, num_cus, stream);    \
  }
  switch (L.dtype) {
    case TS_F16: TS_WIDE_G(TS_F16); break;
    case TS_BF16: TS_WIDE_G(TS_BF16); break;
  }
#undef TS_WIDE_G
  ts_set_error("wide scan: bad dtype %d or group count %d", L.dtype, G);
  return TS_ERR_UNSUPPORTED;
}

int ts_launch_scan_wide(const TsLayout& L, int G, const WideScanParams& p, int num_cus, hipStream_t stream) {
  return launch_scan_wide_any(L, G, p, num_cus, stream);
}

int ts_launch_scan_wide_tomb(const TsLayout& L, int G, const WideTombParams& p, int num_cus, hipStream_t stream) {
  return launch_scan_wide_any(L, G, p, num_cus, stream);
}

bool ts_use_f32_split(const TsLayout& L, int qh) {
  if (L.dtype != TS_F32 || qh != 1) return false;
#ifdef TS_TUNING   // A/B: TS_NO_F32_SPLIT=1 keeps the exact-f32 MFMA kernel
  static const bool off = getenv("TS_NO_F32_SPLIT") != nullptr;
  if (off) return false;
#endif
  const size_t s = ts_scan_f32s_lds_bytes(L);
  if (s == 0 || s > TS_LDS_BYTES) return false;
  // only where the exact-f32 kernel could not take 64 queries per pass anyway
  return (size_t)L.kg * 2 * 1024 + sizeof(StageLds) > TS_LDS_BYTES;
}

size_t ts_scan_lds_bytes(const TsLayout& L, int qh) {
  if (L.dtype == TS_FP8_E4M3) return ts_scan_fp8_lds_bytes(L, qh);
  if (L.dtype == TS_MXFP4_E2M1) return ts_scan_fp4_lds_bytes(L, qh);
  if (ts_use_f32_split(L, qh)) return ts_scan_f32s_lds_bytes(L);
  return (size_t)L.kg * qh * 1024 + sizeof(StageLds);
}

#if defined(TS_TUNING) && defined(DBG_NO_LDS)
template <int DT> using OpDense = OpNoLds<DT>;
#else
template <int DT> using OpDense = Op16<DT>;
#endif

int ts_launch_scan_masked(const TsLayout& L, int qh, const MaskedScanParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (L.dtype == TS_FP8_E4M3) return ts_launch_scan_masked_fp8(L, qh, p, num_cus, stream);
  if (L.dtype == TS_MXFP4_E2M1) return ts_launch_scan_masked_fp4(L, qh, p, num_cus, stream);
  if (ts_scan_lds_bytes(L, qh) > TS_LDS_BYTES) {
    ts_set_error("dimension %d too large for the LDS-resident query image", L.dim);
    return TS_ERR_UNSUPPORTED;
  }
  switch (L.dtype) {   // (fp32 storage: filtered searches take the dense path)
    case TS_F16: return launch_scan<Op16<TS_F16>, WalkLive>(SCAN_FILTER, qh, L.kg, p, num_cus, stream);
    case TS_BF16: return launch_scan<Op16<TS_BF16>, WalkLive>(SCAN_FILTER, qh, L.kg, p, num_cus, stream);
  }
  ts_set_error("the masked scan takes f16 / bf16 storage only");
  return TS_ERR_UNSUPPORTED;
}

int ts_launch_scan(const TsLayout& L, int mode, int qh, const ScanParams& p,
                   int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (L.dtype == TS_FP8_E4M3) return ts_launch_scan_fp8(L, mode, qh, p, num_cus, stream);
  if (L.dtype == TS_MXFP4_E2M1) return ts_launch_scan_fp4(L, mode, qh, p, num_cus, stream);
  if (ts_use_f32_split(L, qh)) return ts_launch_scan_f32s(L, mode, p, num_cus, stream);
  if (ts_scan_lds_bytes(L, qh) > TS_LDS_BYTES) {
    ts_set_error("dimension %d too large for the LDS-resident query image", L.dim);
    return TS_ERR_UNSUPPORTED;
  }
  switch (L.dtype) {
    case TS_F16: return launch_scan<OpDense<TS_F16>, WalkStrided>(mode, qh, L.kg, p, num_cus, stream);
    case TS_BF16: return launch_scan<OpDense<TS_BF16>, WalkStrided>(mode, qh, L.kg, p, num_cus, stream);
    case TS_F32: return launch_scan<OpDense<TS_F32>, WalkStrided>(mode, qh, L.kg, p, num_cus, stream);
  }
  ts_set_error("bad dtype %d", L.dtype);
  return TS_ERR_INVALID;
}

// ------------------------------------------------------------------ live-block list (filtered searches)
// Thread per row block b: OR of the pass's distinct masks at word b (bits at or beyond ntotal cleared),
// compacted into live[] with one atomic per wave (block order is kept inside a wave); per distinct mask
// the allowed rows are summed with one atomic per wave.  Thread t < 64 of workgroup 0 also publishes
// the pass's query -> mask tables for the scan and the threshold kernel.
__global__ __launch_bounds__(256) void live_blocks_kernel(const uint32_t* bits, int64_t words, TsMaskPass mp,
                                                          int64_t nblk, int64_t ntotal, TsMaskDev* md) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  if (blockIdx.x == 0 && tid < TS_MAX_Q) {
    md->qmask[tid] = mp.qmask[tid];
    md->qd[tid] = mp.qd[tid];
  }
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + tid;
  const bool in = b < nblk;
  // rows of block b below ntotal (only the last block is partial)
  const int64_t rows = in ? ntotal - b * TS_ROWS_PER_BLOCK : 0;
  const uint32_t valid = rows >= 32 ? ~0u : (rows > 0 ? ((1u << rows) - 1u) : 0u);
  uint32_t any = 0;
  for (int d = 0; d < mp.nd; ++d) {
    const uint32_t wd = in ? (bits[(int64_t)mp.dist[d] * words + b] & valid) : 0u;
    any |= wd;
    uint32_t c = (uint32_t)__builtin_popcount(wd);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off, 64);
    if (lane == 0 && c) atomicAdd(&md->popc[d], c);
  }
  if (mp.all_live) any = valid;
  const bool live = any != 0u;
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(live);
  if (bal == 0ull) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&md->nlive, (uint32_t)__builtin_popcountll(bal));
  base = (uint32_t)__shfl((int)base, 0, 64);
  if (live) {
    const uint32_t below = (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
    reinterpret_cast<int32_t*>(md + 1)[base + below] = (int32_t)b;
  }
}

int ts_launch_live_blocks(const uint32_t* bits, int64_t words, const TsMaskPass& mp, int64_t nblk,
                          int64_t ntotal, TsMaskDev* md, hipStream_t stream) {
  const int64_t blocks = (nblk + 255) / 256;
  if (blocks < 1 || blocks > 0x7fffffffLL) { ts_set_error("live blocks: bad row block count"); return TS_ERR_INVALID; }
  hipLaunchKernelGGL(live_blocks_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, bits, words, mp, nblk, ntotal, md);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// ------------------------------------------------------------------ layout
// den[i] = |row_i| + 1e-8  (reference src/stage1_retriever.py:285-288)
template <typename TIN>
__global__ void row_den_kernel(const TIN* rows, int64_t n, int dim, float* den) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= n) return;
  const TIN* src = rows + row * dim;
  float s = 0.f;
  for (int k = lane; k < dim; k += 64) {
    float v = ElemIO<TIN>::ld(src + k);
    s += v * v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) den[row] = sqrtf(s) + 1e-8f;
}

// One wave per (row block, k group): 64 lanes write one contiguous 1 KiB unit row.
template <typename TIN>
__global__ void relayout_kernel(const TIN* rows, int64_t n, int dim,
                                int64_t row0, int64_t blk_first, int64_t nunits_wave,
                                uint4* tiled, int kg, int dt, const float* den, int vec) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= nunits_wave) return;
  const int64_t b = blk_first + wv / kg;
  const int g = (int)(wv % kg);
  const int r = lane & 31, h = lane >> 5;
  const int64_t row = b * TS_ROWS_PER_BLOCK + r;
  if (row < row0 || row >= row0 + n) return;
  const TIN* src = rows + (row - row0) * dim;
  const float d = den ? den[row - row0] : 1.0f;
  u32x4 out;
  if (dt == TS_F32) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = frag_k(dt, g, h, e);
      float v = (k < dim) ? ElemIO<TIN>::ld(src + k) : 0.f;
      if (den) v = v / d;
      out[e] = __builtin_bit_cast(uint32_t, v);
    }
  } else if (vec) {
    // 16-bit storage: the unit's 8 values are consecutive in the row -> one (f32 rows: two)
    // 16-byte load instead of eight scalar ones (808 -> ~300 us per 500 k x 768 rows)
    const int k0 = frag_k(dt, g, h, 0);
    float v[8];
    if (k0 < dim) {
      ld8<TIN>(src + k0, v);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v0 = v[2 * e], v1 = v[2 * e + 1];
      if (den) { v0 = v0 / d; v1 = v1 / d; }
      out[e] = (uint32_t)f32_to_storage16(v0, dt) | ((uint32_t)f32_to_storage16(v1, dt) << 16);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k0 = frag_k(dt, g, h, 2 * e), k1 = k0 + 1;
      float v0 = (k0 < dim) ? ElemIO<TIN>::ld(src + k0) : 0.f;
      float v1 = (k1 < dim) ? ElemIO<TIN>::ld(src + k1) : 0.f;
      if (den) { v0 = v0 / d; v1 = v1 / d; }
      out[e] = (uint32_t)f32_to_storage16(v0, dt) |
               ((uint32_t)f32_to_storage16(v1, dt) << 16);
    }
  }
  reinterpret_cast<u32x4*>(tiled)[(size_t)(b * kg + g) * 64 + lane] = out;
}

// den[i] = |row_i| + 1e-8 of n rows: what every normalising relayout divides by
int ts_launch_row_den(const void* rows, int in_dtype, int64_t n, int dim, float* den, hipStream_t s) {
  const int blocks = (int)((n + 3) / 4);
  return ts_typed_rows(rows, in_dtype, [&](auto* r) -> int {
    typedef typename TsPointee<decltype(r)>::type TIN;
    hipLaunchKernelGGL(row_den_kernel<TIN>, dim3(blocks), dim3(256), 0, s, r, n, dim, den);
    TS_HIP(hipGetLastError());
    return TS_OK;
  });
}

int ts_launch_relayout(const TsLayout& L, const void* rows, int in_dtype, int64_t n,
                       int64_t row0, uint4* tiled, bool normalize,
                       float* den_scratch, hipStream_t stream) {
  if (n <= 0) return TS_OK;
  if (L.dtype == TS_FP8_E4M3)
    return ts_launch_relayout_fp8(L, rows, in_dtype, n, row0, tiled, normalize, den_scratch, stream);
  if (L.dtype == TS_MXFP4_E2M1)
    return ts_launch_relayout_fp4(L, rows, in_dtype, n, row0, tiled, normalize, den_scratch, stream);
  if (normalize) TS_CHECK(ts_launch_row_den(rows, in_dtype, n, L.dim, den_scratch, stream));
  return ts_typed_rows(rows, in_dtype, [&](auto* r) -> int {
    typedef typename TsPointee<decltype(r)>::type TIN;
    TsRelayoutGeom g;
    TS_CHECK(ts_relayout_geom(L.dim, L.kg, r, sizeof(TIN), row0, n, g));
    hipLaunchKernelGGL(relayout_kernel<TIN>, dim3(g.blocks), dim3(256), 0, stream, r, n, L.dim, row0, g.blk_first,
                       g.nwave, tiled, L.kg, L.dtype, normalize ? den_scratch : (const float*)nullptr,
                       (int)(L.dtype != TS_F32 && g.vec));   // (f32 storage has no vector path)
    TS_HIP(hipGetLastError());
    return TS_OK;
  });
}

__global__ void reconstruct_kernel(const uint4* tiled, int64_t row0, int64_t n,
                                   int dim, int kg, int dt, float* out) {
  // thread per (row, 16-byte unit)
  const int upr = kg * 2;  // units per row
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * upr) return;
  const int64_t row = row0 + t / upr;
  const int u = (int)(t % upr);
  const int g = u >> 1, h = u & 1;
  const int64_t b = row / TS_ROWS_PER_BLOCK;
  const int lane = h * 32 + (int)(row % TS_ROWS_PER_BLOCK);
  const u32x4 v = reinterpret_cast<const u32x4*>(tiled)[(size_t)(b * kg + g) * 64 + lane];
  float* dst = out + (row - row0) * dim;
  if (dt == TS_F32) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = frag_k(dt, g, h, e);
      const uint32_t w = v[e];
      if (k < dim) dst[k] = __uint_as_float(w);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = frag_k(dt, g, h, e);
      const uint16_t bits = (uint16_t)(v[e >> 1] >> (16 * (e & 1)));
      float f;
      if (dt == TS_F16) f = (float)__builtin_bit_cast(_Float16, bits);
      else f = __builtin_bit_cast(float, (uint32_t)bits << 16);
      if (k < dim) dst[k] = f;
    }
  }
}

int ts_launch_reconstruct(const TsLayout& L, const uint4* tiled, int64_t row0,
                          int64_t n, float* out, hipStream_t stream) {
  if (n <= 0) return TS_OK;
  if (L.dtype == TS_FP8_E4M3) return ts_launch_reconstruct_fp8(L, tiled, row0, n, out, stream);
  if (L.dtype == TS_MXFP4_E2M1) return ts_launch_reconstruct_fp4(L, tiled, row0, n, out, stream);
  unsigned blocks;
  TS_CHECK(ts_reconstruct_blocks(n, L.kg, blocks));
  hipLaunchKernelGGL(reconstruct_kernel, dim3(blocks), dim3(256), 0, stream,
                     tiled, row0, n, L.dim, L.kg, L.dtype, out);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// thread per 16-byte unit of the Q image
template <typename TIN>
__global__ void qprep_kernel(const TIN* q, int nq, int dim, int kg, int qh, int dt,
                             uint4* qimg, uint32_t* cand_cnt, uint32_t* status) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < TS_MAX_Q && cand_cnt) cand_cnt[t] = 0;
  if (t == 0 && status) status[0] = 0;
  if (t >= kg * qh * 64) return;
  const int lane = t & 63;
  const int hq = (t >> 6) % qh;
  const int g = (t >> 6) / qh;
  const int j = lane & 31, h = lane >> 5;
  const int qi = hq * 32 + j;
  const TIN* src = q + (int64_t)qi * dim;
  u32x4 out;
  if (dt == TS_F32) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = frag_k(dt, g, h, e);
      float v = (qi < nq && k < dim) ? ElemIO<TIN>::ld(src + k) : 0.f;
      out[e] = __builtin_bit_cast(uint32_t, v);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k0 = frag_k(dt, g, h, 2 * e), k1 = k0 + 1;
      float v0 = (qi < nq && k0 < dim) ? ElemIO<TIN>::ld(src + k0) : 0.f;
      float v1 = (qi < nq && k1 < dim) ? ElemIO<TIN>::ld(src + k1) : 0.f;
      out[e] = (uint32_t)f32_to_storage16(v0, dt) |
               ((uint32_t)f32_to_storage16(v1, dt) << 16);
    }
  }
  reinterpret_cast<u32x4*>(qimg)[t] = out;
}

int ts_launch_qprep(const TsLayout& L, const void* q, int q_dtype, int nq, int qh,
                    uint4* qimg, uint32_t* cand_cnt, uint32_t* status,
                    hipStream_t stream) {
  if (L.dtype == TS_FP8_E4M3) return ts_launch_qprep_fp8(L, q, q_dtype, nq, qh, qimg, cand_cnt, status, stream);
  if (L.dtype == TS_MXFP4_E2M1) return ts_launch_qprep_fp4(L, q, q_dtype, nq, qh, qimg, cand_cnt, status, stream);
  if (ts_use_f32_split(L, qh)) return ts_launch_qprep_f32s(L, q, q_dtype, nq, qimg, cand_cnt, status, stream);
  const int units = L.kg * qh * 64;
  const int blocks = (units + 255) / 256;
  return ts_typed_queries(q, q_dtype, [&](auto* qt) -> int {
    typedef typename TsPointee<decltype(qt)>::type TIN;
    hipLaunchKernelGGL(qprep_kernel<TIN>, dim3(blocks), dim3(256), 0, stream, qt, nq, L.dim, L.kg, qh, L.dtype, qimg,
                       cand_cnt, status);
    TS_HIP(hipGetLastError());
    return TS_OK;
  });
}
