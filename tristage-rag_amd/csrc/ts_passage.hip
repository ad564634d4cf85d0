// Best passage per candidate on gfx950: windowed MaxSim over the rows of the resident token store
// (ts_maxsim_passages_indexed / _batch, include/tristage.h).
//
// Extends the reference's MaxSim (src/stage2_rescorer.py:167-183: S = normalize(Q) . normalize(D)^T, max over the
// document's tokens, mean over the query's) by a window: for query tokens q_t (t < Lq) and document tokens x_j
// (j < Ld) with c[t][j] = cos(q_t, x_j), width we = min(window, Ld) and positions p in [0, Ld - we],
//   S[p] = sum_t max_{p <= j < p + we} c[t][j]      p* = the lowest p with the largest S[p]
// and the outputs are p*, we, S[p*] / Lq and, if asked for, each query token's best j inside [p*, p* + we).
//
// One 256-thread workgroup per (query, candidate) pair, in rounds of QT query tokens:
//   * cosine tile: the four waves split the document's 32-row tiles.  Both operands are read row-major, in place, in
//     fragment order (lane (r, h): 16 bytes of row r at byte 32g + 16h of k step g; plain loads): the document rows
//     from the store, the round's query rows from the query matrix, which every workgroup of a launch shares and the
//     caches hold.  The k step is the one of ts_maxsim16.hip (m16_mma, m16_sumsq: ts_maxsim16_dev.h), the cosine is
//     (dot * 1/|x_j|) * 1/|q_t| as there, a zero row gives 0.  The tile goes to LDS as f32 c[QT][LDP], LDP odd (the
//     32 lanes of a half wave write 32 different banks).
//   * sliding maximum, per query token, in linear time (van Herk / Gil-Werman): blocks of we positions; g[j] = the
//     maximum of c from j to the end of j's block (one backward pass per block, into a second LDS array), then for
//     p = b * we + o the window maximum is max(g[p], max of c over the first o entries of block b + 1), the latter a
//     running maximum of one forward pass.  A maximum is exact: no bit depends on the method.
//   * window sums: thread p (+ 256 k) adds the round's maxima in ascending t into S[p], kept in registers across
//     the rounds.  The order of summation is therefore ascending t for every p: deterministic, no atomics.
//   * after the last round: arg-max over (S desc, p asc; a NaN sum last) by wave shuffles and one LDS slot per wave.
//   * alignment: one more pass over the rounds recomputes each cosine tile; wave w finds the arg-max of tokens
//     w, w + 4, ... inside the window (value desc, j asc).
// Two instantiations per element type: QT = 32 with LDP = 193 (documents of up to 192 rows, 48.8 KiB of LDS: three
// workgroups per CU) and QT = 16 with LDP = 1025 (up to 1024 rows, 128.7 KiB).  The lengths live on the device and the
// entry points do not synchronise, so every call launches both: a workgroup of the first takes its pair if the
// document has at most 192 rows; in the second, workgroup b of min(pairs, 1024) scans the lengths of the pairs
// b, b + grid, ... 64 at a time and takes the longer ones.
#include "ts_common.h"
#include "ts_maxsim16_dev.h"
#include <algorithm>

#define PSG_THREADS 256
#define PSG_WAVES 4
#define PSG_MAX_BATCH 64     // queries per launch (their offsets travel in the kernel arguments)
#define PSG_MAX_LQ 256
#define PSG_MAX_LD 1024
#define PSG_SMALL_LD 192
#define PSG_NEG (-3.402823466e38f)
#define PSG_KU 8             // k steps whose loads are issued together (12: 124 VGPRs, still three workgroups per CU,
                             // 4.87 against 4.73 ms at 64 x 1000 candidates — no gain; 16 costs a workgroup per CU)

struct PsgParams {
  const unsigned char* q;       // [sum Lq, H] rows of row_bytes
  const unsigned char* store;   // [rows, H]
  const int64_t* starts;
  const int32_t* lens;
  int row_bytes;
  int window;
  int32_t* out_start;
  int32_t* out_len;
  float* out_score;
  int32_t* out_align;           // null, or [pairs][align_ld]
  int align_ld;
  int nq;
  int32_t q_off[PSG_MAX_BATCH + 1];
  int32_t cand_off[PSG_MAX_BATCH + 1];
};

// (S desc, p asc), a NaN sum last: whether (sa, pa) ranks before (sb, pb)
__device__ __forceinline__ bool psg_before(float sa, int pa, float sb, int pb) {
  const bool na = sa != sa, nb = sb != sb;
  if (na || nb) return (na == nb) ? pa < pb : nb;
  return sa > sb || (sa == sb && pa < pb);
}

// LDS of one workgroup: c[QT][LDP], g[QT][LDP], 1/|x_j| of each wave's tile, the waves' arg-max slots, p*
template <int QT, int LDP> struct PsgLds {
  static constexpr size_t tile = (size_t)QT * LDP * 4;
  static constexpr size_t bytes = 2 * tile + PSG_WAVES * 32 * 4 + PSG_WAVES * 8 + 16;
};

// the cosine tile of query tokens [t0, t0 + QT) against the whole document -> c
template <int DT, int QT, int LDP>
__device__ __forceinline__ void psg_tile(const unsigned char* __restrict__ qb, int Lq, int t0,
                                         const unsigned char* __restrict__ doc, int Ld, int rb,
                                         float* __restrict__ c, float* __restrict__ myinv, int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  const int S = (rb + 31) >> 5;
  const int ndt = (Ld + 31) >> 5;
  const int qi = t0 + r;
  const unsigned char* qrow = qb + (size_t)(qi < Lq ? qi : Lq - 1) * rb;
  for (int dt = wave; dt < ndt; dt += PSG_WAVES) {
    const int dj = dt * 32 + r;
    const unsigned char* drow = doc + (size_t)(dj < Ld ? dj : Ld - 1) * rb;
    f32x16 acc;
#pragma unroll
    for (int x = 0; x < 16; ++x) acc[x] = 0.f;
    float dsq = 0.f, qsq = 0.f;
    for (int g0 = 0; g0 < S; g0 += PSG_KU) {
      u32x4 a[PSG_KU], b[PSG_KU];
      // always-issued loads from a valid address of the row, zeroed when consumed (no branch around a load)
#pragma unroll
      for (int i = 0; i < PSG_KU; ++i) {
        const int k = 32 * (g0 + i) + 16 * h;
        const int off = k < rb ? k : 0;
        a[i] = *reinterpret_cast<const u32x4*>(drow + off);
        b[i] = *reinterpret_cast<const u32x4*>(qrow + off);
      }
#pragma unroll
      for (int i = 0; i < PSG_KU; ++i) {
        const bool ok = 32 * (g0 + i) + 16 * h < rb;
        const u32x4 av = u32x4{ok ? a[i][0] : 0u, ok ? a[i][1] : 0u, ok ? a[i][2] : 0u, ok ? a[i][3] : 0u};
        const u32x4 bv = u32x4{ok ? b[i][0] : 0u, ok ? b[i][1] : 0u, ok ? b[i][2] : 0u, ok ? b[i][3] : 0u};
        dsq = m16_sumsq<DT>(av, dsq);
        qsq = m16_sumsq<DT>(bv, qsq);
        m16_mma<DT>(acc, av, bv);
      }
    }
    // accumulator column <-> query token (lane & 31), accumulator register x <-> document row (x & 3) + 8 (x >> 2)
    // + 4 h of the tile: 1/|x_j| reaches that layout through 128 bytes of wave-private LDS, as in ts_maxsim16.hip
    dsq += __shfl_xor(dsq, 32, 64);
    qsq += __shfl_xor(qsq, 32, 64);
    const float invq = 1.0f / fmaxf(sqrtf(qsq), 1e-12f);
    if (h == 0) myinv[r] = 1.0f / fmaxf(sqrtf(dsq), 1e-12f);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int x4 = 0; x4 < 4; ++x4) {
      const float4 iv = *reinterpret_cast<const float4*>(myinv + 8 * x4 + 4 * h);
      const int j = dt * 32 + 8 * x4 + 4 * h;
      if (r < QT) {
        float* row = c + (size_t)r * LDP + j;
        if (j + 0 < Ld) row[0] = (acc[4 * x4 + 0] * iv.x) * invq;
        if (j + 1 < Ld) row[1] = (acc[4 * x4 + 1] * iv.y) * invq;
        if (j + 2 < Ld) row[2] = (acc[4 * x4 + 2] * iv.z) * invq;
        if (j + 3 < Ld) row[3] = (acc[4 * x4 + 3] * iv.w) * invq;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// one (query, candidate) pair; 1 <= Ld <= LDP - 1, 1 <= Lq.  Every thread of the workgroup calls it.
template <int DT, int QT, int LDP>
__device__ __forceinline__ void psg_pair(const PsgParams& p, int pair, int Ld, unsigned char* smem) {
  constexpr int PPT = (LDP - 1 + PSG_THREADS - 1) / PSG_THREADS;   // window positions per thread
  float* c = reinterpret_cast<float*>(smem);
  float* g = c + (size_t)QT * LDP;
  float* winv = g + (size_t)QT * LDP;               // [waves][32]
  float* rs = winv + PSG_WAVES * 32;                // [waves] arg-max slots
  int* rp = reinterpret_cast<int*>(rs + PSG_WAVES); // [waves]
  int* pstar = rp + PSG_WAVES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int qj = 0;
  while (qj + 1 < p.nq && pair >= p.cand_off[qj + 1]) ++qj;     // (uniform; <= 64 steps over kernel arguments)
  const int Lq = p.q_off[qj + 1] - p.q_off[qj];
  const int rb = p.row_bytes;
  const unsigned char* qb = p.q + (size_t)p.q_off[qj] * rb;
  const unsigned char* doc = p.store + (size_t)p.starts[pair] * rb;
  const int we = min(p.window, Ld);
  const int npos = Ld - we + 1;
  const int nb = (Ld + we - 1) / we;
  float* myinv = winv + wave * 32;

  float S[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) S[k] = 0.f;

  for (int t0 = 0; t0 < Lq; t0 += QT) {
    const int nv = min(QT, Lq - t0);
    psg_tile<DT, QT, LDP>(qb, Lq, t0, doc, Ld, rb, c, myinv, wave, lane);
    __syncthreads();
    // g[j] = max of c[j .. end of j's block]
    for (int item = tid; item < nv * nb; item += PSG_THREADS) {
      const int t = item % nv, b = item / nv;
      const float* cr = c + (size_t)t * LDP;
      float* gr = g + (size_t)t * LDP;
      const int j0 = b * we, j1 = min(j0 + we, Ld);
      float run = cr[j1 - 1];
      gr[j1 - 1] = run;
      for (int j = j1 - 2; j >= j0; --j) {
        run = fmaxf(run, cr[j]);
        gr[j] = run;
      }
    }
    __syncthreads();
    // g[p] = max(g[p], max of c over the first o entries of the next block), p = b * we + o
    for (int item = tid; item < nv * nb; item += PSG_THREADS) {
      const int t = item % nv, b = item / nv;
      const float* cr = c + (size_t)t * LDP;
      float* gr = g + (size_t)t * LDP;
      const int p0 = b * we;
      const int o1 = min(we, npos - p0);     // positions p0 + o, o < o1, are windows
      if (o1 > 1) {
        float run = cr[p0 + we];
        gr[p0 + 1] = fmaxf(gr[p0 + 1], run);
        for (int o = 2; o < o1; ++o) {
          run = fmaxf(run, cr[p0 + we + o - 1]);
          gr[p0 + o] = fmaxf(gr[p0 + o], run);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int pos = tid + k * PSG_THREADS;
      if (pos < npos) {
        float s = S[k];
        for (int t = 0; t < nv; ++t) s += g[(size_t)t * LDP + pos];
        S[k] = s;
      }
    }
    // (the next round's tile writes c, which nobody reads any more; its first write of g comes after a barrier)
  }

  // ---- arg-max over (S desc, p asc)
  float bs = __builtin_nanf("");
  int bp = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int pos = tid + k * PSG_THREADS;
    if (pos < npos && psg_before(S[k], pos, bs, bp)) { bs = S[k]; bp = pos; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o, 64);
    const int op = __shfl_xor(bp, o, 64);
    if (psg_before(os, op, bs, bp)) { bs = os; bp = op; }
  }
  if (lane == 0) { rs[wave] = bs; rp[wave] = bp; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < PSG_WAVES; ++w)
      if (psg_before(rs[w], rp[w], bs, bp)) { bs = rs[w]; bp = rp[w]; }
    p.out_start[pair] = bp;
    p.out_len[pair] = we;
    p.out_score[pair] = bs / (float)Lq;
    *pstar = bp;
  }
  if (!p.out_align) return;     // (uniform)
  __syncthreads();
  const int ps = *pstar;
  int32_t* al = p.out_align + (size_t)pair * p.align_ld;
  for (int t = Lq + tid; t < p.align_ld; t += PSG_THREADS) al[t] = -1;
  for (int t0 = 0; t0 < Lq; t0 += QT) {
    const int nv = min(QT, Lq - t0);
    __syncthreads();            // the previous round's readers of c are done
    psg_tile<DT, QT, LDP>(qb, Lq, t0, doc, Ld, rb, c, myinv, wave, lane);
    __syncthreads();
    for (int t = wave; t < nv; t += PSG_WAVES) {
      const float* cr = c + (size_t)t * LDP;
      float bv = __builtin_nanf("");
      int bj = 0x7fffffff;
      for (int j = ps + lane; j < ps + we; j += 64) {
        const float v = cr[j];
        if (psg_before(v, j, bv, bj)) { bv = v; bj = j; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (psg_before(ov, oj, bv, bj)) { bv = ov; bj = oj; }
      }
      if (lane == 0) al[t0 + t] = bj;
    }
  }
}

// a candidate without rows: start -1, length 0, score -FLT_MAX, alignment -1; one with more than PSG_MAX_LD rows (the
// host cannot refuse it without reading the lengths back): the same with start -2
__device__ __forceinline__ void psg_refuse(const PsgParams& p, int pair, int start) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    p.out_start[pair] = start;
    p.out_len[pair] = 0;
    p.out_score[pair] = PSG_NEG;
  }
  if (p.out_align)
    for (int t = tid; t < p.align_ld; t += PSG_THREADS) p.out_align[(size_t)pair * p.align_ld + t] = -1;
}

// documents of 1 .. PSG_SMALL_LD rows (and the refusals): workgroup = pair
template <int DT>
__global__ __launch_bounds__(PSG_THREADS) void passage_small_kernel(PsgParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int pair = blockIdx.x;
  const int Ld = p.lens[pair];
  if (Ld <= 0 || Ld > PSG_MAX_LD) { psg_refuse(p, pair, Ld <= 0 ? -1 : -2); return; }
  if (Ld > PSG_SMALL_LD) return;     // passage_large_kernel's
  psg_pair<DT, 32, PSG_SMALL_LD + 1>(p, pair, Ld, smem);
}

// documents of PSG_SMALL_LD + 1 .. PSG_MAX_LD rows.  Workgroup b owns the pairs b, b + grid, b + 2 grid, ... (grid =
// min(pairs, 1024): up to 1024 pairs every pair has a workgroup of its own, and the long pairs of a larger call are
// spread over all of them) and looks at the lengths of 64 of its pairs at a time (each wave loads the same 64 lengths,
// so the set of pairs to do is uniform for the workgroup)
template <int DT>
__global__ __launch_bounds__(PSG_THREADS) void passage_large_kernel(PsgParams p, int pairs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const long long grid = gridDim.x;
  for (long long k0 = 0; blockIdx.x + k0 * grid < pairs; k0 += 64) {
    const long long i = blockIdx.x + (k0 + lane) * grid;
    const int len = i < pairs ? p.lens[i] : 0;
    uint64_t mask = __builtin_amdgcn_ballot_w64(len > PSG_SMALL_LD && len <= PSG_MAX_LD);
    while (mask) {
      const int bit = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int Ld = __builtin_amdgcn_readlane(len, bit);
      __syncthreads();           // the previous pair's LDS is no longer read
      psg_pair<DT, 16, PSG_MAX_LD + 1>(p, (int)(blockIdx.x + (k0 + bit) * grid), Ld, smem);
    }
  }
}

template <int DT>
static int psg_launch_t(const PsgParams& p, int pairs, hipStream_t s) {
  using Small = PsgLds<32, PSG_SMALL_LD + 1>;
  using Large = PsgLds<16, PSG_MAX_LD + 1>;
  static_assert(Small::bytes <= 53 * 1024, "three small workgroups per CU");
  static_assert(Large::bytes <= TS_LDS_BYTES, "the large tile fits the CU's LDS");
  hipLaunchKernelGGL(passage_small_kernel<DT>, dim3(pairs), dim3(PSG_THREADS), Small::bytes, s, p);
  TS_HIP(hipGetLastError());
  static TsDeviceOnce lds_attr;   // per instantiation, per device
  TS_CHECK(ts_allow_max_lds(lds_attr, reinterpret_cast<const void*>(passage_large_kernel<DT>)));
  const int grid = std::min(pairs, 1024);
  hipLaunchKernelGGL(passage_large_kernel<DT>, dim3(grid), dim3(PSG_THREADS), Large::bytes, s, p, pairs);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// argument checks shared by both entry points, before any HIP call
static int psg_check(const char* who, const void* q, const void* store, const void* starts, const void* lens,
                     const void* out_start, const void* out_len, const void* out_score, int32_t H, int32_t dtype,
                     int32_t window) {
  if (!q || !store || !starts || !lens || !out_start || !out_len || !out_score) {
    ts_set_error("%s: null pointer", who);
    return TS_ERR_INVALID;
  }
  if (window < 1) {
    ts_set_error("%s: window = %d, must be >= 1", who, window);
    return TS_ERR_INVALID;
  }
  if (H <= 0 || dtype < TS_F32 || dtype > TS_FP8_E4M3) {
    ts_set_error("%s: bad H = %d or dtype = %d", who, H, dtype);
    return TS_ERR_INVALID;
  }
  return TS_OK;
}
static int psg_check_shape(const char* who, const void* q, const void* store, int32_t H, int32_t dtype) {
  if (dtype == TS_FP8_E4M3) {
    ts_set_error("%s: an e4m3 token store is not supported", who);
    return TS_ERR_UNSUPPORTED;
  }
  const int64_t rb = (int64_t)H * (dtype == TS_F32 ? 4 : 2);
  if (rb % 16 != 0 || rb > (1 << 20)) {
    ts_set_error("%s: rows of %lld bytes (H = %d): a multiple of 16 bytes is needed", who, (long long)rb, H);
    return TS_ERR_UNSUPPORTED;
  }
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(store)) & 15) {
    ts_set_error("%s: q and store must be 16-byte aligned", who);
    return TS_ERR_UNSUPPORTED;
  }
  return TS_OK;
}

extern "C" int ts_maxsim_passages_indexed_batch(const void* q, const int32_t* q_off, int32_t nq, const void* store,
                                                const int64_t* starts, const int32_t* lens, const int32_t* cand_off,
                                                int32_t H, int32_t dtype, int32_t window, int32_t* out_start,
                                                int32_t* out_len, float* out_score, int32_t* out_align,
                                                int32_t align_ld, int32_t device, void* stream) {
  const char* who = "maxsim_passages_indexed_batch";
  TS_CHECK(psg_check(who, q, store, starts, lens, out_start, out_len, out_score, H, dtype, window));
  if (!q_off || !cand_off || nq < 0) {
    ts_set_error("%s: null offsets or nq = %d < 0", who, nq);
    return TS_ERR_INVALID;
  }
  int max_lq = 0;
  for (int j = 0; j < nq; ++j) {
    const int64_t lq = (int64_t)q_off[j + 1] - q_off[j], nc = (int64_t)cand_off[j + 1] - cand_off[j];
    if (lq < 0 || nc < 0) {
      ts_set_error("%s: offsets must be non-decreasing", who);
      return TS_ERR_INVALID;
    }
    if (nc > 0 && lq < 1) {
      ts_set_error("%s: query %d has candidates and no tokens", who, j);
      return TS_ERR_INVALID;
    }
    max_lq = (int)std::max<int64_t>(max_lq, std::min<int64_t>(lq, 1 << 30));
  }
  if (nq > 0 && (q_off[0] != 0 || cand_off[0] != 0)) {
    ts_set_error("%s: offsets must start at 0", who);
    return TS_ERR_INVALID;
  }
  if (out_align && align_ld < max_lq) {
    ts_set_error("%s: align_ld = %d is below the longest query (%d tokens)", who, align_ld, max_lq);
    return TS_ERR_INVALID;
  }
  if (max_lq > PSG_MAX_LQ) {
    ts_set_error("%s: a query of %d tokens (at most %d)", who, max_lq, PSG_MAX_LQ);
    return TS_ERR_UNSUPPORTED;
  }
  TS_CHECK(psg_check_shape(who, q, store, H, dtype));
  if (nq == 0 || cand_off[nq] == 0) return TS_OK;

  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  PsgParams p;
  p.row_bytes = H * (dtype == TS_F32 ? 4 : 2);
  p.window = window;
  p.store = (const unsigned char*)store;
  p.align_ld = out_align ? align_ld : 0;
  for (int j0 = 0; j0 < nq; j0 += PSG_MAX_BATCH) {     // (one pair of launches unless > 64 queries)
    const int nb = std::min(PSG_MAX_BATCH, nq - j0);
    const int qa = q_off[j0], ca = cand_off[j0];
    const int pairs = cand_off[j0 + nb] - ca;
    if (pairs == 0) continue;
    for (int j = 0; j <= nb; ++j) {
      p.q_off[j] = q_off[j0 + j] - qa;
      p.cand_off[j] = cand_off[j0 + j] - ca;
    }
    p.nq = nb;
    p.q = (const unsigned char*)q + (size_t)qa * p.row_bytes;
    p.starts = starts + ca;
    p.lens = lens + ca;
    p.out_start = out_start + ca;
    p.out_len = out_len + ca;
    p.out_score = out_score + ca;
    p.out_align = out_align ? out_align + (size_t)ca * align_ld : nullptr;
    int st;
    switch (dtype) {
      case TS_F16: st = psg_launch_t<TS_F16>(p, pairs, (hipStream_t)stream); break;
      case TS_BF16: st = psg_launch_t<TS_BF16>(p, pairs, (hipStream_t)stream); break;
      default: st = psg_launch_t<TS_F32>(p, pairs, (hipStream_t)stream); break;
    }
    TS_CHECK(st);
  }
  return TS_OK;
}

extern "C" int ts_maxsim_passages_indexed(const void* q, int32_t Lq, const void* store, const int64_t* starts,
                                          const int32_t* lens, int32_t n_docs, int32_t H, int32_t dtype,
                                          int32_t window, int32_t* out_start, int32_t* out_len, float* out_score,
                                          int32_t* out_align, int32_t device, void* stream) {
  const char* who = "maxsim_passages_indexed";
  TS_CHECK(psg_check(who, q, store, starts, lens, out_start, out_len, out_score, H, dtype, window));
  if (Lq < 1 || n_docs < 0) {
    ts_set_error("%s: Lq = %d (at least 1), n_docs = %d (at least 0)", who, Lq, n_docs);
    return TS_ERR_INVALID;
  }
  const int32_t q_off[2] = {0, Lq}, cand_off[2] = {0, n_docs};
  return ts_maxsim_passages_indexed_batch(q, q_off, 1, store, starts, lens, cand_off, H, dtype, window, out_start,
                                          out_len, out_score, out_align, Lq, device, stream);
}
