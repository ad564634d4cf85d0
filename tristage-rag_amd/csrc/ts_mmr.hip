// Maximal marginal relevance over stored rows (ts_index_mmr / ts_mmr_ivf).
//
// Per query: C candidate ids with C relevances, k picks.  Step 0 picks the largest relevance; step t the unpicked
// candidate with the largest  lambda * rel_i - (1 - lambda) * max_{j picked} sim(i, j)  in f32, ties to the lower
// position; sim is the f32 inner product of the STORED rows.  Three kernels, all on the caller's stream:
//
//   gather   the candidates' 16-byte units out of the tiled corpus into a per-query candidate tile in the same
//            fragment order (32 candidates per workgroup; padding, unknown and removed ids are zero rows and are
//            marked invalid; IVF ids go through id2slot).  One kernel for every storage type: it moves units.
//   gram     S = X X^T per query on the matrix cores.  The A and B fragments of the 32x32 MFMAs have the same per-lane
//            shape, so a candidate tile is both operands.  A wave owns a 64 x 64 tile of S on or above the diagonal
//            (and writes its transpose): four 1 KiB loads feed four MFMAs (eight for e4m3) per k group.  Every 32 x 32 tile accumulates over the k groups in ascending order,
//            and the products of S[i][j] and S[j][i] are the same numbers in the same order: the same bits.
//   greedy   one workgroup per query, one thread per candidate; rel and the running max similarity in registers,
//            one coalesced row of S and one workgroup arg-max over (objective desc, position asc) per step.
//
// Scratch per query: the candidate tile (blocks * kg KiB), S (f32 [ld, ld], ld = 32 * blocks) and ld validity words,
// blocks = ceil(C / 32) rounded up to even.  A batch goes through it in chunks of queries (kMmrScratchCap).
#include <algorithm>
#include <math.h>

#include "ts_scan_dev.h"

namespace {

constexpr size_t kMmrScratchCap = 384u << 20;   // candidate tiles + Gram matrices of one chunk of queries: a 64-query
                                                // pass at C = 1024, d = 768, 16-bit rows (5.5 MiB each) is one chunk
constexpr int kMmrMaxC = 1024;
constexpr int kMmrRing = 4;                     // k groups the Gram kernel keeps in flight (divides TS_RING)
static_assert(TS_RING % kMmrRing == 0, "kg is a multiple of TS_RING");

struct MmrGatherParams {
  const uint4* corpus;
  const int64_t* ids;        // [nq, C] of the chunk
  int C, cbp, kg;
  int64_t ntotal, id_offset;
  const uint32_t* live;      // flat index with removed rows: its live words
  const int64_t* id2slot;    // IVF
  const uint32_t* blk_valid; // IVF
  uint4* tile;               // [nq][cbp][kg][64]
  int32_t* valid;            // [nq][32 * cbp]
};

// grid (cbp, nq): candidates 32 b .. 32 b + 31 of query q
template <bool IVF>
__global__ __launch_bounds__(256) void mmr_gather_kernel(MmrGatherParams p) {
  __shared__ int64_t srow[32];
  const int b = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  if (tid < 32) {
    const int c = b * 32 + tid;
    int64_t row = -1;
    if (c < p.C) {
      const int64_t id = p.ids[(int64_t)q * p.C + c];
      const int64_t r = id - p.id_offset;
      if (id != -1 && r >= 0 && r < p.ntotal) {
        if constexpr (IVF) {
          const int64_t s = p.id2slot[r];
          if (s >= 0 && ((p.blk_valid[s >> 5] >> (s & 31)) & 1u)) row = s;
        } else {
          if (!p.live || ((p.live[r >> 5] >> (r & 31)) & 1u)) row = r;
        }
      }
    }
    srow[tid] = row;
    p.valid[((int64_t)q * p.cbp + b) * 32 + tid] = row >= 0 ? 1 : 0;
  }
  __syncthreads();
  uint4* dst = p.tile + ((int64_t)q * p.cbp + b) * p.kg * 64;
  const int units = p.kg * 64;
  for (int u = tid; u < units; u += 256) {
    const int g = u >> 6, l = u & 63;
    const int64_t row = srow[l & 31];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row >= 0) v = p.corpus[((row >> 5) * p.kg + g) * 64 + (l & 32) + (row & 31)];
    dst[u] = v;
  }
}

// e4m3 bytes -> the bf16 fragment of one k step (the conversion of ts_scan_fp8.hip's fp8_frag: every e4m3 value is a
// bf16 value)
__device__ __forceinline__ u32x4 mmr_fp8_frag(uint32_t w0, uint32_t w1) {
  u32x4 o;
  o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
  o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
  o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
  o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
  return o;
}

template <int DT>
__device__ __forceinline__ void mmr_mma4(f32x16 (&acc)[2][2], const u32x4 (&a)[2], const u32x4 (&b)[2]) {
  if constexpr (DT == TS_FP8_E4M3) {
    u32x4 a0[2], b0[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {   // k steps 2g and 2g + 1, in that order
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a0[i] = mmr_fp8_frag(a[i][2 * m], a[i][2 * m + 1]);
        b0[i] = mmr_fp8_frag(b[i][2 * m], b[i][2 * m + 1]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mma_group<TS_BF16>(acc[i][j], a0[i], b0[j]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) mma_group<DT>(acc[i][j], a[i], b[j]);
  }
}

// grid (ceil(T (T + 1) / 2 / 4), nq), T = cbp / 2, 4 waves: a wave owns rows 64 ti .. +64, columns 64 tj .. +64 of S
// for one pair ti <= tj, and writes the tile's transpose too when ti < tj (the same registers: S is symmetric bit for
// bit; on the diagonal both halves are computed, from the same products in the same order)
template <int DT>
__global__ __launch_bounds__(256) void mmr_gram_kernel(const u32x4* tile, float* S, int cbp, int kg, float scale) {
  const int lane = threadIdx.x & 63;
  const int T = cbp >> 1;
  const int st = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (st >= T * (T + 1) / 2) return;
  int ti = 0, tj = st;
  while (tj >= T - ti) { tj -= T - ti; ++ti; }   // (wave-uniform: row ti of the upper triangle holds T - ti pairs)
  tj += ti;
  const int64_t q = blockIdx.y;
  const int ld = cbp * 32;
  const u32x4* base = tile + q * cbp * kg * 64 + lane;
  const u32x4* pa = base + (int64_t)(2 * ti) * kg * 64;
  const u32x4* pb = base + (int64_t)(2 * tj) * kg * 64;
  const int64_t blk = (int64_t)kg * 64;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // kMmrRing k groups of the four blocks stay in flight (16 loads of 1 KiB per wave): the tile comes from L2, and a
  // wave that waited for every group before its MFMAs spent its time on that latency.  kg is a multiple of TS_RING.
  u32x4 ra[kMmrRing][2], rb[kMmrRing][2];
#pragma unroll
  for (int i = 0; i < kMmrRing; ++i) {
    ra[i][0] = pa[(int64_t)i * 64];
    ra[i][1] = pa[blk + (int64_t)i * 64];
    rb[i][0] = pb[(int64_t)i * 64];
    rb[i][1] = pb[blk + (int64_t)i * 64];
  }
  for (int g0 = 0; g0 < kg; g0 += kMmrRing) {
#pragma unroll
    for (int i = 0; i < kMmrRing; ++i) {
      mmr_mma4<DT>(acc, ra[i], rb[i]);   // k group g0 + i: ascending order
      const int gn = g0 + kMmrRing + i;
      if (gn < kg) {
        ra[i][0] = pa[(int64_t)gn * 64];
        ra[i][1] = pa[blk + (int64_t)gn * 64];
        rb[i][0] = pb[(int64_t)gn * 64];
        rb[i][1] = pb[blk + (int64_t)gn * 64];
      }
    }
  }
  float* Sq = S + q * ld * ld;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = (2 * tj + j) * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (2 * ti + i) * 32 + acc_row(r, lane);
        Sq[(int64_t)row * ld + col] = acc[i][j][r] * scale;
      }
      if (ti != tj) {   // the transpose: a lane's registers 4 r4 .. 4 r4 + 3 are four consecutive columns of row `col`
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int row0 = (2 * ti + i) * 32 + acc_row(4 * r4, lane);
          float4 v;
          v.x = acc[i][j][4 * r4 + 0] * scale;
          v.y = acc[i][j][4 * r4 + 1] * scale;
          v.z = acc[i][j][4 * r4 + 2] * scale;
          v.w = acc[i][j][4 * r4 + 3] * scale;
          *reinterpret_cast<float4*>(Sq + (int64_t)col * ld + row0) = v;
        }
      }
    }
}

struct MmrGreedyParams {
  const int64_t* ids;     // [nq, C] of the chunk
  const float* rel;       // [nq, C]
  const float* S;         // [nq][ld][ld]
  const int32_t* valid;   // [nq][ld]
  int C, ld, k;
  float lam, oml;
  float* out_rel;         // [nq, k]
  int64_t* out_ids;
};

#define MMR_NONE 0x7fffffff

__device__ __forceinline__ void mmr_better(float& o, int& p, float o2, int p2) {
  if (p2 != MMR_NONE && (p == MMR_NONE || o2 > o || (o2 == o && p2 < p))) { o = o2; p = p2; }
}

// one workgroup per query, blockDim.x = C rounded up to 64
__global__ __launch_bounds__(1024) void mmr_greedy_kernel(MmrGreedyParams p) {
  __shared__ float s_obj[2][16];
  __shared__ int s_pos[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int64_t q = blockIdx.x;
  const bool in = tid < p.C;
  const float rel = in ? p.rel[q * p.C + tid] : 0.f;
  bool ok = in && p.valid[q * p.ld + tid] != 0;
  float maxsim = -INFINITY;
  const float* Sq = p.S + q * p.ld * p.ld;
  float* out_rel = p.out_rel + q * p.k;
  int64_t* out_ids = p.out_ids + q * p.k;
  for (int t = 0; t < p.k; ++t) {
    float o = t == 0 ? rel : __fsub_rn(__fmul_rn(p.lam, rel), __fmul_rn(p.oml, maxsim));
    if (!(o == o)) o = -INFINITY;   // a NaN objective ranks last
    int pos = ok ? tid : MMR_NONE;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const float o2 = __shfl_xor(o, d, 64);
      const int p2 = __shfl_xor(pos, d, 64);
      mmr_better(o, pos, o2, p2);
    }
    const int buf = t & 1;
    if (lane == 0) { s_obj[buf][wave] = o; s_pos[buf][wave] = pos; }
    __syncthreads();
    o = s_obj[buf][0];
    pos = s_pos[buf][0];
    for (int w = 1; w < nw; ++w) mmr_better(o, pos, s_obj[buf][w], s_pos[buf][w]);
    if (pos == MMR_NONE) {   // uniform: fewer than k valid candidates
      for (int u = t + tid; u < p.k; u += blockDim.x) { out_rel[u] = -3.402823466e38f; out_ids[u] = -1; }
      return;
    }
    if (tid == pos) {
      ok = false;
      out_rel[t] = rel;
      out_ids[t] = p.ids[q * p.C + tid];
    }
    if (ok) maxsim = fmaxf(maxsim, Sq[(int64_t)pos * p.ld + tid]);
  }
}

template <int DT>
int launch_gram(const u32x4* tile, float* S, int cbp, int kg, float scale, int nq, hipStream_t s) {
  const int T = cbp / 2;
  hipLaunchKernelGGL(mmr_gram_kernel<DT>, dim3((unsigned)((T * (T + 1) / 2 + 3) / 4), (unsigned)nq), dim3(256), 0, s, tile, S,
                     cbp, kg, scale);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

}  // namespace

int ts_mmr_check_args(const void* h, const void* cand_ids, const void* cand_rel, int32_t nq, int32_t fetch_k,
                      int32_t k, float lambda, const void* out_rel, const void* out_ids) {
  if (!h) { ts_set_error("mmr: null handle"); return TS_ERR_INVALID; }
  if (nq < 0) { ts_set_error("mmr: nq = %d", nq); return TS_ERR_INVALID; }
  if (k < 1 || k > fetch_k) { ts_set_error("mmr: k = %d must be in 1 .. fetch_k = %d", k, fetch_k); return TS_ERR_INVALID; }
  if (!(lambda >= 0.f && lambda <= 1.f)) { ts_set_error("mmr: lambda = %g is outside [0, 1]", (double)lambda); return TS_ERR_INVALID; }
  if (fetch_k > kMmrMaxC) {
    ts_set_error("mmr: fetch_k = %d exceeds %d (one thread per candidate)", fetch_k, kMmrMaxC);
    return TS_ERR_UNSUPPORTED;
  }
  if (nq > 0 && (!cand_ids || !cand_rel || !out_rel || !out_ids)) { ts_set_error("mmr: null pointer"); return TS_ERR_INVALID; }
  return TS_OK;
}

void ts_mmr_release(TsMmrWork& w) {
  if (w.scratch) (void)hipFree(w.scratch);
  if (w.stage) (void)hipFree(w.stage);
  if (w.ev) (void)hipEventDestroy(w.ev);
  for (hipEvent_t e : w.tev)
    if (e) (void)hipEventDestroy(e);
  w = TsMmrWork();
}

// The gather on its own (ts_index_rescore uses it too): candidates ids[q * C + c] of nq queries -> tile[q][cbp][kg][64]
// and valid[q][32 * cbp]; cbp >= ceil(C / 32).
int ts_launch_gather_tiles(const TsMmrSource& src, const int64_t* ids, int C, int cbp, int nq, uint4* tile,
                           int32_t* valid, hipStream_t s) {
  MmrGatherParams gp;
  gp.corpus = src.corpus;
  gp.ids = ids;
  gp.C = C; gp.cbp = cbp; gp.kg = src.L.kg;
  gp.ntotal = src.ntotal; gp.id_offset = src.id_offset;
  gp.live = src.live; gp.id2slot = src.id2slot; gp.blk_valid = src.blk_valid;
  gp.tile = tile; gp.valid = valid;
  if (src.ivf) hipLaunchKernelGGL(mmr_gather_kernel<true>, dim3(cbp, nq), dim3(256), 0, s, gp);
  else hipLaunchKernelGGL(mmr_gather_kernel<false>, dim3(cbp, nq), dim3(256), 0, s, gp);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

static int mmr_ensure(void*& p, size_t& have, size_t bytes) {
  if (p && have >= bytes) return TS_OK;
  if (p) { TS_HIP(hipFree(p)); p = nullptr; have = 0; }   // (hipFree waits for the work that still reads it)
  const size_t want = (bytes + 0xFFFFF) & ~(size_t)0xFFFFF;
  const hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) {
    p = nullptr;
    ts_set_error("mmr: hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
    return TS_ERR_OOM;
  }
  have = want;
  return TS_OK;
}

int ts_mmr_run(const TsMmrSource& src, TsMmrWork& w, const int64_t* cand_ids, const float* cand_rel, int32_t nq,
               int32_t C, int32_t k, float lambda, float* out_rel, int64_t* out_ids, uint32_t flags,
               hipStream_t s) {
  const TsLayout& L = src.L;
  if (L.dtype == TS_MXFP4_E2M1) {
    ts_set_error("mmr is not supported on a 4-bit MX (mxfp4) index");
    return TS_ERR_UNSUPPORTED;
  }
  const bool host = (flags & TS_FLAG_HOST_PTR) != 0;
  const size_t n_in = (size_t)nq * C, n_out = (size_t)nq * k;
  if (host) {   // the ids are readable here: an id that is neither padding nor a row of the index fails the call
    for (size_t i = 0; i < n_in; ++i) {
      const int64_t id = cand_ids[i];
      if (id != -1 && (id < src.id_offset || id - src.id_offset >= src.ntotal)) {
        ts_set_error("mmr: candidate id %lld (query %zu, position %zu) is outside [%lld, %lld)", (long long)id, i / C,
                     i % C, (long long)src.id_offset, (long long)(src.id_offset + src.ntotal));
        return TS_ERR_INVALID;
      }
    }
  }
  if (!w.ev) TS_HIP(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
  if (w.used) TS_HIP(hipStreamWaitEvent(s, w.ev, 0));   // the scratch is shared: calls on one handle run in order
  const int64_t* d_ids = cand_ids;
  const float* d_rel = cand_rel;
  float* d_orel = out_rel;
  int64_t* d_oids = out_ids;
  if (host) {
    const size_t b_ids = n_in * 8, b_oids = n_out * 8, b_rel = (n_in * 4 + 15) & ~(size_t)15;
    TS_CHECK(mmr_ensure(w.stage, w.stage_bytes, b_ids + b_oids + b_rel + n_out * 4));
    char* st = (char*)w.stage;
    d_ids = (int64_t*)st;
    d_oids = (int64_t*)(st + b_ids);
    d_rel = (float*)(st + b_ids + b_oids);
    d_orel = (float*)(st + b_ids + b_oids + b_rel);
    TS_HIP(hipMemcpyAsync((void*)d_ids, cand_ids, b_ids, hipMemcpyHostToDevice, s));
    TS_HIP(hipMemcpyAsync((void*)d_rel, cand_rel, n_in * 4, hipMemcpyHostToDevice, s));
  }
  const int cbp = 2 * ((C + 63) / 64);
  const int ld = cbp * 32;
  const size_t tile_b = (size_t)cbp * L.kg * 1024, s_b = (size_t)ld * ld * 4, v_b = (size_t)ld * 4;
  const size_t per_q = tile_b + s_b + v_b;
  const int qc = (int)std::max<size_t>(1, std::min<size_t>((size_t)nq, kMmrScratchCap / per_q));
  TS_CHECK(mmr_ensure(w.scratch, w.scratch_bytes, per_q * qc));
  uint4* tile = (uint4*)w.scratch;
  float* S = (float*)((char*)w.scratch + tile_b * qc);
  int32_t* valid = (int32_t*)((char*)w.scratch + (tile_b + s_b) * qc);
  // e4m3: a stored byte is x * 2^s, so a product of two rows carries 2^2s (an exact power of two on the f32 sum)
  const float scale = L.dtype == TS_FP8_E4M3 ? ldexpf(1.f, -2 * L.fp8_scale_log2) : 1.f;
  const int threads = std::max(64, ((C + 63) / 64) * 64);
  if (w.timing)
    for (hipEvent_t& e : w.tev)
      if (!e) TS_HIP(hipEventCreate(&e));
  for (int q0 = 0; q0 < nq; q0 += qc) {
    const int n = std::min(qc, nq - q0);
    if (w.timing) TS_HIP(hipEventRecord(w.tev[0], s));
    TS_CHECK(ts_launch_gather_tiles(src, d_ids + (size_t)q0 * C, C, cbp, n, tile, valid, s));
    if (w.timing) TS_HIP(hipEventRecord(w.tev[1], s));
    switch (L.dtype) {
      case TS_F16: TS_CHECK(launch_gram<TS_F16>((const u32x4*)tile, S, cbp, L.kg, scale, n, s)); break;
      case TS_BF16: TS_CHECK(launch_gram<TS_BF16>((const u32x4*)tile, S, cbp, L.kg, scale, n, s)); break;
      case TS_FP8_E4M3: TS_CHECK(launch_gram<TS_FP8_E4M3>((const u32x4*)tile, S, cbp, L.kg, scale, n, s)); break;
      default: TS_CHECK(launch_gram<TS_F32>((const u32x4*)tile, S, cbp, L.kg, scale, n, s)); break;
    }
    if (w.timing) TS_HIP(hipEventRecord(w.tev[2], s));
    MmrGreedyParams yp;
    yp.ids = d_ids + (size_t)q0 * C;
    yp.rel = d_rel + (size_t)q0 * C;
    yp.S = S; yp.valid = valid;
    yp.C = C; yp.ld = ld; yp.k = k;
    yp.lam = lambda; yp.oml = 1.f - lambda;
    yp.out_rel = d_orel + (size_t)q0 * k;
    yp.out_ids = d_oids + (size_t)q0 * k;
    hipLaunchKernelGGL(mmr_greedy_kernel, dim3(n), dim3(threads), 0, s, yp);
    TS_HIP(hipGetLastError());
    if (w.timing) {   // a measurement run: wait for the chunk and charge its three intervals
      TS_HIP(hipEventRecord(w.tev[3], s));
      TS_HIP(hipEventSynchronize(w.tev[3]));
      for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        TS_HIP(hipEventElapsedTime(&ms, w.tev[i], w.tev[i + 1]));
        w.phase_ms[i] += ms;
      }
    }
  }
  if (w.timing) ++w.timed_calls;
  if (host) {
    TS_HIP(hipMemcpyAsync(out_rel, d_orel, n_out * 4, hipMemcpyDeviceToHost, s));
    TS_HIP(hipMemcpyAsync(out_ids, d_oids, n_out * 8, hipMemcpyDeviceToHost, s));
    TS_HIP(hipStreamSynchronize(s));
  }
  TS_HIP(hipEventRecord(w.ev, s));
  w.used = true;
  return TS_OK;
}
