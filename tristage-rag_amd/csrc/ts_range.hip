// Range search: what follows the scans of ts_index_range_search.  Variable-length output in
// FAISS's CSR form, every query's rows in ascending id order.
//
//   small path   range_sort_kernel    the filter scan's (id, score) pairs of one query, sorted by id in LDS
//   dense path   range_count_kernel   survivors per (query, 1024-row tile) of a dense score chunk
//                range_prefix_kernel  exclusive prefix of a query's tile counts, its total
//                range_fill_kernel    the predicate again; survivor -> base + tile prefix + rank in tile
//
// Every global store is guarded by a count or a capacity that was computed before the launch (the scan's exact
// counts on the host, the tile counts of the count phase): an index that fails its guard is dropped, never written.
#include "ts_common.h"

#define RANGE_SORT_THREADS 1024
#define RANGE_TILE_THREADS 256
#define RANGE_PREFIX_THREADS 1024

// ------------------------------------------------------------------ small path
// One workgroup per query.  keys: id << 32 | score bits; ids are unique, so the order is total and the sort has no
// ties.  P (a power of two >= every count of the pass, <= 16384) keys of dynamic LDS; the tail is padded with ~0.
__global__ __launch_bounds__(RANGE_SORT_THREADS) void range_sort_kernel(TsRangeSortParams p, uint32_t P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long range_keys[];
  const int q = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  uint32_t n = p.cnt[q];
  if (n > p.cand_cap) n = p.cand_cap;   // (the host takes this path only when no count exceeds the cap)
  if (n > P) n = P;
  if (n == 0) return;                   // uniform
  const float* cs = p.cand_score + (size_t)q * p.cand_cap;
  const int32_t* ci = p.cand_id + (size_t)q * p.cand_cap;
  // only the power of two that covers this query's count is filled and sorted (Pq <= P: P covers every count)
  uint32_t Pq = 2;
  while (Pq < n) Pq <<= 1;
  for (uint32_t i = tid; i < Pq; i += RANGE_SORT_THREADS) {
    unsigned long long k = ~0ull;
    if (i < n) k = ((unsigned long long)(uint32_t)ci[i] << 32) | (unsigned long long)__float_as_uint(cs[i]);
    range_keys[i] = k;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= Pq; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t t = tid; t < (Pq >> 1); t += RANGE_SORT_THREADS) {
        const uint32_t i = 2 * t - (t & (stride - 1));
        const uint32_t j = i + stride;
        const bool asc = (i & size) == 0;
        const unsigned long long a = range_keys[i], b = range_keys[j];
        if (asc ? (a > b) : (b > a)) { range_keys[i] = b; range_keys[j] = a; }
      }
      __syncthreads();
    }
  }
  const int64_t base = p.off[q];
  for (uint32_t i = tid; i < n; i += RANGE_SORT_THREADS) {
    const int64_t pos = base + (int64_t)i;
    if (pos < p.off[q + 1] && pos < p.capacity) {
      const unsigned long long k = range_keys[i];
      p.out_scores[pos] = __uint_as_float((uint32_t)k);
      p.out_ids[pos] = (int64_t)(k >> 32) + p.id_offset;
    }
  }
}

int ts_launch_range_sort(const TsRangeSortParams& p, int nq, uint32_t max_count, hipStream_t stream) {
  if (nq <= 0 || max_count == 0) return TS_OK;
  if (nq > TS_MAX_Q || max_count > p.cand_cap || p.cand_cap > TS_SEL_LDS_KEYS) {
    ts_set_error("range sort: %d queries / %u entries are more than one pass holds", nq, max_count);
    return TS_ERR_INVALID;
  }
  uint32_t P = 2;
  while (P < max_count) P <<= 1;
  static TsDeviceOnce lds_attr;
  TS_CHECK(ts_allow_max_lds(lds_attr, reinterpret_cast<const void*>(range_sort_kernel)));
  hipLaunchKernelGGL(range_sort_kernel, dim3(nq), dim3(RANGE_SORT_THREADS), (size_t)P * 8, stream, p, P);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// ------------------------------------------------------------------ dense path
// A tile is TS_RANGE_TILE consecutive rows of a dense score chunk; thread t of its workgroup owns rows 4t .. 4t + 3.
// bit j of the result: row 4t + j of the tile survives (score >= radius, row inside the chunk, allowed).  NaN scores
// fail the comparison; the -FLT_MAX the dense scan writes behind ntotal is cut off by `rows`.
__device__ __forceinline__ uint32_t range_pred4(const TsRangeDenseParams& p, int q, uint32_t i0) {
  if (i0 >= p.rows) return 0u;
  const float r = p.radius[q];
  const float4 s = *reinterpret_cast<const float4*>(p.dense + (int64_t)q * p.ld + i0);
  uint32_t m = (s.x >= r ? 1u : 0u) | (s.y >= r ? 2u : 0u) | (s.z >= r ? 4u : 0u) | (s.w >= r ? 8u : 0u);
  if (p.mids) {
    const int4 a = *reinterpret_cast<const int4*>(p.mids + (int64_t)q * p.ld + i0);
    m &= (a.x >= 0 ? 1u : 0u) | (a.y >= 0 ? 2u : 0u) | (a.z >= 0 ? 4u : 0u) | (a.w >= 0 ? 8u : 0u);
  }
  const uint32_t left = p.rows - i0;   // >= 1
  if (left < 4) m &= (1u << left) - 1u;
  return m;
}

__global__ __launch_bounds__(RANGE_TILE_THREADS) void range_count_kernel(TsRangeDenseParams p) {
  __shared__ uint32_t wsum[RANGE_TILE_THREADS / 64];
  const int q = blockIdx.y;
  const uint32_t tile = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t m = range_pred4(p, q, tile * TS_RANGE_TILE + 4 * tid);
  uint32_t c = (uint32_t)__builtin_popcount(m);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = c;
  __syncthreads();
  if (tid == 0 && tile < p.chunk_tiles && p.tile0 + tile < p.ntiles)
    p.tilecnt[(int64_t)q * p.ntiles + p.tile0 + tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup per query: tilecnt[q][0 .. ntiles) becomes its exclusive prefix, total[q] the sum.
__global__ __launch_bounds__(RANGE_PREFIX_THREADS) void range_prefix_kernel(uint32_t* tilecnt, int64_t ntiles,
                                                                            uint32_t* total) {
  __shared__ uint32_t wsum[RANGE_PREFIX_THREADS / 64];
  __shared__ uint32_t carry_s;
  const int q = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63, wv = tid >> 6;
  uint32_t* row = tilecnt + (int64_t)q * ntiles;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int64_t i0 = 0; i0 < ntiles; i0 += RANGE_PREFIX_THREADS) {
    const int64_t i = i0 + tid;
    const uint32_t v = i < ntiles ? row[i] : 0u;
    uint32_t inc = v;   // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)inc, off, 64);
      if (lane >= (uint32_t)off) inc += o;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = carry_s;
    for (uint32_t w = 0; w < wv; ++w) before += wsum[w];
    if (i < ntiles) row[i] = before + inc - v;
    __syncthreads();
    if (tid == RANGE_PREFIX_THREADS - 1) carry_s = before + inc;
    __syncthreads();
  }
  if (tid == 0) total[q] = carry_s;
}

// The predicate of range_count_kernel again; a survivor's place is the query's offset + its tile's prefix + its rank
// inside the tile (ballot / popcount over the wave, the waves' sums through LDS), so the rows come out in ascending id.
__global__ __launch_bounds__(RANGE_TILE_THREADS) void range_fill_kernel(TsRangeDenseParams p) {
  __shared__ uint32_t wsum[RANGE_TILE_THREADS / 64];
  const int q = blockIdx.y;
  const uint32_t tile = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63, wv = tid >> 6;
  const uint32_t i0 = tile * TS_RANGE_TILE + 4 * tid;
  const uint32_t m = range_pred4(p, q, i0);
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t rank = 0, wave_total = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned long long b = __builtin_amdgcn_ballot_w64((m >> j) & 1u);
    rank += (uint32_t)__builtin_popcountll(b & below);
    wave_total += (uint32_t)__builtin_popcountll(b);
  }
  if (lane == 0) wsum[wv] = wave_total;
  __syncthreads();
  for (uint32_t w = 0; w < wv; ++w) rank += wsum[w];
  if (m == 0u || tile >= p.chunk_tiles || p.tile0 + tile >= p.ntiles) return;
  const int64_t end = p.off[q + 1];
  int64_t pos = p.off[q] + (int64_t)p.tilecnt[(int64_t)q * p.ntiles + p.tile0 + tile] + (int64_t)rank;
  const float4 s = *reinterpret_cast<const float4*>(p.dense + (int64_t)q * p.ld + i0);
  const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if ((m >> j) & 1u) {
      if (pos < end && pos < p.capacity) {
        p.out_scores[pos] = sv[j];
        p.out_ids[pos] = p.row0 + (int64_t)i0 + j + p.id_offset;
      }
      ++pos;
    }
  }
}

static int range_dense_check(const TsRangeDenseParams& p, int nq) {
  if (nq <= 0 || nq > TS_MAX_Q || p.rows == 0 || (p.ld & 3) || p.chunk_tiles == 0 ||
      (int64_t)p.chunk_tiles * TS_RANGE_TILE < (int64_t)p.rows || p.tile0 + p.chunk_tiles > p.ntiles) {
    ts_set_error("range search: bad dense chunk geometry");
    return TS_ERR_INVALID;
  }
  return TS_OK;
}

int ts_launch_range_count(const TsRangeDenseParams& p, int nq, hipStream_t stream) {
  TS_CHECK(range_dense_check(p, nq));
  hipLaunchKernelGGL(range_count_kernel, dim3(p.chunk_tiles, nq), dim3(RANGE_TILE_THREADS), 0, stream, p);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

int ts_launch_range_prefix(uint32_t* tilecnt, int64_t ntiles, int nq, uint32_t* total, hipStream_t stream) {
  if (nq <= 0 || nq > TS_MAX_Q || ntiles <= 0) { ts_set_error("range search: bad prefix geometry"); return TS_ERR_INVALID; }
  hipLaunchKernelGGL(range_prefix_kernel, dim3(nq), dim3(RANGE_PREFIX_THREADS), 0, stream, tilecnt, ntiles, total);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

int ts_launch_range_fill(const TsRangeDenseParams& p, int nq, hipStream_t stream) {
  TS_CHECK(range_dense_check(p, nq));
  hipLaunchKernelGGL(range_fill_kernel, dim3(p.chunk_tiles, nq), dim3(RANGE_TILE_THREADS), 0, stream, p);
  TS_HIP(hipGetLastError());
  return TS_OK;
}
