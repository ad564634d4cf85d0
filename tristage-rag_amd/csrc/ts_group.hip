// Grouped search: the collapse of a ranked candidate list to its first k distinct groups, at most group_size entries
// of each (ts_group_topk).
//
// Per query: C entries (id, score) in rank order and a table groups[row] shared by all queries.  An entry is VALID when
// id != -1 and 0 <= id - id_base < n_rows; its group is groups[id - id_base], a negative table value making the entry a
// group of its own.  Walking the list in position order, occ(i) = earlier valid entries of i's group and rank(i) =
// distinct groups whose first entry comes before the first entry of i's group; entry i is kept iff rank(i) < k and
// occ(i) < group_size.  Kept entries come out in ascending position, padded with -FLT_MAX / -1 / -1.  No score is ever
// compared.
//
// One workgroup per query, one launch, everything between the reads of the list and the writes of the result in LDS:
//
//   keys     key(i) = group key << 32 | i for position i: the table value of a grouped entry, 0x80000000 | i for an
//            ungrouped one (unique to its position), 0xFFFFFFFF for an invalid entry and for the padding up to the next
//            power of two (they sort last).  ids are read coalesced, the table is gathered.
//   sort     bitonic, ascending, in LDS (three distances per pass in registers, eight keys per thread).  The keys are
//            distinct, so the order is total and the result does not depend on the schedule.  Afterwards a group is a
//            run of keys with its positions ascending: the first key of the run is the group's first entry, and an
//            entry's distance from it is occ.
//   first    a flag bit per POSITION for every run's first key, then a prefix over the flag words: the number of set
//            bits below position p is the rank of the group that starts at p, and their total is n_groups.
//   keep     per sorted key: the run's start by a lower-bound search for the group key, rank through the flag prefix,
//            a second flag bit per position where rank < k and occ < group_size; its prefix is the output slot.
//   write    per kept position (coalesced over the list again): id, score and the table value to its slot.
//
// The flag bits are set with LDS atomic ORs (commutative: no dependence on the order).  No global atomics, no scratch,
// no host round trip; LDS is 8 n + 16 ceil(n / 32) + 128 bytes for n = C rounded up to a power of two (>= 8),
// 136.1 KiB at 16384 (a workgroup may hold all 160 KiB of an MI355X CU).
#include <float.h>

#include "ts_common.h"

namespace {

constexpr int kGroupMaxC = 16384;          // TS_SEL_LDS_KEYS: what ts_index_search returns at most per query
constexpr uint32_t kGroupInvalid = 0xFFFFFFFFu;
constexpr uint32_t kGroupSingle = 0x80000000u;

struct GroupParams {
  const int64_t* ids;       // [nq, C]
  const float* scores;      // [nq, C]
  const int32_t* groups;    // [n_rows]
  int64_t n_rows, id_base;
  int C, n;                 // n: C rounded up to a power of two, at least 8
  int k, group_size;
  float* out_scores;        // [nq, k * group_size]
  int64_t* out_ids;
  int32_t* out_groups;
  int32_t* out_ngroups;     // [nq]
  int32_t* out_nvalid;
};

__device__ __forceinline__ bool group_valid_row(int64_t id, int64_t id_base, int64_t n_rows, int64_t* row) {
  if (id == -1 || id < id_base) return false;
  const uint64_t r = (uint64_t)id - (uint64_t)id_base;   // id >= id_base: the difference is exact in 64 unsigned bits
  if (r >= (uint64_t)n_rows) return false;
  *row = (int64_t)r;
  return true;
}

// first index of keys[0, n) that is not below `key`
__device__ __forceinline__ int group_lower_bound(const uint64_t* keys, int n, uint64_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// orders a and b: ascending when up
__device__ __forceinline__ void group_cx(uint64_t& a, uint64_t& b, bool up) {
  const bool sw = (a > b) == up;
  const uint64_t x = sw ? b : a, y = sw ? a : b;
  a = x;
  b = y;
}

// NS consecutive distances of block k2 in one pass, in registers: a thread takes the 2^NS keys base + m * jlow and
// does the distances 2^(NS-1) jlow .. jlow on them (register distances 2^(NS-1) .. 1); base runs over the indices
// whose NS bits from jlow upwards are zero.  k2 >= 2^NS jlow, so the keys of a set share their direction.
template <int THREADS, int NS>
__device__ __forceinline__ void group_sort_pass(uint64_t* keys, int n, int jlow, int k2) {
  constexpr int K = 1 << NS;
  for (int r = threadIdx.x; r < (n >> NS); r += THREADS) {
    const int base = ((r & ~(jlow - 1)) << NS) | (r & (jlow - 1));
    uint64_t e[K];
#pragma unroll
    for (int m = 0; m < K; ++m) e[m] = keys[base + m * jlow];
    const bool up = (base & k2) == 0;
#pragma unroll
    for (int j = K >> 1; j >= 1; j >>= 1)
#pragma unroll
      for (int i = 0; i < K; ++i)
        if ((i & j) == 0) group_cx(e[i], e[i | j], up);
#pragma unroll
    for (int m = 0; m < K; ++m) keys[base + m * jlow] = e[m];
  }
}

// Blocks 2, 4 and 8 of the network (its first six distances) on every aligned run of eight keys of keys[0, n), n >= 8.
template <int THREADS>
__device__ __forceinline__ void group_sort_head(uint64_t* keys, int n) {
  for (int r = threadIdx.x; r < (n >> 3); r += THREADS) {
    uint64_t* base = keys + (r << 3);
    uint64_t e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = base[i];
#pragma unroll
    for (int i = 0; i < 8; i += 2) group_cx(e[i], e[i + 1], (i & 2) == 0);
#pragma unroll
    for (int j = 2; j >= 1; j >>= 1)
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if ((i & j) == 0) group_cx(e[i], e[i | j], (i & 4) == 0);
    const bool up = (r & 1) == 0;
#pragma unroll
    for (int j = 4; j >= 1; j >>= 1)
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if ((i & j) == 0) group_cx(e[i], e[i | j], up);
#pragma unroll
    for (int i = 0; i < 8; ++i) base[i] = e[i];
  }
}

// pre[w] = set bits of bits[0, w), for the nw <= THREADS words; returns their total.  wsum: one word per wave.
template <int THREADS>
__device__ __forceinline__ int group_bit_prefix(const uint32_t* bits, uint32_t* pre, int nw, uint32_t* wsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v = tid < nw ? __popc(bits[tid]) : 0;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  if (lane == 63) wsum[wave] = (uint32_t)inc;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const int s = (int)wsum[w];
    if (w < wave) base += s;
    total += s;
  }
  if (tid < nw) pre[tid] = (uint32_t)(base + inc - v);
  __syncthreads();
  return total;
}

__device__ __forceinline__ int group_bits_below(const uint32_t* bits, const uint32_t* pre, int p) {
  return (int)pre[p >> 5] + __popc(bits[p >> 5] & ((1u << (p & 31)) - 1u));
}

// grid nq, THREADS threads, dynamic LDS group_lds_bytes(n)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void group_topk_kernel(GroupParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char group_smem[];
  const int tid = threadIdx.x, n = p.n, C = p.C;
  const int nw = (n + 31) >> 5;
  uint64_t* keys = reinterpret_cast<uint64_t*>(group_smem);
  uint32_t* fbits = reinterpret_cast<uint32_t*>(keys + n);   // position p starts a group
  uint32_t* fpre = fbits + nw;
  uint32_t* kbits = fpre + nw;                               // position p is kept
  uint32_t* kpre = kbits + nw;
  uint32_t* wsum = kpre + nw;                                // [2][16]
  const int64_t q = blockIdx.x;
  const int64_t* ids = p.ids + q * C;
  const float* scores = p.scores + q * C;

  for (int w = tid; w < nw; w += THREADS) { fbits[w] = 0u; kbits[w] = 0u; }
  // eight ids, then their eight table entries, in flight per thread: the second read depends on the first, and a
  // thread that took them one entry at a time would wait out both latencies sixteen times at C = 16384
  constexpr int U = 8;
  for (int i0 = tid; i0 < n; i0 += THREADS * U) {
    int64_t id[U];
    int32_t g[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * THREADS;
      id[u] = i < C ? ids[i] : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int64_t row = 0;
      ok[u] = group_valid_row(id[u], p.id_base, p.n_rows, &row);
      g[u] = ok[u] ? p.groups[row] : 0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * THREADS;
      const uint32_t hi = !ok[u] ? kGroupInvalid : g[u] >= 0 ? (uint32_t)g[u] : (kGroupSingle | (uint32_t)i);
      if (i < n) keys[i] = ((uint64_t)hi << 32) | (uint32_t)i;
    }
  }
  __syncthreads();

  // Bitonic network, ascending: block k2 = 2^m has the m distances k2 / 2 .. 1.  A pass does three consecutive
  // distances on eight keys per thread in registers (the m % 3 left over first, on two or four keys): 38 passes over
  // the LDS and as many barriers for the 105 distances of n = 16384.
  group_sort_head<THREADS>(keys, n);
  __syncthreads();
  for (int k2 = 16, m = 4; k2 <= n; k2 <<= 1, ++m) {
    int left = m;
    const int first = m % 3;
    if (first == 1) group_sort_pass<THREADS, 1>(keys, n, k2 >> 1, k2);
    if (first == 2) group_sort_pass<THREADS, 2>(keys, n, k2 >> 2, k2);
    if (first != 0) __syncthreads();
    left -= first;
    while (left > 0) {
      left -= 3;
      group_sort_pass<THREADS, 3>(keys, n, 1 << left, k2);
      __syncthreads();
    }
  }

  // every valid entry sorts below the first invalid key
  const int n_valid = group_lower_bound(keys, n, (uint64_t)kGroupInvalid << 32);
  for (int s = tid; s < n_valid; s += THREADS) {
    const uint64_t key = keys[s];
    if (s == 0 || (uint32_t)(keys[s - 1] >> 32) != (uint32_t)(key >> 32)) {
      const uint32_t pos = (uint32_t)key;
      atomicOr(&fbits[pos >> 5], 1u << (pos & 31));
    }
  }
  __syncthreads();
  const int n_groups = group_bit_prefix<THREADS>(fbits, fpre, nw, wsum);

  for (int s = tid; s < n_valid; s += THREADS) {
    const uint64_t key = keys[s];
    const uint32_t hi = (uint32_t)(key >> 32), pos = (uint32_t)key;
    int start = s;
    if (s > 0 && (uint32_t)(keys[s - 1] >> 32) == hi) start = group_lower_bound(keys, s, (uint64_t)hi << 32);
    const int first = (int)(uint32_t)keys[start];
    if (s - start < p.group_size && group_bits_below(fbits, fpre, first) < p.k)
      atomicOr(&kbits[pos >> 5], 1u << (pos & 31));
  }
  __syncthreads();
  const int n_kept = group_bit_prefix<THREADS>(kbits, kpre, nw, wsum + 16);

  const int64_t out_n = (int64_t)p.k * p.group_size;
  float* out_scores = p.out_scores + q * out_n;
  int64_t* out_ids = p.out_ids + q * out_n;
  int32_t* out_groups = p.out_groups + q * out_n;
  for (int i = tid; i < C; i += THREADS) {
    if (!((kbits[i >> 5] >> (i & 31)) & 1u)) continue;
    const int slot = group_bits_below(kbits, kpre, i);   // < n_kept <= k * group_size
    const int64_t id = ids[i];
    int64_t row;
    // (a kept entry is valid and there are at most k * group_size of them: both accesses stay guarded all the same)
    if (slot >= out_n || !group_valid_row(id, p.id_base, p.n_rows, &row)) continue;
    const int32_t g = p.groups[row];
    out_scores[slot] = scores[i];
    out_ids[slot] = id;
    out_groups[slot] = g >= 0 ? g : -1;
  }
  for (int64_t u = n_kept + tid; u < out_n; u += THREADS) {
    out_scores[u] = -FLT_MAX;
    out_ids[u] = -1;
    out_groups[u] = -1;
  }
  if (tid == 0) {
    p.out_ngroups[q] = n_groups;
    p.out_nvalid[q] = n_valid;
  }
}

size_t group_lds_bytes(int n) {
  const size_t nw = ((size_t)n + 31) / 32;
  return (size_t)n * 8 + 4 * nw * 4 + 2 * 16 * 4;
}

TsDeviceOnce g_group_lds_once;

// Size classes by the sorted length n: up to 1024 keys a 256-thread workgroup, above that 1024 threads; above 4096
// keys the LDS request passes the 64 KiB a kernel gets by default and the attribute is set once per device.
int group_launch(const GroupParams& p, int nq, hipStream_t s) {
  const size_t lds = group_lds_bytes(p.n);
  if (p.n <= 1024) {
    hipLaunchKernelGGL(group_topk_kernel<256>, dim3((unsigned)nq), dim3(256), lds, s, p);
  } else {
    if (p.n > 4096) TS_CHECK(ts_allow_max_lds(g_group_lds_once, (const void*)group_topk_kernel<1024>));
    hipLaunchKernelGGL(group_topk_kernel<1024>, dim3((unsigned)nq), dim3(1024), lds, s, p);
  }
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// frees the staging of a host-pointer call on every way out
struct GroupStage {
  void* p = nullptr;
  ~GroupStage() { if (p) (void)hipFree(p); }
};

size_t group_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" int ts_group_topk(const int64_t* cand_ids, const float* cand_scores, int32_t nq, int32_t ncand,
                             const int32_t* groups, int64_t n_rows, int64_t id_base, int32_t k, int32_t group_size,
                             float* out_scores, int64_t* out_ids, int32_t* out_groups, int32_t* out_ngroups,
                             int32_t* out_nvalid, uint32_t flags, int32_t device, void* stream) {
  if (nq < 0) { ts_set_error("group: nq = %d", nq); return TS_ERR_INVALID; }
  if (ncand < 1) { ts_set_error("group: ncand = %d must be positive", ncand); return TS_ERR_INVALID; }
  if (k < 1 || group_size < 1) {
    ts_set_error("group: k = %d and group_size = %d must be positive", k, group_size);
    return TS_ERR_INVALID;
  }
  if (n_rows < 0) { ts_set_error("group: n_rows = %lld", (long long)n_rows); return TS_ERR_INVALID; }
  if (ncand > kGroupMaxC) {
    ts_set_error("group: ncand = %d exceeds %d (one workgroup sorts a query's list in LDS)", ncand, kGroupMaxC);
    return TS_ERR_UNSUPPORTED;
  }
  if ((int64_t)k * group_size > kGroupMaxC) {
    ts_set_error("group: k * group_size = %lld exceeds %d", (long long)k * group_size, kGroupMaxC);
    return TS_ERR_UNSUPPORTED;
  }
  if (nq == 0) return TS_OK;
  if (!cand_ids || !cand_scores || !groups || !out_scores || !out_ids || !out_groups || !out_ngroups || !out_nvalid) {
    ts_set_error("group: null pointer");
    return TS_ERR_INVALID;
  }
  const bool host = (flags & TS_FLAG_HOST_PTR) != 0;
  const size_t n_in = (size_t)nq * ncand, n_out = (size_t)nq * k * group_size;
  if (host) {   // the ids are readable here: an id that is neither padding nor a row of the table fails the call
    for (size_t i = 0; i < n_in; ++i) {
      const int64_t id = cand_ids[i];
      if (id != -1 && (id < id_base || (uint64_t)id - (uint64_t)id_base >= (uint64_t)n_rows)) {
        ts_set_error("group: candidate id %lld (query %zu, position %zu) is outside [%lld, %lld + %lld)", (long long)id,
                     i / ncand, i % ncand, (long long)id_base, (long long)id_base, (long long)n_rows);
        return TS_ERR_INVALID;
      }
    }
  }
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  hipStream_t s = (hipStream_t)stream;
  GroupParams p;
  p.ids = cand_ids; p.scores = cand_scores; p.groups = groups;
  p.n_rows = n_rows; p.id_base = id_base;
  p.C = ncand;
  p.n = 8;   // (the sort works on runs of eight keys)
  while (p.n < ncand) p.n <<= 1;
  p.k = k; p.group_size = group_size;
  p.out_scores = out_scores; p.out_ids = out_ids; p.out_groups = out_groups;
  p.out_ngroups = out_ngroups; p.out_nvalid = out_nvalid;
  if (!host) return group_launch(p, nq, s);

  // host pointers: one staging block for the call, freed before it returns (the entry point keeps no state)
  const size_t b_ids = group_align(n_in * 8), b_sc = group_align(n_in * 4), b_tab = group_align((size_t)n_rows * 4 + 4);
  const size_t b_oid = group_align(n_out * 8), b_osc = group_align(n_out * 4), b_og = group_align(n_out * 4);
  const size_t b_cnt = group_align((size_t)nq * 4);
  GroupStage st;
  const size_t total = b_ids + b_sc + b_tab + b_oid + b_osc + b_og + 2 * b_cnt;
  const hipError_t e = hipMalloc(&st.p, total);
  if (e != hipSuccess) {
    st.p = nullptr;
    ts_set_error("group: hipMalloc(%zu bytes) failed: %s", total, hipGetErrorString(e));
    return TS_ERR_OOM;
  }
  char* b = (char*)st.p;
  int64_t* d_ids = (int64_t*)b;            b += b_ids;
  float* d_sc = (float*)b;                 b += b_sc;
  int32_t* d_tab = (int32_t*)b;            b += b_tab;
  int64_t* d_oid = (int64_t*)b;            b += b_oid;
  float* d_osc = (float*)b;                b += b_osc;
  int32_t* d_og = (int32_t*)b;             b += b_og;
  int32_t* d_ng = (int32_t*)b;             b += b_cnt;
  int32_t* d_nv = (int32_t*)b;
  TS_HIP(hipMemcpyAsync(d_ids, cand_ids, n_in * 8, hipMemcpyHostToDevice, s));
  TS_HIP(hipMemcpyAsync(d_sc, cand_scores, n_in * 4, hipMemcpyHostToDevice, s));
  if (n_rows > 0) TS_HIP(hipMemcpyAsync(d_tab, groups, (size_t)n_rows * 4, hipMemcpyHostToDevice, s));
  p.ids = d_ids; p.scores = d_sc; p.groups = d_tab;
  p.out_scores = d_osc; p.out_ids = d_oid; p.out_groups = d_og;
  p.out_ngroups = d_ng; p.out_nvalid = d_nv;
  TS_CHECK(group_launch(p, nq, s));
  TS_HIP(hipMemcpyAsync(out_scores, d_osc, n_out * 4, hipMemcpyDeviceToHost, s));
  TS_HIP(hipMemcpyAsync(out_ids, d_oid, n_out * 8, hipMemcpyDeviceToHost, s));
  TS_HIP(hipMemcpyAsync(out_groups, d_og, n_out * 4, hipMemcpyDeviceToHost, s));
  TS_HIP(hipMemcpyAsync(out_ngroups, d_ng, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  TS_HIP(hipMemcpyAsync(out_nvalid, d_nv, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  TS_HIP(hipStreamSynchronize(s));
  return TS_OK;
}
