// Update of stored rows in place (ts_index_update / ts_update_ivf): the kernels that move the rows of a
// staging tile, written there by the relayout of ts_index_add, to the places of the ids they replace.
//
// A row of the tiled layout (ts_common.h) is 2 * kg units of 16 bytes, one per (k group g, half h), each in a
// different 1 KiB unit row: unit (b * kg + g) * 64 + h * 32 + r for row 32 b + r.  The host sorts the ids of a staging
// chunk by row and groups them per row block (ts_update_group_blocks); of a row that is not updated no byte is
// written.  One wave owns a (block, k group) unit row and writes every updated row of the block in it, so the rows of
// one block share their unit rows:
//   upd_block_kernel   blocks all 32 of whose rows are updated: whole unit rows, 64 lanes x 16 contiguous bytes, as the
//                      relayout of an add writes them
//   upd_rows_kernel    the other blocks: per unit row the two 16-byte pieces (h = 0 / 1) of each updated row
// Every device write below is a plain vector store or a vector atomic.
#include "ts_common.h"

#include <algorithm>
#include <utility>
#include <vector>

// ---------------------------------------------------------------- host: the ids of a call
// keys[i] = rows[i] << 32 | i, ordered by row (stable: equal rows keep their order): three 11-bit counting passes over
// the row bits, rows < 2^31.  The keys are moved themselves, so every pass reads its input in sequence and the
// grouping below reads rows and positions in sequence too.  (Per call of 100 000 random ids: std::sort of (row,
// position) pairs 9.8 ms; counting passes over positions, which gather rows[position], 1.8 ms.)
void ts_update_sort_rows(const int64_t* rows, int64_t n, std::vector<uint64_t>* keys) {
  std::vector<uint64_t>& k = *keys;
  k.resize((size_t)n);
  bool asc = true;
  for (int64_t i = 0; i < n; ++i) {
    k[(size_t)i] = ((uint64_t)rows[i] << 32) | (uint64_t)i;
    if (i && rows[i] < rows[i - 1]) asc = false;
  }
  if (asc) return;
  std::vector<uint64_t> tmp((size_t)n);
  for (int shift = 32; shift < 65; shift += 11) {
    size_t cnt[2049] = {0};
    for (int64_t i = 0; i < n; ++i) ++cnt[((k[(size_t)i] >> shift) & 2047) + 1];
    for (int b = 0; b < 2048; ++b) cnt[b + 1] += cnt[b];
    for (int64_t i = 0; i < n; ++i) tmp[cnt[(k[(size_t)i] >> shift) & 2047]++] = k[(size_t)i];
    k.swap(tmp);
  }
}

int ts_update_check_ids(const int64_t* ids, int64_t n, int64_t id_offset, int64_t ntotal, int64_t* rows,
                        std::vector<uint64_t>* keys) {
  if (n >= (1LL << 31)) { ts_set_error("update: too many ids in one call"); return TS_ERR_INVALID; }
  bool asc = true;   // strictly ascending: no id twice, and nothing to order
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = ids[i] - id_offset;
    if (r < 0 || r >= ntotal) {
      ts_set_error("update: id %lld is not an id of this index (%lld rows)", (long long)ids[i], (long long)ntotal);
      return TS_ERR_INVALID;
    }
    rows[i] = r;
    if (i && r <= rows[i - 1]) asc = false;
  }
  keys->clear();
  if (asc) return TS_OK;
  ts_update_sort_rows(rows, n, keys);
  const std::vector<uint64_t>& k = *keys;
  int64_t first = -1;   // the earliest position that repeats an id given before it
  for (int64_t i = 1; i < n; ++i)
    if ((k[(size_t)i] >> 32) == (k[(size_t)i - 1] >> 32) && (first < 0 || (int64_t)(uint32_t)k[(size_t)i] < first))
      first = (int64_t)(uint32_t)k[(size_t)i];
  if (first >= 0) {
    ts_set_error("update: id %lld is given twice in one call", (long long)ids[first]);
    return TS_ERR_INVALID;
  }
  return TS_OK;
}

void ts_update_group_blocks(const uint64_t* keys, int64_t n, TsUpdateTables* t) {
  t->full_blk.clear();
  t->full_src.clear();
  t->part_blk.clear();
  t->part_first.clear();
  t->part_item.clear();
  t->part_blk.reserve((size_t)n);
  t->part_first.reserve((size_t)n + 1);
  t->part_item.reserve((size_t)n);
  for (int64_t i = 0; i < n;) {
    const uint64_t b = keys[i] >> 37;   // the row block
    int64_t e = i + 1;
    while (e < n && (keys[e] >> 37) == b) ++e;
    if (e - i == 32) {   // (distinct rows of one block: all of them)
      t->full_blk.push_back((int32_t)b);
      const size_t at = t->full_src.size();
      t->full_src.resize(at + 32);
      for (int64_t k = i; k < e; ++k) t->full_src[at + (size_t)((keys[k] >> 32) & 31)] = (int32_t)(uint32_t)keys[k];
    } else {
      t->part_blk.push_back((int32_t)b);
      t->part_first.push_back((int32_t)t->part_item.size());
      for (int64_t k = i; k < e; ++k)
        t->part_item.push_back((int32_t)((uint32_t)keys[k] * 32u + (uint32_t)((keys[k] >> 32) & 31)));
    }
    i = e;
  }
  t->part_first.push_back((int32_t)t->part_item.size());
}

// ---------------------------------------------------------------- kernels
// ids of a call against the tombstone bitmap: out[0] += rows whose live bit is clear, out[1] = min(out[1], position in
// the call of such a row).  rows[] are ids after the id offset, already range-checked by the host.
__global__ void upd_live_check_kernel(const uint32_t* live, const int64_t* rows, int64_t n, unsigned long long* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool dead = false;
  if (i < n) {
    const int64_t r = rows[i];
    dead = ((live[r >> 5] >> (r & 31)) & 1u) == 0u;
  }
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(dead);
  if (bal == 0ull) return;
  if (dead && (bal & ((1ull << (threadIdx.x & 63)) - 1ull)) == 0ull) {   // the wave's first such lane
    atomicAdd(&out[0], (unsigned long long)__builtin_popcountll(bal));
    atomicMin(&out[1], (unsigned long long)i);
  }
}

int ts_launch_update_live_check(const uint32_t* live, const int64_t* rows, int64_t n, unsigned long long* out,
                                hipStream_t stream) {
  if (n <= 0) return TS_OK;
  hipLaunchKernelGGL(upd_live_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, live, rows, n,
                     out);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

typedef uint32_t upd_u32x4 __attribute__((ext_vector_type(4)));

// one wave per (entry, k group): a whole unit row of a fully updated block
__global__ __launch_bounds__(256) void upd_block_kernel(const uint4* stage, uint4* corpus, const int32_t* blk,
                                                        const int32_t* src, int64_t nwave, int kg) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= nwave) return;
  const int64_t e = wv / kg;
  const int g = (int)(wv % kg);
  const int64_t j = src[e * 32 + (lane & 31)];
  corpus[((int64_t)blk[e] * kg + g) * 64 + lane] = stage[((j >> 5) * kg + g) * 64 + (lane & 32) + (j & 31)];
}

// one wave per (entry, TS_RING k groups): in each of its unit rows the pieces of the block's updated rows; the loads
// of all TS_RING unit rows are in flight before the first store.  Entry e holds the items first[e] .. first[e + 1)
// (fewer than 32), item = staging row * 32 + row of the block.
__global__ __launch_bounds__(256) void upd_rows_kernel(const uint4* stage, uint4* corpus, const int32_t* blk,
                                                       const int32_t* first, const int32_t* item, int64_t nwave,
                                                       int kg) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= nwave) return;
  const int per = kg / TS_RING;   // (kg is a multiple of TS_RING: ts_make_layout)
  const int64_t e = wv / per;
  const int g0 = (int)(wv % per) * TS_RING;
  const int f0 = first[e], cnt = first[e + 1] - f0;
  const int mine = lane < cnt ? item[f0 + lane] : -1;
  int64_t j = -1;
  for (int t = 0; t < cnt; ++t) {
    const int it = __shfl(mine, t, 64);
    if ((it & 31) == (lane & 31)) j = it >> 5;
  }
  if (j < 0) return;
  const upd_u32x4* s = reinterpret_cast<const upd_u32x4*>(stage) + ((j >> 5) * kg + g0) * 64 + (lane & 32) + (j & 31);
  upd_u32x4* d = reinterpret_cast<upd_u32x4*>(corpus) + ((int64_t)blk[e] * kg + g0) * 64 + lane;
  upd_u32x4 v[TS_RING];   // (a register vector type: an array of HIP's uint4 struct goes to scratch)
#pragma unroll
  for (int i = 0; i < TS_RING; ++i) v[i] = s[i * 64];
#pragma unroll
  for (int i = 0; i < TS_RING; ++i) d[i * 64] = v[i];
}

int ts_launch_update_blocks(const TsLayout& L, const uint4* stage, uint4* corpus, const int32_t* blk,
                            const int32_t* src, int64_t n_entries, hipStream_t stream) {
  if (n_entries <= 0) return TS_OK;
  const int64_t nwave = n_entries * L.kg;
  const int64_t blocks = (nwave + 3) / 4;
  if (blocks > 0x7fffffffLL) { ts_set_error("update: too many rows in one chunk"); return TS_ERR_INVALID; }
  hipLaunchKernelGGL(upd_block_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, stage, corpus, blk, src, nwave,
                     L.kg);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

int ts_launch_update_rows(const TsLayout& L, const uint4* stage, uint4* corpus, const int32_t* blk,
                          const int32_t* first, const int32_t* item, int64_t n_entries, hipStream_t stream) {
  if (n_entries <= 0) return TS_OK;
  if (L.dtype == TS_MXFP4_E2M1)   // (its row block is not a multiple of TS_RING units: ts_scan_fp4.hip)
    return ts_launch_update_rows_fp4(L, stage, corpus, blk, first, item, n_entries, stream);
  const int64_t nwave = n_entries * (L.kg / TS_RING);
  const int64_t blocks = (nwave + 3) / 4;
  if (blocks > 0x7fffffffLL) { ts_set_error("update: too many rows in one chunk"); return TS_ERR_INVALID; }
  hipLaunchKernelGGL(upd_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, stage, corpus, blk, first, item,
                     nwave, L.kg);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// ---------------------------------------------------------------- IVF
// ids of a call against the lists: a live id's slot is occupied and points back to it (a removed id keeps id2slot but
// has left slot2id and its block's valid word); out as upd_live_check_kernel
__global__ void upd_ivf_check_kernel(const int64_t* rows, int64_t n, const int64_t* id2slot, const int64_t* slot2id,
                                     const uint32_t* blk_valid, unsigned long long* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool dead = false;
  if (i < n) {
    const int64_t r = rows[i];
    const int64_t s = id2slot[r];
    dead = slot2id[s] != r || ((blk_valid[s >> 5] >> (s & 31)) & 1u) == 0u;
  }
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(dead);
  if (bal == 0ull) return;
  if (dead && (bal & ((1ull << (threadIdx.x & 63)) - 1ull)) == 0ull) {
    atomicAdd(&out[0], (unsigned long long)__builtin_popcountll(bal));
    atomicMin(&out[1], (unsigned long long)i);
  }
}

int ts_launch_update_ivf_check(const int64_t* rows, int64_t n, const int64_t* id2slot, const int64_t* slot2id,
                               const uint32_t* blk_valid, unsigned long long* out, hipStream_t stream) {
  if (n <= 0) return TS_OK;
  hipLaunchKernelGGL(upd_ivf_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, rows, n, id2slot,
                     slot2id, blk_valid, out);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// row r of the chunk's tiled staging goes to slot dst[r] under its old id ids[r]; one thread per (row, 16-byte unit),
// as the scatter of the IVF add
__global__ void upd_ivf_place_kernel(const uint4* src, uint4* corpus, const int64_t* dst, const int64_t* ids, int64_t n,
                                     int kg, int64_t* slot2id, int64_t* id2slot, uint32_t* blk_valid) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)kg * 2;
  if (t >= n * per) return;
  const int64_t r = t / per;
  const int u = (int)(t % per);
  const int g = u >> 1, hh = u & 1;
  const int64_t s = dst[r];
  corpus[((s >> 5) * kg + g) * 64 + hh * 32 + (s & 31)] = src[((r >> 5) * kg + g) * 64 + hh * 32 + (r & 31)];
  if (u == 0) {
    slot2id[s] = ids[r];
    id2slot[ids[r]] = s;
    atomicOr(&blk_valid[s >> 5], 1u << (s & 31));
  }
}

int ts_launch_update_ivf_place(const TsLayout& L, const uint4* src, uint4* corpus, const int64_t* dst,
                               const int64_t* ids, int64_t n, int64_t* slot2id, int64_t* id2slot, uint32_t* blk_valid,
                               hipStream_t stream) {
  if (n <= 0) return TS_OK;
  const int64_t th = n * L.kg * 2;
  hipLaunchKernelGGL(upd_ivf_place_kernel, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, stream, src, corpus, dst,
                     ids, n, L.kg, slot2id, id2slot, blk_valid);
  TS_HIP(hipGetLastError());
  return TS_OK;
}
