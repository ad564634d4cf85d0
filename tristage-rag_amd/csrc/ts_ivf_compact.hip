// Compaction of an IVF-Flat index (ts_compact_ivf in ts_ivf.hip): the kernels that tell the host which
// ids are live and in which list, and that write the new corpus and its tables from the old ones.
//
// The host places the survivors with the placement routine of ts_ivf_add (ivf_place in ts_ivf.hip), so the new index is
// the one a fresh add of the surviving rows would build.  Out of place: the old slot -> new slot map is not monotone
// across lists (list 3's second block may lie behind list 5's first in the old corpus and in front of it in the new
// one), so no order of in-place chunks reads every block before it is overwritten.
//   ivfc_classify_kernel  per old id: its list, or -1 when it was removed
//   ivfc_tables_kernel    per new id: slot2id / id2slot of the new index and src_slot[new slot] = the row's old slot
//   ivfc_move_kernel      per (new block, TS_RING k groups): whole 1 KiB unit rows of the new corpus, each lane's 16
//                         bytes gathered from its row's old slot (zeros for a padding slot); the block's valid word
// Every device write below is a plain vector store.
#include "ts_common.h"

// An id is live iff its slot points back at it: a removed id keeps id2slot but its slot's slot2id is -1 (or, after an
// update took the slot's place elsewhere, the id points at its new slot, which points back).
__global__ void ivfc_classify_kernel(const int64_t* id2slot, const int64_t* slot2id, const int32_t* blk_list,
                                     int64_t ntotal, int32_t* lists) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= ntotal) return;
  const int64_t s = id2slot[id];
  lists[id] = slot2id[s] == id ? blk_list[s >> 5] : -1;
}

int ts_launch_ivf_compact_classify(const int64_t* id2slot, const int64_t* slot2id, const int32_t* blk_list,
                                   int64_t ntotal, int32_t* lists, hipStream_t stream) {
  if (ntotal <= 0) return TS_OK;
  hipLaunchKernelGGL(ivfc_classify_kernel, dim3((unsigned)((ntotal + 255) / 256)), dim3(256), 0, stream, id2slot,
                     slot2id, blk_list, ntotal, lists);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// New id j is old id new2old[j] and takes slot dst[j].  src_slot and new_slot2id were filled with -1 (padding slots).
__global__ void ivfc_tables_kernel(const int32_t* new2old, const int32_t* dst, int64_t nlive,
                                   const int64_t* old_id2slot, int32_t* src_slot, int64_t* new_slot2id,
                                   int64_t* new_id2slot) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nlive) return;
  const int64_t ns = dst[j];
  src_slot[ns] = (int32_t)old_id2slot[new2old[j]];
  new_slot2id[ns] = j;
  new_id2slot[j] = ns;
}

typedef uint32_t ivfc_u32x4 __attribute__((ext_vector_type(4)));

// One wave per (new block, TS_RING k groups): lane h * 32 + r writes the 16-byte unit of new row r in each of its unit
// rows, read from unit (ob * kg + g) * 64 + h * 32 + orow of the row's old slot 32 ob + orow.  The loads of all
// TS_RING unit rows are in flight before the first store; a store instruction writes 1 KiB contiguously.  A list's
// survivors keep their order unless they were updated, so the 16-byte reads are mostly runs inside one old unit row.
__global__ __launch_bounds__(256) void ivfc_move_kernel(const uint4* old_corpus, uint4* new_corpus,
                                                        const int32_t* src_slot, int64_t nwave, int kg,
                                                        uint32_t* new_valid) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= nwave) return;
  const int per = kg / TS_RING;   // (kg is a multiple of TS_RING: ts_make_layout)
  const int64_t b = wv / per;
  const int g0 = (int)(wv % per) * TS_RING;
  const int64_t s = src_slot[b * 32 + (lane & 31)];
  if (g0 == 0) {
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(s >= 0);
    if (lane == 0) new_valid[b] = (uint32_t)bal;
  }
  const int64_t os = s < 0 ? 0 : s;   // (a padding lane loads nothing)
  const ivfc_u32x4* src = reinterpret_cast<const ivfc_u32x4*>(old_corpus) + ((os >> 5) * kg + g0) * 64 + (lane & 32) +
                          (os & 31);
  ivfc_u32x4* d = reinterpret_cast<ivfc_u32x4*>(new_corpus) + (b * kg + g0) * 64 + lane;
  ivfc_u32x4 v[TS_RING];   // (a register vector type: an array of HIP's uint4 struct goes to scratch)
#pragma unroll
  for (int i = 0; i < TS_RING; ++i) v[i] = s >= 0 ? src[i * 64] : ivfc_u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < TS_RING; ++i) d[i * 64] = v[i];
}

int ts_launch_ivf_compact_move(const TsLayout& L, const uint4* old_corpus, const int64_t* old_id2slot,
                               const int32_t* new2old, const int32_t* dst, int64_t nlive, int64_t new_blocks,
                               uint4* new_corpus, int32_t* src_slot, int64_t* new_slot2id, int64_t* new_id2slot,
                               uint32_t* new_valid, hipStream_t stream) {
  if (nlive <= 0 || new_blocks <= 0) return TS_OK;
  TS_HIP(hipMemsetAsync(src_slot, 0xFF, (size_t)new_blocks * 32 * 4, stream));
  TS_HIP(hipMemsetAsync(new_slot2id, 0xFF, (size_t)new_blocks * 32 * 8, stream));
  hipLaunchKernelGGL(ivfc_tables_kernel, dim3((unsigned)((nlive + 255) / 256)), dim3(256), 0, stream, new2old, dst,
                     nlive, old_id2slot, src_slot, new_slot2id, new_id2slot);
  TS_HIP(hipGetLastError());
  const int64_t nwave = new_blocks * (L.kg / TS_RING);
  const int64_t blocks = (nwave + 3) / 4;
  if (blocks > 0x7fffffffLL) { ts_set_error("compact: too many row blocks"); return TS_ERR_INVALID; }
  hipLaunchKernelGGL(ivfc_move_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, old_corpus, new_corpus,
                     (const int32_t*)src_slot, nwave, L.kg, new_valid);
  TS_HIP(hipGetLastError());
  return TS_OK;
}
