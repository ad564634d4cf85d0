// IVF-Flat index (include/tristage.h "IVF-Flat"): spherical k-means lists over the flat index's tiled storage, and a
// search that scans only the 32-row blocks of the lists its queries probe.
//
// Reference seam: faiss.IndexIVFFlat(quantizer, d, nlist, METRIC_INNER_PRODUCT) with nprobe
// (reference src/stage1_retriever.py:256-283), which the reference builds above 1000 documents.
//
//   storage    row blocks of 32 slots in MFMA A-fragment order (ts_common.h "layout"), each block holding rows of
//              ONE list; per list a host table of its blocks, so an add appends to a list's last block or takes
//              fresh blocks at the end.  Device tables: blk_list[b] (list of block b), blk_valid[b] (occupied
//              slots, bit i = slot 32b + i), slot2id[slot] (local id, -1 for a free slot), id2slot[id].
//   quantizer  an fp32 ts_index holding the centroids: assignment and probing are its exact top-1 / top-nprobe.
//   search     per pass of <= 64 queries: probe bitmap + union of the probed lists' blocks (the live list), a dense
//              scan of a strided sample of the live list, per-query thresholds from the probed sample rows, the
//              filter scan over the live list (scan_ivf_kernel: allow word = probed(q, list) ? valid : 0), slot ->
//              id remap, exact select; fewer than min(k, N_q) survivors or an overflowing list: dense redo.
#include "ts_scan_dev.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

namespace {

constexpr int kIvfMaxList = 16384;             // nlist limit: nprobe = nlist must fit the select (16384 keys)
constexpr int64_t kIvfMinFilterSlots = 32768;  // below this the dense path is used (as ts_index)
constexpr int kIvfMaxFilterK = 2048;
constexpr uint32_t kIvfCandCap = 16384;        // candidate slots per query
constexpr int kIvfSampleDiv = 32;              // threshold sample: 1/32 of the live blocks ...
constexpr int kIvfMinSampleBlocks = 64;        // ... and at least 64 of them (or all)
constexpr uint32_t kIvfMinSampleRank = 24;
constexpr int64_t kIvfDenseChunkRows = 1 << 20;
constexpr int64_t kIvfAddChunkRows = 1 << 16;
constexpr int kIvfTrainPerList = 256;          // FAISS max_points_per_centroid
constexpr float kIvfSplitEps = 1.0f / 1024.0f; // FAISS's empty-cluster split perturbation

// a buffer that keeps its first `keep` bytes when it grows
int ivf_grow(TsDevBuf& b, size_t bytes, size_t keep, hipStream_t s) {
  if (b.bytes >= bytes && b.p) return TS_OK;
  const size_t want = std::max((bytes + 0xFFFFF) & ~(size_t)0xFFFFF, b.bytes + b.bytes / 2);
  void* np = nullptr;
  hipError_t e = hipMalloc(&np, want);
  if (e != hipSuccess) {
    ts_set_error("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
    return TS_ERR_OOM;
  }
  if (keep && b.p) TS_HIP(hipMemcpyAsync(np, b.p, keep, hipMemcpyDeviceToDevice, s));
  TS_HIP(hipStreamSynchronize(s));
  if (b.p) TS_HIP(hipFree(b.p));
  b.p = np;
  b.bytes = want;
  return TS_OK;
}

uint64_t splitmix64(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace

struct ts_ivf {
  int device = 0;
  int num_cus = 256;
  int nlist = 0;
  int pwords = 0;         // 32-bit words of one probe bitmap (nlist bits)
  TsLayout L{};
  ts_index* quant = nullptr;
  bool trained = false;
  int64_t ntotal = 0;
  int64_t nblocks = 0;    // row blocks in use
  int64_t id_offset = 0;
  int64_t info[4] = {0, 0, 0, 0};
  std::vector<std::vector<int32_t>> list_blocks;
  std::vector<int64_t> list_size;      // slots taken per list (where add continues)
  std::vector<int64_t> list_removed;   // of them removed (ts_remove_ivf): dlist_size = list_size - list_removed
  TsDevBuf corpus, blk_list, blk_valid, slot2id, id2slot, dlist_size;
  // add staging
  TsDevBuf tmp_tiled, tmp_f32, den, assign, ascore, dst;
  TsDevBuf upd_ids;   // ts_update_ivf: the chunk's local ids
  // search workspace
  TsDevBuf qimg, small, pid, pscore, bits, live, sample, cand_score, cand_id, dense, mids, list_score, list_id;
  // training
  TsDevBuf train_x, cent, perm, offs;
  uint32_t* host_rep = nullptr;      // pinned + mapped: select report (64 counts, status, live blocks)
  uint32_t* host_rep_dev = nullptr;
  TsMmrWork mmr;                     // ts_mmr_ivf: scratch and staging, allocated at the first call
  float* tau() { return (float*)small.p; }
  uint32_t* cand_cnt() { return (uint32_t*)small.p + 64; }
  uint32_t* status() { return (uint32_t*)small.p + 128; }
  uint32_t* need() { return (uint32_t*)small.p + 192; }
  uint32_t* nlive() { return (uint32_t*)small.p + 256; }
};

// ------------------------------------------------------------------ kernels
typedef const uint32_t __attribute__((address_space(4)))* ivf_sgpr_u32p;
typedef const int32_t __attribute__((address_space(4)))* ivf_sgpr_i32p;

// scan_masked_kernel's parameters for inverted lists: work item w is row block live[w] (w < *nlive); a survivor of
// query q in block b needs bit (row % 32) of probed(q, blk_list[b]) ? blk_valid[b] : 0.  Dense mode (the threshold
// sample): work item w < items = min(nlive, max(sample_min, nlive / sample_div)) is live block live[w * (nlive / items)],
// written at dense[q][32w..].
struct IvfScanParams : ScanParams {
  const int32_t* live;
  const uint32_t* nlive;
  const int32_t* blk_list;
  const uint32_t* blk_valid;
  const uint32_t* probe_bits;   // [64][pwords]
  int32_t pwords;
  int32_t sample_min;   // dense mode: sample items = min(nlive, max(sample_min, nlive / sample_div))
  int32_t sample_div;
};

__device__ __forceinline__ void ivf_sample_geom(uint32_t n, int32_t min_items, int32_t div, int64_t* items,
                                                int64_t* stride) {
  int64_t it = (int64_t)n / div;
  it = it > min_items ? it : min_items;
  it = it < (int64_t)n ? it : (int64_t)n;
  *items = it;
  *stride = it > 0 ? (int64_t)n / it : 1;
}

// scan_masked_kernel with the allow word of a block derived from the pass's probe bitmaps: the block's list and
// valid word are wave-uniform (scalar loads, lgkmcnt), the lane's probe word is requested before the next block's
// first ring loads and is complete by that block's epilogue, as the masked scan's allow word is.
template <int DT, int QH, int MODE>
__global__ __launch_bounds__(SCAN_THREADS) void scan_ivf_kernel(IvfScanParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* qlds = reinterpret_cast<u32x4*>(smem);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kg = p.kg;

  const int64_t nwaves = (int64_t)gridDim.x * SCAN_WAVES;
  int64_t w = (int64_t)blockIdx.x * SCAN_WAVES + wave;
  const uint32_t nl = *(ivf_sgpr_u32p)p.nlive;
  int64_t nwork = nl, wstride = 1;
  if constexpr (MODE == SCAN_DENSE) ivf_sample_geom(nl, p.sample_min, p.sample_div, &nwork, &wstride);
  const bool active = w < nwork;
  const u32x4* base = reinterpret_cast<const u32x4*>(p.corpus) + lane;
  const size_t blk_units = (size_t)kg * 64;
  int64_t blk = active ? (int64_t)((ivf_sgpr_i32p)p.live)[w * wstride] : 0;
  const u32x4* cur = base + (size_t)blk * blk_units;
  u32x4 ring[TS_RING];
  if (active) {
#pragma unroll
    for (int i = 0; i < TS_RING; ++i) ring[i] = stream_load(cur + (size_t)i * 64);
  }

  {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.qimg);
    const int units = kg * QH * 64;
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
  StageLds* st = reinterpret_cast<StageLds*>(smem + (size_t)kg * QH * 1024);
  if constexpr (MODE == SCAN_FILTER) {
    if (tid == 0) st->cnt = 0;
  }
  __syncthreads();

  if (active) {

  float tau[QH];
  const uint32_t* prow[QH];
  uint32_t mw[QH];
  if constexpr (MODE == SCAN_FILTER) {
    const int32_t lst = ((ivf_sgpr_i32p)p.blk_list)[blk];
    const uint32_t vld = ((ivf_sgpr_u32p)p.blk_valid)[blk];
#pragma unroll
    for (int hq = 0; hq < QH; ++hq) {
      const int q = hq * 32 + (lane & 31);
      tau[hq] = p.tau[q];
      prow[hq] = p.probe_bits + (int64_t)q * p.pwords;
      mw[hq] = ((prow[hq][lst >> 5] >> (lst & 31)) & 1u) ? vld : 0u;
    }
  }

  const u32x4* ql = qlds + lane;

  while (true) {
    const int64_t wn = w + nwaves;
    const bool has_next = wn < nwork;
    const int64_t blkn = has_next ? (int64_t)((ivf_sgpr_i32p)p.live)[wn * wstride] : blk;
    const u32x4* nxt = base + (size_t)blkn * blk_units;

    f32x16 acc[QH];
#pragma unroll
    for (int hq = 0; hq < QH; ++hq)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[hq][r] = 0.f;

    int g0 = 0;
    for (; g0 < kg - TS_RING; g0 += TS_RING) {
#pragma unroll
      for (int i = 0; i < TS_RING; ++i) {
#pragma unroll
        for (int hq = 0; hq < QH; ++hq) {
          const u32x4 b = ql[(size_t)((g0 + i) * QH + hq) * 64];
          mma_group<DT>(acc[hq], ring[i], b);
        }
        ring[i] = stream_load(cur + (size_t)(g0 + i + TS_RING) * 64);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // tail: the next block's list, valid word and probe words, then the ring is refilled from that block
    int32_t lstn = 0;
    uint32_t vldn = 0, pwn[QH];
    if constexpr (MODE == SCAN_FILTER) {
      lstn = ((ivf_sgpr_i32p)p.blk_list)[blkn];
      vldn = ((ivf_sgpr_u32p)p.blk_valid)[blkn];
#pragma unroll
      for (int hq = 0; hq < QH; ++hq) pwn[hq] = prow[hq][lstn >> 5];
    }
#pragma unroll
    for (int i = 0; i < TS_RING; ++i) {
#pragma unroll
      for (int hq = 0; hq < QH; ++hq) {
        const u32x4 b = ql[(size_t)((g0 + i) * QH + hq) * 64];
        mma_group<DT>(acc[hq], ring[i], b);
      }
      ring[i] = stream_load(nxt + (size_t)i * 64);
      __builtin_amdgcn_sched_barrier(0);
    }

    if constexpr (MODE == SCAN_DENSE)
      epilogue_dense<QH>(p, acc, w, blk, lane);
    else
      epilogue_filter<QH, StageLds, true>(p, st, acc, tau, blk, lane, mw);

    if (!has_next) break;
    w = wn;
    blk = blkn;
    cur = nxt;
    if constexpr (MODE == SCAN_FILTER) {
#pragma unroll
      for (int hq = 0; hq < QH; ++hq) mw[hq] = ((pwn[hq] >> (lstn & 31)) & 1u) ? vldn : 0u;
    }
  }
  }  // active
  if constexpr (MODE == SCAN_FILTER) flush_stage(p, st, tid);
}

// probe bitmaps of the pass (bits[q][pwords]) and their union (bits[64][pwords]); thread per (query, probe)
__global__ void ivf_probe_bits_kernel(const int64_t* pid, int nq, int nprobe, int pwords, uint32_t* bits) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nq * nprobe) return;
  const int q = (int)(t / nprobe);
  const int64_t l = pid[t];
  if (l < 0) return;
  const uint32_t bit = 1u << (l & 31);
  atomicOr(&bits[(int64_t)q * pwords + (l >> 5)], bit);
  atomicOr(&bits[(int64_t)TS_MAX_Q * pwords + (l >> 5)], bit);
}

// live[] = occupied blocks of a probed list (one atomic per wave, block order kept inside a wave)
__global__ __launch_bounds__(256) void ivf_live_kernel(const int32_t* blk_list, const uint32_t* blk_valid,
                                                       int64_t nblk, const uint32_t* ubits, int32_t* live,
                                                       uint32_t* nlive) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool on = false;
  if (b < nblk) {
    const int32_t l = blk_list[b];
    on = blk_valid[b] != 0u && ((ubits[l >> 5] >> (l & 31)) & 1u);
  }
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(on);
  if (bal == 0ull) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(nlive, (uint32_t)__builtin_popcountll(bal));
  base = (uint32_t)__shfl((int)base, 0, 64);
  if (on) live[base + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull))] = (int32_t)b;
}

__device__ __forceinline__ uint32_t ivf_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ivf_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Per query (one workgroup): N_q = rows of its probed lists, S_q = its probed rows in the sample, m_q =
// max(min_rank, ceil(over * k * S_q / N_q)); tau = the m_q-th best probed sample score, exactly: the sample row is
// rewritten in place as order-preserving keys (0 = not a probed row), then a 4-round 8-bit radix select over them.
// -FLT_MAX when S_q < m_q.  need[q] = min(k, N_q).  +FLT_MAX for q >= nq.
#define IVF_TAU_THREADS 256
__global__ __launch_bounds__(IVF_TAU_THREADS) void ivf_tau_kernel(
    float* sample, int64_t ld, int32_t sample_min, int32_t sample_div, const int32_t* live, const uint32_t* nlive,
    const int32_t* blk_list, const uint32_t* blk_valid, const uint32_t* bits, int pwords, const int64_t* pid,
    int nprobe, const int64_t* list_size, int nq, int k, uint32_t over, uint32_t min_rank, float* tau,
    uint32_t* need, uint32_t* report) {
  __shared__ uint32_t hist[256];
  __shared__ unsigned long long red[IVF_TAU_THREADS / 64];
  __shared__ uint32_t redc[IVF_TAU_THREADS / 64];
  __shared__ uint32_t sel[2];
  const int q = blockIdx.x;
  const int tid = threadIdx.x;
  if (q == 0 && tid == 0 && report) report[0] = *nlive;
  if (q >= nq) {
    if (tid == 0) { tau[q] = 3.402823466e38f; need[q] = 0u; }
    return;
  }
  int64_t items, stride;
  ivf_sample_geom(*nlive, sample_min, sample_div, &items, &stride);
  const int64_t ne = items * 32;
  unsigned long long nq_rows = 0;
  for (int j = tid; j < nprobe; j += IVF_TAU_THREADS) {
    const int64_t l = pid[(int64_t)q * nprobe + j];
    if (l >= 0) nq_rows += (unsigned long long)list_size[l];
  }
  const uint32_t* qb = bits + (int64_t)q * pwords;
  uint32_t* keys = reinterpret_cast<uint32_t*>(sample + (int64_t)q * ld);
  uint32_t s_q = 0;
  for (int64_t e = tid; e < ne; e += IVF_TAU_THREADS) {
    const int64_t blk = live[(e >> 5) * stride];
    const int32_t l = blk_list[blk];
    const bool ok = ((qb[l >> 5] >> (l & 31)) & 1u) && ((blk_valid[blk] >> (e & 31)) & 1u);
    keys[e] = ok ? ivf_key(__uint_as_float(keys[e])) : 0u;
    s_q += ok ? 1u : 0u;
  }
  for (int off = 32; off > 0; off >>= 1) {
    nq_rows += (unsigned long long)__shfl_xor((long long)nq_rows, off, 64);
    s_q += (uint32_t)__shfl_xor((int)s_q, off, 64);
  }
  if ((tid & 63) == 0) { red[tid >> 6] = nq_rows; redc[tid >> 6] = s_q; }
  __syncthreads();
  unsigned long long N = 0;
  uint32_t S = 0;
  for (int i = 0; i < IVF_TAU_THREADS / 64; ++i) { N += red[i]; S += redc[i]; }
  uint32_t m = N ? (uint32_t)(((unsigned long long)over * (unsigned long long)k * S + N - 1) / N) : 0u;
  m = m > min_rank ? m : min_rank;
  if (tid == 0) need[q] = (uint32_t)((unsigned long long)k < N ? (unsigned long long)k : N);
  if (S < m || N == 0) {
    if (tid == 0) tau[q] = -3.402823466e38f;
    return;
  }
  // the m-th largest key, 8 bits per round
  uint32_t prefix = 0, mask = 0, want = m;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;   // (IVF_TAU_THREADS == 256 bins)
    __syncthreads();
    for (int64_t e = tid; e < ne; e += IVF_TAU_THREADS) {
      const uint32_t kk = keys[e];
      if (kk != 0u && (kk & mask) == prefix) atomicAdd(&hist[(kk >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t cum = 0;
      int b = 255;
      for (; b > 0; --b) {
        if (cum + hist[b] >= want) break;
        cum += hist[b];
      }
      sel[0] = (uint32_t)b;
      sel[1] = want - cum;
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    want = sel[1];
    mask |= 255u << shift;
    __syncthreads();
  }
  if (tid == 0) tau[q] = ivf_unkey(prefix);
}

// candidate slot -> local id, so that the select orders ties by original id
__global__ void ivf_remap_kernel(int32_t* cand_id, const uint32_t* cand_cnt, uint32_t cap, int nq,
                                 const int64_t* slot2id) {
  const int q = blockIdx.y;
  if (q >= nq) return;
  const uint32_t n = cand_cnt[q] < cap ? cand_cnt[q] : cap;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    int32_t* p = cand_id + (size_t)q * cap + j;
    *p = (int32_t)slot2id[*p];
  }
}

// the dense path's ids: ids[q][i] = local id of slot row0 + i if it is occupied and its list probed by q, else -1
__global__ void ivf_dense_ids_kernel(const int32_t* blk_list, const int64_t* slot2id, const uint32_t* bits,
                                     int pwords, int nq, int64_t row0, uint32_t rows, int64_t ld, int32_t* ids) {
  const int q = blockIdx.y;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq || i >= rows) return;
  const int64_t slot = row0 + i;
  const int64_t id = slot2id[slot];
  const int32_t l = blk_list[slot >> 5];
  const bool ok = id >= 0 && ((bits[(int64_t)q * pwords + (l >> 5)] >> (l & 31)) & 1u);
  ids[(int64_t)q * ld + i] = ok ? (int32_t)id : -1;
}

// add: row r of the chunk's tiled staging goes to slot dst[r]; one thread per (row, 16-byte unit)
__global__ void ivf_scatter_kernel(const uint4* src, uint4* corpus, const int64_t* dst, int64_t n, int kg,
                                   int64_t id0, int64_t* slot2id, int64_t* id2slot, uint32_t* blk_valid) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)kg * 2;
  if (t >= n * per) return;
  const int64_t r = t / per;
  const int u = (int)(t % per);
  const int g = u >> 1, hh = u & 1;
  const int64_t s = dst[r];
  corpus[((s >> 5) * kg + g) * 64 + hh * 32 + (s & 31)] = src[((r >> 5) * kg + g) * 64 + hh * 32 + (r & 31)];
  if (u == 0) {
    slot2id[s] = id0 + r;
    id2slot[id0 + r] = s;
    atomicOr(&blk_valid[s >> 5], 1u << (s & 31));
  }
}

// remove (ts_remove_ivf): the slot of each id in [0, ntotal) leaves its block's valid word and slot2id; lists[i] = the
// list of a slot this call freed, else -1.  id2slot keeps the slot, so that reconstruct still reads the stored row.
__global__ void ivf_remove_kernel(const int64_t* ids, int64_t n, int64_t id_offset, int64_t ntotal,
                                  const int64_t* id2slot, const int32_t* blk_list, uint32_t* blk_valid,
                                  int64_t* slot2id, int32_t* lists) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = ids[i] - id_offset;
  int32_t l = -1;
  if (r >= 0 && r < ntotal) {
    const int64_t s = id2slot[r];
    const uint32_t bit = 1u << (s & 31);
    if (atomicAnd(&blk_valid[s >> 5], ~bit) & bit) {
      slot2id[s] = -1;
      l = blk_list[s >> 5];
    }
  }
  lists[i] = l;
}

// reconstruct in id order: out[i] = stored row of id id0 + i, as float32
__global__ void ivf_reconstruct_kernel(const uint4* corpus, const int64_t* id2slot, int64_t id0, int64_t n, int dim,
                                       int kg, int dt, float* out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * dim) return;
  const int64_t i = t / dim;
  const int k = (int)(t % dim);
  const int64_t s = id2slot[id0 + i];
  const int g = k >> 4, hh = (k >> 3) & 1, e = k & 7;
  const uint16_t* u = reinterpret_cast<const uint16_t*>(corpus + ((s >> 5) * kg + g) * 64 + hh * 32 + (s & 31));
  const uint32_t v = u[e];
  out[t] = dt == TS_F16 ? (float)__builtin_bit_cast(_Float16, (uint16_t)v) : __uint_as_float(v << 16);
}

// training points: x[idx[i]] (x_dtype) -> fp32 rows
template <typename T>
__global__ void ivf_gather_kernel(const T* x, const int64_t* idx, int64_t n, int dim, float* out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * dim) return;
  const int64_t i = t / dim;
  out[t] = ElemIO<T>::ld(x + idx[i] * dim + (t % dim));
}

// k-means update, deterministic: centroid c = sum of its members in ascending point order (perm[offs[c]..offs[c+1])),
// one workgroup per centroid, a thread per dimension; empty clusters keep their centroid (split on the host's order)
__global__ void ivf_centroid_sum_kernel(const float* x, const int32_t* perm, const int64_t* offs, int dim, float* cent) {
  const int c = blockIdx.x;
  const int64_t b = offs[c], e = offs[c + 1];
  if (b == e) return;
  for (int j = threadIdx.x; j < dim; j += blockDim.x) {
    float s = 0.f;
    for (int64_t i = b; i < e; ++i) s += x[(int64_t)perm[i] * dim + j];
    cent[(int64_t)c * dim + j] = s;
  }
}

// FAISS split_clusters: the empty centroid ci takes a perturbed copy of cj, which is perturbed the other way
__global__ void ivf_split_kernel(float* cent, int dim, int ci, int cj, float eps) {
  for (int j = threadIdx.x; j < dim; j += blockDim.x) {
    const float v = cent[(int64_t)cj * dim + j];
    const bool even = (j & 1) == 0;
    cent[(int64_t)ci * dim + j] = v * (even ? 1.f + eps : 1.f - eps);
    cent[(int64_t)cj * dim + j] = v * (even ? 1.f - eps : 1.f + eps);
  }
}

// spherical k-means: every centroid L2-normalised (fixed reduction order: deterministic)
__global__ __launch_bounds__(256) void ivf_normalize_kernel(float* cent, int dim) {
  __shared__ float red[256];
  float* c = cent + (int64_t)blockIdx.x * dim;
  float s = 0.f;
  for (int j = threadIdx.x; j < dim; j += 256) s += c[j] * c[j];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float nrm = sqrtf(red[0]);
  if (nrm > 0.f)
    for (int j = threadIdx.x; j < dim; j += 256) c[j] = c[j] / nrm;
}

// ------------------------------------------------------------------ host helpers
static size_t ivf_scan_lds(const TsLayout& L, int qh, int mode) { return ts_scan_lds(L.kg, qh, mode, sizeof(StageLds)); }

template <int DT, int QH, int MODE>
static int launch_ivf_t(const TsLayout& L, const IvfScanParams& p, int grid, hipStream_t s) {
  auto kern = scan_ivf_kernel<DT, QH, MODE>;
  static TsDeviceOnce lds_attr;
  TS_CHECK(ts_allow_max_lds(lds_attr, reinterpret_cast<const void*>(kern)));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(SCAN_THREADS), ivf_scan_lds(L, QH, MODE), s, p);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

static int launch_ivf_scan(const TsLayout& L, int mode, int qh, const IvfScanParams& p, int grid, hipStream_t s) {
  if (grid < 1) grid = 1;
  if (L.dtype == TS_F16) {
    if (mode == SCAN_DENSE) return qh == 1 ? launch_ivf_t<TS_F16, 1, SCAN_DENSE>(L, p, grid, s)
                                           : launch_ivf_t<TS_F16, 2, SCAN_DENSE>(L, p, grid, s);
    return qh == 1 ? launch_ivf_t<TS_F16, 1, SCAN_FILTER>(L, p, grid, s)
                   : launch_ivf_t<TS_F16, 2, SCAN_FILTER>(L, p, grid, s);
  }
  if (mode == SCAN_DENSE) return qh == 1 ? launch_ivf_t<TS_BF16, 1, SCAN_DENSE>(L, p, grid, s)
                                         : launch_ivf_t<TS_BF16, 2, SCAN_DENSE>(L, p, grid, s);
  return qh == 1 ? launch_ivf_t<TS_BF16, 1, SCAN_FILTER>(L, p, grid, s)
                 : launch_ivf_t<TS_BF16, 2, SCAN_FILTER>(L, p, grid, s);
}

// the quantizer's exact top-k of `n` fp32 / f16 / bf16 rows against the centroids, in asynchronous slices (its dense
// path: nothing to verify); the results are complete in stream order
static int ivf_quant_topk(ts_ivf* h, const void* x, int64_t n, int dt, int k, float* out_s, int64_t* out_i,
                          hipStream_t s) {
  const size_t row = (size_t)h->L.dim * (dt == TS_F32 ? 4 : 2);
  const TsLayout QL = ts_make_layout(h->L.dim, TS_F32);
  const int64_t slice = ts_queries_per_pass(QL) * 4;
  for (int64_t r0 = 0; r0 < n; r0 += slice) {
    const int c = (int)std::min(slice, n - r0);
    TS_CHECK(ts_index_search(h->quant, (const char*)x + (size_t)r0 * row, c, dt, k, out_s + (size_t)r0 * k,
                             out_i + (size_t)r0 * k, TS_FLAG_ASYNC, s));
  }
  return TS_OK;
}

static int ivf_load_centroids(ts_ivf* h, const float* cent, hipStream_t s) {
  TS_CHECK(ts_index_reset(h->quant));
  TS_CHECK(ts_index_add(h->quant, cent, h->nlist, TS_F32, 0, s));
  return TS_OK;
}

// ------------------------------------------------------------------ C ABI
extern "C" int ts_ivf_create(int32_t dim, int32_t nlist, int32_t storage_dtype, int32_t device, ts_ivf** out) {
  if (!out) { ts_set_error("out is null"); return TS_ERR_INVALID; }
  *out = nullptr;
  if (dim <= 0 || dim > 65536) { ts_set_error("bad dim %d", dim); return TS_ERR_INVALID; }
  if (nlist < 1 || nlist > kIvfMaxList) { ts_set_error("nlist %d outside [1, %d]", nlist, kIvfMaxList); return TS_ERR_INVALID; }
  if (storage_dtype != TS_F16 && storage_dtype != TS_BF16) {
    ts_set_error("IVF storage dtype must be f16 or bf16, got %d", storage_dtype);
    return TS_ERR_INVALID;
  }
  const TsLayout L = ts_make_layout(dim, storage_dtype);
  if (ivf_scan_lds(L, 1, SCAN_FILTER) > TS_LDS_BYTES) {
    ts_set_error("dim %d too large for the LDS-resident query image", dim);
    return TS_ERR_UNSUPPORTED;
  }
  int ndev = 0;
  TS_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) { ts_set_error("device %d not present (%d HIP devices)", device, ndev); return TS_ERR_INVALID; }
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  ts_ivf* h = new (std::nothrow) ts_ivf();
  if (!h) { ts_set_error("out of host memory"); return TS_ERR_OOM; }
  h->device = device;
  h->nlist = nlist;
  h->pwords = (nlist + 31) / 32;
  h->L = L;
  h->list_blocks.resize(nlist);
  h->list_size.assign(nlist, 0);
  h->list_removed.assign(nlist, 0);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    h->num_cus = prop.multiProcessorCount;
  int st = ts_index_create(dim, TS_F32, TS_METRIC_INNER_PRODUCT, device, &h->quant);
  if (st == TS_OK) st = ts_buf_ensure(h->small, 4096);
  if (st == TS_OK) st = ts_buf_ensure(h->dlist_size, (size_t)nlist * 8);
  if (st == TS_OK && (hipMemset(h->small.p, 0, 4096) != hipSuccess || hipMemset(h->dlist_size.p, 0, (size_t)nlist * 8) != hipSuccess)) {
    ts_set_error("hipMemset failed");
    st = TS_ERR_HIP;
  }
  if (st == TS_OK && hipStreamSynchronize(nullptr) != hipSuccess) {   // (as in ts_ivf_reset: done before any stream's first use)
    ts_set_error("hipStreamSynchronize failed");
    st = TS_ERR_HIP;
  }
  if (st == TS_OK &&
      (hipHostMalloc((void**)&h->host_rep, 128 * 4, hipHostMallocMapped) != hipSuccess ||
       hipHostGetDevicePointer((void**)&h->host_rep_dev, h->host_rep, 0) != hipSuccess)) {
    ts_set_error("hipHostMalloc(mapped) failed");
    st = TS_ERR_HIP;
  }
  if (st != TS_OK) {
    ts_ivf_destroy(h);
    return st;
  }
  *out = h;
  return TS_OK;
}

extern "C" int ts_ivf_destroy(ts_ivf* h) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  TsDeviceGuard g(h->device);
  (void)hipDeviceSynchronize();
  if (h->quant) ts_index_destroy(h->quant);
  TsDevBuf* bufs[] = {&h->corpus, &h->blk_list, &h->blk_valid, &h->slot2id, &h->id2slot, &h->dlist_size,
                      &h->tmp_tiled, &h->tmp_f32, &h->den, &h->assign, &h->ascore, &h->dst, &h->qimg, &h->small,
                      &h->pid, &h->pscore, &h->bits, &h->live, &h->sample, &h->cand_score, &h->cand_id, &h->dense,
                      &h->mids, &h->list_score, &h->list_id, &h->train_x, &h->cent, &h->perm, &h->offs,
                      &h->upd_ids};
  for (TsDevBuf* b : bufs) ts_buf_release(*b);
  if (h->host_rep) (void)hipHostFree(h->host_rep);
  ts_mmr_release(h->mmr);
  delete h;
  return TS_OK;
}

extern "C" int ts_ivf_reset(ts_ivf* h) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  TsDeviceGuard g(h->device);
  // The list sizes are cleared on the null stream, which a non-blocking caller stream does not wait for, and a memset
  // of device memory need not be complete when hipMemset returns: the next add, on any stream, must find it done.
  TS_HIP(hipMemset(h->dlist_size.p, 0, (size_t)h->nlist * 8));
  TS_HIP(hipStreamSynchronize(nullptr));
  h->ntotal = 0;
  h->nblocks = 0;
  for (auto& v : h->list_blocks) v.clear();
  std::fill(h->list_size.begin(), h->list_size.end(), 0);
  std::fill(h->list_removed.begin(), h->list_removed.end(), 0);
  return TS_OK;
}

extern "C" int64_t ts_ivf_ntotal(const ts_ivf* h) { return h ? h->ntotal : -1; }

// removal with the contract of ts_index_remove (include/tristage.h): removed ids keep their slots as holes until
// ts_compact_ivf; the live list sizes feed the thresholds' N_q
extern "C" int ts_remove_ivf(ts_ivf* h, const int64_t* ids, int64_t n, int64_t* n_removed, void* stream) {
  if (!h || !n_removed || n < 0 || (n > 0 && !ids)) { ts_set_error("bad arguments to remove"); return TS_ERR_INVALID; }
  *n_removed = 0;
  if (n == 0 || h->ntotal == 0) return TS_OK;
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunk = std::min<int64_t>(n, 1 << 20);
  TS_CHECK(ts_buf_ensure(h->dst, (size_t)chunk * 8));
  TS_CHECK(ts_buf_ensure(h->assign, (size_t)chunk * 8));
  std::vector<int32_t> lists(chunk);
  std::vector<int64_t> live_size(h->nlist);
  int64_t cleared = 0;
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    const int64_t c = std::min(chunk, n - i0);
    TS_HIP(hipMemcpyAsync(h->dst.p, ids + i0, (size_t)c * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ivf_remove_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, s, (const int64_t*)h->dst.p,
                       c, h->id_offset, h->ntotal, (const int64_t*)h->id2slot.p, (const int32_t*)h->blk_list.p,
                       (uint32_t*)h->blk_valid.p, (int64_t*)h->slot2id.p, (int32_t*)h->assign.p);
    TS_HIP(hipGetLastError());
    TS_HIP(hipMemcpyAsync(lists.data(), h->assign.p, (size_t)c * 4, hipMemcpyDeviceToHost, s));
    TS_HIP(hipStreamSynchronize(s));
    for (int64_t i = 0; i < c; ++i)
      if (lists[i] >= 0) { ++h->list_removed[lists[i]]; ++cleared; }
  }
  for (int l = 0; l < h->nlist; ++l) live_size[l] = h->list_size[l] - h->list_removed[l];
  TS_HIP(hipMemcpyAsync(h->dlist_size.p, live_size.data(), (size_t)h->nlist * 8, hipMemcpyHostToDevice, s));
  TS_HIP(hipStreamSynchronize(s));
  *n_removed = cleared;
  return TS_OK;
}
extern "C" int32_t ts_ivf_is_trained(const ts_ivf* h) { return h ? (h->trained ? 1 : 0) : -1; }

extern "C" int ts_ivf_set_id_offset(ts_ivf* h, int64_t offset) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  h->id_offset = offset;
  return TS_OK;
}

extern "C" int ts_ivf_list_sizes(const ts_ivf* h, int64_t* out) {
  if (!h || !out) { ts_set_error("bad arguments to list_sizes"); return TS_ERR_INVALID; }
  for (int l = 0; l < h->nlist; ++l) out[l] = h->list_size[l] - h->list_removed[l];
  return TS_OK;
}

extern "C" int ts_ivf_last_search_info(const ts_ivf* h, int64_t info[4]) {
  if (!h || !info) { ts_set_error("bad arguments to last_search_info"); return TS_ERR_INVALID; }
  for (int i = 0; i < 4; ++i) info[i] = h->info[i];
  return TS_OK;
}

extern "C" int ts_ivf_set_centroids(ts_ivf* h, const float* centroids, void* stream) {
  if (!h || !centroids) { ts_set_error("bad arguments to set_centroids"); return TS_ERR_INVALID; }
  if (h->ntotal > 0) { ts_set_error("set_centroids on a non-empty IVF index: reset() first"); return TS_ERR_INVALID; }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(ivf_load_centroids(h, centroids, s));
  TS_HIP(hipStreamSynchronize(s));
  h->trained = true;
  return TS_OK;
}

extern "C" int ts_ivf_get_centroids(ts_ivf* h, float* out, void* stream) {
  if (!h || !out) { ts_set_error("bad arguments to get_centroids"); return TS_ERR_INVALID; }
  if (!h->trained) { ts_set_error("the IVF index is not trained"); return TS_ERR_INVALID; }
  TsDeviceGuard g(h->device);
  return ts_index_reconstruct(h->quant, 0, h->nlist, out, 0, stream);
}

extern "C" int ts_ivf_train(ts_ivf* h, const void* x, int64_t n, int32_t x_dtype, int64_t seed, int32_t iters,
                            double* objective, void* stream) {
  if (!h || !x || n < 0 || iters < 0 || (x_dtype != TS_F32 && x_dtype != TS_F16 && x_dtype != TS_BF16)) {
    ts_set_error("bad arguments to train");
    return TS_ERR_INVALID;
  }
  if (n < h->nlist) {
    ts_set_error("%lld training points for %d lists: need at least nlist", (long long)n, h->nlist);
    return TS_ERR_INVALID;
  }
  if (h->ntotal > 0) { ts_set_error("train on a non-empty IVF index: reset() first"); return TS_ERR_INVALID; }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int dim = h->L.dim, nl = h->nlist;
  // the training sample and the initial centroids: a seeded partial Fisher-Yates shuffle of the point ids
  const int64_t nt = std::min<int64_t>(n, (int64_t)kIvfTrainPerList * nl);
  std::vector<int64_t> ids(n);
  for (int64_t i = 0; i < n; ++i) ids[i] = i;
  uint64_t rs = (uint64_t)seed;
  for (int64_t i = 0; i < nt; ++i) {
    const int64_t j = i + (int64_t)(splitmix64(rs) % (uint64_t)(n - i));
    std::swap(ids[i], ids[j]);
  }
  TS_CHECK(ts_buf_ensure(h->perm, (size_t)std::max<int64_t>(nt, 1) * 8));
  TS_CHECK(ts_buf_ensure(h->train_x, (size_t)nt * dim * 4));
  TS_CHECK(ts_buf_ensure(h->cent, (size_t)nl * dim * 4));
  TS_CHECK(ts_buf_ensure(h->assign, (size_t)nt * 8));
  TS_CHECK(ts_buf_ensure(h->ascore, (size_t)nt * 4));
  TS_CHECK(ts_buf_ensure(h->offs, (size_t)(nl + 1) * 8));
  TS_HIP(hipMemcpyAsync(h->perm.p, ids.data(), (size_t)nt * 8, hipMemcpyHostToDevice, s));
  const int64_t tot = nt * dim;
  const unsigned gb = (unsigned)((tot + 255) / 256);
  if (x_dtype == TS_F32)
    hipLaunchKernelGGL(ivf_gather_kernel<float>, dim3(gb), dim3(256), 0, s, (const float*)x, (const int64_t*)h->perm.p, nt, dim, (float*)h->train_x.p);
  else if (x_dtype == TS_F16)
    hipLaunchKernelGGL(ivf_gather_kernel<_Float16>, dim3(gb), dim3(256), 0, s, (const _Float16*)x, (const int64_t*)h->perm.p, nt, dim, (float*)h->train_x.p);
  else
    hipLaunchKernelGGL(ivf_gather_kernel<__bf16>, dim3(gb), dim3(256), 0, s, (const __bf16*)x, (const int64_t*)h->perm.p, nt, dim, (float*)h->train_x.p);
  TS_HIP(hipGetLastError());
  float* cent = (float*)h->cent.p;
  // initial centroids: the first nlist points of the sample (distinct points), normalised
  TS_HIP(hipMemcpyAsync(cent, h->train_x.p, (size_t)nl * dim * 4, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(ivf_normalize_kernel, dim3(nl), dim3(256), 0, s, cent, dim);
  TS_HIP(hipGetLastError());
  std::vector<int64_t> asg(nt), cnt(nl), offs(nl + 1);
  std::vector<float> sc(nt);
  std::vector<int32_t> order(nt);
  for (int it = 0; it < iters; ++it) {
    TS_CHECK(ivf_load_centroids(h, cent, s));
    TS_CHECK(ivf_quant_topk(h, h->train_x.p, nt, TS_F32, 1, (float*)h->ascore.p, (int64_t*)h->assign.p, s));
    TS_HIP(hipMemcpyAsync(asg.data(), h->assign.p, (size_t)nt * 8, hipMemcpyDeviceToHost, s));
    TS_HIP(hipMemcpyAsync(sc.data(), h->ascore.p, (size_t)nt * 4, hipMemcpyDeviceToHost, s));
    TS_HIP(hipStreamSynchronize(s));
    if (objective) {
      double o = 0.0;
      for (int64_t i = 0; i < nt; ++i) o += sc[i];
      objective[it] = o;
    }
    // members of each centroid in ascending point order (counting sort)
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int64_t i = 0; i < nt; ++i) {
      if (asg[i] < 0 || asg[i] >= nl) { ts_set_error("k-means: bad assignment %lld", (long long)asg[i]); return TS_ERR_HIP; }
      ++cnt[asg[i]];
    }
    offs[0] = 0;
    for (int c = 0; c < nl; ++c) offs[c + 1] = offs[c] + cnt[c];
    std::vector<int64_t> fill(offs.begin(), offs.end() - 1);
    for (int64_t i = 0; i < nt; ++i) order[fill[asg[i]]++] = (int32_t)i;
    TS_HIP(hipMemcpyAsync(h->perm.p, order.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
    TS_HIP(hipMemcpyAsync(h->offs.p, offs.data(), (size_t)(nl + 1) * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ivf_centroid_sum_kernel, dim3(nl), dim3(256), 0, s, (const float*)h->train_x.p,
                       (const int32_t*)h->perm.p, (const int64_t*)h->offs.p, dim, cent);
    TS_HIP(hipGetLastError());
    // empty clusters: split the largest (lowest id on ties), as FAISS does with its count bookkeeping
    for (int c = 0; c < nl; ++c) {
      if (cnt[c] != 0) continue;
      int big = 0;
      for (int j = 1; j < nl; ++j) if (cnt[j] > cnt[big]) big = j;
      hipLaunchKernelGGL(ivf_split_kernel, dim3(1), dim3(256), 0, s, cent, dim, c, big, kIvfSplitEps);
      TS_HIP(hipGetLastError());
      cnt[c] = cnt[big] / 2;
      cnt[big] -= cnt[c];
    }
    hipLaunchKernelGGL(ivf_normalize_kernel, dim3(nl), dim3(256), 0, s, cent, dim);
    TS_HIP(hipGetLastError());
    TS_HIP(hipStreamSynchronize(s));   // (order / offs are reused by the next iteration)
  }
  TS_CHECK(ivf_load_centroids(h, cent, s));
  TS_HIP(hipStreamSynchronize(s));
  h->trained = true;
  return TS_OK;
}

static int ivf_grow_blocks(ts_ivf* h, int64_t need, hipStream_t s) {
  const size_t bb = ts_block_bytes(h->L);
  const int64_t used = h->nblocks;
  TS_CHECK(ivf_grow(h->corpus, (size_t)need * bb, (size_t)used * bb, s));
  TS_CHECK(ivf_grow(h->blk_list, (size_t)need * 4, (size_t)used * 4, s));
  TS_CHECK(ivf_grow(h->blk_valid, (size_t)need * 4, (size_t)used * 4, s));
  TS_CHECK(ivf_grow(h->slot2id, (size_t)need * 32 * 8, (size_t)used * 32 * 8, s));
  // fresh blocks: zero rows, no occupied slot
  TS_HIP(hipMemsetAsync((char*)h->corpus.p + (size_t)used * bb, 0, (size_t)(need - used) * bb, s));
  TS_HIP(hipMemsetAsync((uint32_t*)h->blk_valid.p + used, 0, (size_t)(need - used) * 4, s));
  TS_HIP(hipMemsetAsync((int64_t*)h->slot2id.p + used * 32, 0xFF, (size_t)(need - used) * 32 * 8, s));
  return TS_OK;
}

// The placement rule of the index: rows take their slots in the order given, each the next slot of its list; a list
// continues in its last block, and one whose last block is full (or that has none) takes the next fresh block at the
// end.  asg[r] = list of row r (in [0, nlist); a negative entry is no row and gets dst -1).  Appends to list_blocks /
// list_size and *nblocks; new_lists receives the list of every block taken, in block order.
template <typename A, typename D>
static void ivf_place(std::vector<std::vector<int32_t>>& list_blocks, std::vector<int64_t>& list_size, int64_t* nblocks,
                      const A* asg, int64_t n, D* dst, std::vector<int32_t>* new_lists) {
  int64_t nb = *nblocks;
  for (int64_t r = 0; r < n; ++r) {
    const int64_t l = (int64_t)asg[r];
    if (l < 0) { dst[r] = (D)-1; continue; }
    const int64_t pos = list_size[l];
    if (pos % 32 == 0) {
      list_blocks[l].push_back((int32_t)nb++);
      new_lists->push_back((int32_t)l);
    }
    dst[r] = (D)((int64_t)list_blocks[l][pos / 32] * 32 + pos % 32);
    ++list_size[l];
  }
  *nblocks = nb;
}

extern "C" int ts_ivf_add(ts_ivf* h, const void* rows, int64_t n, int32_t rows_dtype, uint32_t flags, void* stream) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  if (n == 0) return TS_OK;
  if (!rows || n < 0 || (rows_dtype != TS_F32 && rows_dtype != TS_F16 && rows_dtype != TS_BF16) ||
      (flags & TS_FLAG_HOST_PTR)) {
    ts_set_error("bad arguments to add (device rows of f32 / f16 / bf16)");
    return TS_ERR_INVALID;
  }
  if (!h->trained) { ts_set_error("add before train: the IVF index has no centroids"); return TS_ERR_INVALID; }
  if ((h->ntotal + n) + 32LL * h->nlist >= (1LL << 31)) { ts_set_error("at most 2^31 slots per IVF index"); return TS_ERR_UNSUPPORTED; }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const bool norm = (flags & TS_FLAG_NORMALIZE) != 0;
  const size_t row_bytes = (size_t)h->L.dim * (rows_dtype == TS_F32 ? 4 : 2);
  const int64_t chunk = std::min(n, kIvfAddChunkRows);
  const int64_t cblk = (chunk + 31) / 32;
  TS_CHECK(ts_buf_ensure(h->tmp_tiled, (size_t)cblk * ts_block_bytes(h->L)));
  TS_CHECK(ts_buf_ensure(h->tmp_f32, (size_t)chunk * h->L.dim * 4));
  TS_CHECK(ts_buf_ensure(h->den, (size_t)chunk * 4));
  TS_CHECK(ts_buf_ensure(h->assign, (size_t)chunk * 8));
  TS_CHECK(ts_buf_ensure(h->ascore, (size_t)chunk * 4));
  TS_CHECK(ts_buf_ensure(h->dst, (size_t)chunk * 8));
  std::vector<int64_t> asg(chunk), dst(chunk), live_size(h->nlist);
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t c = std::min(chunk, n - r0);
    // the flat index's relayout (same rounding and normalisation), then the stored rows back as fp32 for the assignment
    TS_CHECK(ts_launch_relayout(h->L, (const char*)rows + (size_t)r0 * row_bytes, rows_dtype, c, 0,
                                (uint4*)h->tmp_tiled.p, norm, (float*)h->den.p, s));
    TS_CHECK(ts_launch_reconstruct(h->L, (const uint4*)h->tmp_tiled.p, 0, c, (float*)h->tmp_f32.p, s));
    TS_CHECK(ivf_quant_topk(h, h->tmp_f32.p, c, TS_F32, 1, (float*)h->ascore.p, (int64_t*)h->assign.p, s));
    TS_HIP(hipMemcpyAsync(asg.data(), h->assign.p, (size_t)c * 8, hipMemcpyDeviceToHost, s));
    TS_HIP(hipStreamSynchronize(s));
    // slots: a list continues in its last block, then takes fresh blocks at the end; rows keep id order in a list
    for (int64_t r = 0; r < c; ++r)
      if (asg[r] < 0 || asg[r] >= h->nlist) { ts_set_error("add: bad assignment %lld", (long long)asg[r]); return TS_ERR_HIP; }
    const int64_t old_blocks = h->nblocks;
    int64_t nb = h->nblocks;
    std::vector<int32_t> new_lists;
    ivf_place(h->list_blocks, h->list_size, &nb, asg.data(), c, dst.data(), &new_lists);
    if (nb > old_blocks) TS_CHECK(ivf_grow_blocks(h, nb, s));
    h->nblocks = nb;
    TS_CHECK(ivf_grow(h->id2slot, (size_t)(h->ntotal + c) * 8, (size_t)h->ntotal * 8, s));
    if (nb > old_blocks)
      TS_HIP(hipMemcpyAsync((int32_t*)h->blk_list.p + old_blocks, new_lists.data(), (size_t)(nb - old_blocks) * 4,
                            hipMemcpyHostToDevice, s));
    TS_HIP(hipMemcpyAsync(h->dst.p, dst.data(), (size_t)c * 8, hipMemcpyHostToDevice, s));
    const int64_t th = c * h->L.kg * 2;
    hipLaunchKernelGGL(ivf_scatter_kernel, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, s,
                       (const uint4*)h->tmp_tiled.p, (uint4*)h->corpus.p, (const int64_t*)h->dst.p, c, h->L.kg,
                       h->ntotal, (int64_t*)h->slot2id.p, (int64_t*)h->id2slot.p, (uint32_t*)h->blk_valid.p);
    TS_HIP(hipGetLastError());
    for (int l = 0; l < h->nlist; ++l) live_size[l] = h->list_size[l] - h->list_removed[l];
    TS_HIP(hipMemcpyAsync(h->dlist_size.p, live_size.data(), (size_t)h->nlist * 8, hipMemcpyHostToDevice, s));
    TS_HIP(hipStreamSynchronize(s));   // (staging reused by the next chunk; host tables read by the copies)
    h->ntotal += c;
  }
  return TS_OK;
}

// update in place, with the contract of ts_index_update (include/tristage.h): each row leaves its list as
// ts_remove_ivf makes it leave, is staged, read back and assigned as ts_ivf_add assigns a new row, and is placed at the
// end of its new list under its old id.  The hole stays, as after a removal, until ts_compact_ivf.
extern "C" int ts_update_ivf(ts_ivf* h, const int64_t* ids, int64_t n, const void* rows, int32_t rows_dtype,
                             uint32_t flags, void* stream) {
  if (!h || n < 0 || (n > 0 && (!ids || !rows)) ||
      (rows_dtype != TS_F32 && rows_dtype != TS_F16 && rows_dtype != TS_BF16) || (flags & TS_FLAG_HOST_PTR)) {
    ts_set_error("bad arguments to update (device rows of f32 / f16 / bf16)");
    return TS_ERR_INVALID;
  }
  if (n == 0) return TS_OK;
  std::vector<int64_t> loc((size_t)n);
  std::vector<uint64_t> keys;
  TS_CHECK(ts_update_check_ids(ids, n, h->id_offset, h->ntotal, loc.data(), &keys));
  if (h->nblocks * 32 + n + 32LL * h->nlist >= (1LL << 31)) { ts_set_error("at most 2^31 slots per IVF index"); return TS_ERR_UNSUPPORTED; }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const bool norm = (flags & TS_FLAG_NORMALIZE) != 0;
  const size_t row_bytes = (size_t)h->L.dim * (rows_dtype == TS_F32 ? 4 : 2);
  const int64_t chunk = std::min(n, kIvfAddChunkRows);
  const int64_t cblk = (chunk + 31) / 32;
  TS_CHECK(ts_buf_ensure(h->tmp_tiled, (size_t)cblk * ts_block_bytes(h->L)));
  TS_CHECK(ts_buf_ensure(h->tmp_f32, (size_t)chunk * h->L.dim * 4));
  TS_CHECK(ts_buf_ensure(h->den, (size_t)chunk * 4));
  TS_CHECK(ts_buf_ensure(h->assign, (size_t)chunk * 8));
  TS_CHECK(ts_buf_ensure(h->ascore, (size_t)chunk * 4));
  TS_CHECK(ts_buf_ensure(h->dst, (size_t)chunk * 8));
  TS_CHECK(ts_buf_ensure(h->upd_ids, (size_t)chunk * 8 + 256));
  unsigned long long* cnt = (unsigned long long*)((char*)h->upd_ids.p + (size_t)chunk * 8);
  // a removed id cannot be updated: every id is checked before the first row moves
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    const int64_t c = std::min(chunk, n - i0);
    unsigned long long dead[2] = {0ull, ~0ull};
    TS_HIP(hipMemcpyAsync(cnt, dead, 16, hipMemcpyHostToDevice, s));
    TS_HIP(hipMemcpyAsync(h->upd_ids.p, loc.data() + i0, (size_t)c * 8, hipMemcpyHostToDevice, s));
    TS_CHECK(ts_launch_update_ivf_check((const int64_t*)h->upd_ids.p, c, (const int64_t*)h->id2slot.p,
                                        (const int64_t*)h->slot2id.p, (const uint32_t*)h->blk_valid.p, cnt, s));
    TS_HIP(hipMemcpyAsync(dead, cnt, 16, hipMemcpyDeviceToHost, s));
    TS_HIP(hipStreamSynchronize(s));
    if (dead[0] != 0ull) {
      ts_set_error("update: id %lld was removed", (long long)ids[i0 + (int64_t)dead[1]]);
      return TS_ERR_INVALID;
    }
  }
  std::vector<int64_t> asg(chunk), dst(chunk), live_size(h->nlist);
  std::vector<int32_t> lists(chunk);
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t c = std::min(chunk, n - r0);
    // the new rows' lists, as ts_ivf_add finds them
    TS_CHECK(ts_launch_relayout(h->L, (const char*)rows + (size_t)r0 * row_bytes, rows_dtype, c, 0,
                                (uint4*)h->tmp_tiled.p, norm, (float*)h->den.p, s));
    TS_CHECK(ts_launch_reconstruct(h->L, (const uint4*)h->tmp_tiled.p, 0, c, (float*)h->tmp_f32.p, s));
    TS_CHECK(ivf_quant_topk(h, h->tmp_f32.p, c, TS_F32, 1, (float*)h->ascore.p, (int64_t*)h->assign.p, s));
    TS_HIP(hipMemcpyAsync(asg.data(), h->assign.p, (size_t)c * 8, hipMemcpyDeviceToHost, s));
    TS_HIP(hipStreamSynchronize(s));
    for (int64_t r = 0; r < c; ++r)
      if (asg[r] < 0 || asg[r] >= h->nlist) { ts_set_error("update: bad assignment %lld", (long long)asg[r]); return TS_ERR_HIP; }
    // the old rows leave their lists (ts_remove_ivf's kernel; ids without the offset)
    TS_HIP(hipMemcpyAsync(h->upd_ids.p, loc.data() + r0, (size_t)c * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ivf_remove_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, s,
                       (const int64_t*)h->upd_ids.p, c, (int64_t)0, h->ntotal, (const int64_t*)h->id2slot.p,
                       (const int32_t*)h->blk_list.p, (uint32_t*)h->blk_valid.p, (int64_t*)h->slot2id.p,
                       (int32_t*)h->assign.p);
    TS_HIP(hipGetLastError());
    TS_HIP(hipMemcpyAsync(lists.data(), h->assign.p, (size_t)c * 4, hipMemcpyDeviceToHost, s));
    TS_HIP(hipStreamSynchronize(s));
    for (int64_t i = 0; i < c; ++i)
      if (lists[i] >= 0) ++h->list_removed[lists[i]];
    // and take the next slots of their new ones
    const int64_t old_blocks = h->nblocks;
    int64_t nb = h->nblocks;
    std::vector<int32_t> new_lists;
    ivf_place(h->list_blocks, h->list_size, &nb, asg.data(), c, dst.data(), &new_lists);
    if (nb > old_blocks) TS_CHECK(ivf_grow_blocks(h, nb, s));
    h->nblocks = nb;
    if (nb > old_blocks)
      TS_HIP(hipMemcpyAsync((int32_t*)h->blk_list.p + old_blocks, new_lists.data(), (size_t)(nb - old_blocks) * 4,
                            hipMemcpyHostToDevice, s));
    TS_HIP(hipMemcpyAsync(h->dst.p, dst.data(), (size_t)c * 8, hipMemcpyHostToDevice, s));
    TS_CHECK(ts_launch_update_ivf_place(h->L, (const uint4*)h->tmp_tiled.p, (uint4*)h->corpus.p,
                                        (const int64_t*)h->dst.p, (const int64_t*)h->upd_ids.p, c,
                                        (int64_t*)h->slot2id.p, (int64_t*)h->id2slot.p, (uint32_t*)h->blk_valid.p, s));
    for (int l = 0; l < h->nlist; ++l) live_size[l] = h->list_size[l] - h->list_removed[l];
    TS_HIP(hipMemcpyAsync(h->dlist_size.p, live_size.data(), (size_t)h->nlist * 8, hipMemcpyHostToDevice, s));
    TS_HIP(hipStreamSynchronize(s));   // (staging reused by the next chunk; host tables read by the copies)
  }
  return TS_OK;
}

// Compaction (include/tristage.h): the index a fresh ts_ivf_add of the surviving rows, in id order and
// into the lists they are in, would build.  Out of place and all or nothing: the new corpus and tables are written
// beside the old ones (peak: old + new corpus) and take their place at the end; until then nothing of the index changes.
namespace {
struct IvfCompactBufs {   // the new index while it is built; after the swap, the old one
  TsDevBuf corpus, blk_list, blk_valid, slot2id, id2slot, dlist_size, src_slot;
  ~IvfCompactBufs() {
    TsDevBuf* bufs[] = {&corpus, &blk_list, &blk_valid, &slot2id, &id2slot, &dlist_size, &src_slot};
    for (TsDevBuf* b : bufs) ts_buf_release(*b);
  }
};
}  // namespace

extern "C" int ts_compact_ivf(ts_ivf* h, int64_t* old2new, void* stream) {
  if (!h) { ts_set_error("bad arguments to compact"); return TS_ERR_INVALID; }
  const int64_t n = h->ntotal;
  bool holes = false;
  for (int l = 0; l < h->nlist; ++l) holes = holes || h->list_removed[l] != 0;
  if (!holes) {   // (an empty index too) nothing to move
    if (old2new)
      for (int64_t i = 0; i < n; ++i) old2new[i] = i;
    return TS_OK;
  }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  // (1) the list of every id, -1 for a removed one
  std::vector<int32_t> lists((size_t)n);
  TS_CHECK(ts_buf_ensure(h->assign, (size_t)n * 4));
  TS_CHECK(ts_launch_ivf_compact_classify((const int64_t*)h->id2slot.p, (const int64_t*)h->slot2id.p,
                                          (const int32_t*)h->blk_list.p, n, (int32_t*)h->assign.p, s));
  TS_HIP(hipMemcpyAsync(lists.data(), h->assign.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  TS_HIP(hipStreamSynchronize(s));
  // (2) the survivors in id order and their places, by the placement routine of add
  std::vector<int64_t> live_size(h->nlist, 0);
  int64_t nlive = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t l = lists[i];
    if (l >= h->nlist) { ts_set_error("compact: bad list %d of id %lld", (int)l, (long long)i); return TS_ERR_HIP; }
    if (l >= 0) { ++live_size[l]; ++nlive; }
  }
  for (int l = 0; l < h->nlist; ++l)
    if (live_size[l] != h->list_size[l] - h->list_removed[l]) {
      ts_set_error("compact: list %d holds %lld live rows, its table says %lld", l, (long long)live_size[l],
                   (long long)(h->list_size[l] - h->list_removed[l]));
      return TS_ERR_HIP;
    }
  std::vector<int32_t> up((size_t)nlive * 2);   // new2old[nlive], then dst[nlive]
  int32_t* new2old = up.data();
  int32_t* dst = up.data() + nlive;
  {
    int64_t j = 0;
    for (int64_t i = 0; i < n; ++i)
      if (lists[i] >= 0) { new2old[j] = (int32_t)i; lists[j] = lists[i]; ++j; }   // (lists: now per new id)
  }
  std::vector<std::vector<int32_t>> new_blocks(h->nlist);
  std::vector<int64_t> new_size(h->nlist, 0);
  std::vector<int32_t> new_blk_list;
  int64_t nb = 0;
  for (int l = 0; l < h->nlist; ++l) new_blocks[l].reserve((size_t)((live_size[l] + 31) / 32));
  ivf_place(new_blocks, new_size, &nb, lists.data(), nlive, dst, &new_blk_list);
  // (3) the new corpus and tables beside the old ones
  IvfCompactBufs nw;
  TS_CHECK(ts_buf_ensure(nw.dlist_size, (size_t)h->nlist * 8));
  TS_HIP(hipMemcpyAsync(nw.dlist_size.p, new_size.data(), (size_t)h->nlist * 8, hipMemcpyHostToDevice, s));
  if (nlive > 0) {
    TS_CHECK(ts_buf_ensure(nw.corpus, (size_t)nb * ts_block_bytes(h->L)));
    TS_CHECK(ts_buf_ensure(nw.blk_list, (size_t)nb * 4));
    TS_CHECK(ts_buf_ensure(nw.blk_valid, (size_t)nb * 4));
    TS_CHECK(ts_buf_ensure(nw.slot2id, (size_t)nb * 32 * 8));
    TS_CHECK(ts_buf_ensure(nw.id2slot, (size_t)nlive * 8));
    TS_CHECK(ts_buf_ensure(nw.src_slot, (size_t)nb * 32 * 4));
    TS_CHECK(ts_buf_ensure(h->dst, (size_t)nlive * 8));
    TS_HIP(hipMemcpyAsync(h->dst.p, up.data(), (size_t)nlive * 8, hipMemcpyHostToDevice, s));
    TS_HIP(hipMemcpyAsync(nw.blk_list.p, new_blk_list.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
    TS_CHECK(ts_launch_ivf_compact_move(h->L, (const uint4*)h->corpus.p, (const int64_t*)h->id2slot.p,
                                        (const int32_t*)h->dst.p, (const int32_t*)h->dst.p + nlive, nlive, nb,
                                        (uint4*)nw.corpus.p, (int32_t*)nw.src_slot.p, (int64_t*)nw.slot2id.p,
                                        (int64_t*)nw.id2slot.p, (uint32_t*)nw.blk_valid.p, s));
  }
  TS_HIP(hipStreamSynchronize(s));
  // (4) the swap: host state only from here on.  With no survivor the index keeps its (empty) buffers, as after reset.
  std::swap(h->dlist_size, nw.dlist_size);
  if (nlive > 0) {
    std::swap(h->corpus, nw.corpus);
    std::swap(h->blk_list, nw.blk_list);
    std::swap(h->blk_valid, nw.blk_valid);
    std::swap(h->slot2id, nw.slot2id);
    std::swap(h->id2slot, nw.id2slot);
  }
  h->list_blocks.swap(new_blocks);
  h->list_size.swap(new_size);
  std::fill(h->list_removed.begin(), h->list_removed.end(), 0);
  h->nblocks = nb;
  h->ntotal = nlive;
  if (old2new) {
    int64_t j = 0, i = 0;
    for (; j < nlive; ++j) {
      for (; i < new2old[j]; ++i) old2new[i] = -1;
      old2new[i++] = j;
    }
    for (; i < n; ++i) old2new[i] = -1;
  }
  return TS_OK;
}

extern "C" int ts_ivf_reconstruct(ts_ivf* h, int64_t id0, int64_t n, float* out, void* stream) {
  if (!h || !out || id0 < 0 || n < 0 || id0 + n > h->ntotal) { ts_set_error("bad arguments to reconstruct"); return TS_ERR_INVALID; }
  if (n == 0) return TS_OK;
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int64_t t = n * h->L.dim;
  hipLaunchKernelGGL(ivf_reconstruct_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s,
                     (const uint4*)h->corpus.p, (const int64_t*)h->id2slot.p, id0, n, h->L.dim, h->L.kg, h->L.dtype, out);
  TS_HIP(hipGetLastError());
  TS_HIP(hipStreamSynchronize(s));
  return TS_OK;
}

// MMR over the rows of an IVF index (kernels: ts_mmr.hip; outside the ts_ivf_ prefix, as ts_remove_ivf)
extern "C" int ts_mmr_ivf(ts_ivf* h, const int64_t* cand_ids, const float* cand_rel, int32_t nq, int32_t fetch_k,
                          int32_t k, float lambda, float* out_rel, int64_t* out_ids, uint32_t flags, void* stream) {
  TS_CHECK(ts_mmr_check_args(h, cand_ids, cand_rel, nq, fetch_k, k, lambda, out_rel, out_ids));
  if (nq == 0) return TS_OK;
  TsDeviceGuard g(h->device);
  TsMmrSource src;
  src.corpus = (const uint4*)h->corpus.p;
  src.L = h->L;
  src.ntotal = h->ntotal;
  src.id_offset = h->id_offset;
  src.ivf = true;
  src.live = nullptr;
  src.id2slot = (const int64_t*)h->id2slot.p;
  src.blk_valid = (const uint32_t*)h->blk_valid.p;
  return ts_mmr_run(src, h->mmr, cand_ids, cand_rel, nq, fetch_k, k, lambda, out_rel, out_ids, flags,
                    (hipStream_t)stream);
}

extern "C" int ts_ivf_probe(ts_ivf* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t nprobe,
                            float* out_scores, int64_t* out_lists, void* stream) {
  if (!h || !queries || !out_scores || !out_lists || nq < 0 || nprobe <= 0 ||
      (q_dtype != TS_F32 && q_dtype != TS_F16 && q_dtype != TS_BF16)) {
    ts_set_error("bad arguments to probe");
    return TS_ERR_INVALID;
  }
  if (nprobe > h->nlist) { ts_set_error("nprobe %d > nlist %d", nprobe, h->nlist); return TS_ERR_INVALID; }
  if (!h->trained) { ts_set_error("the IVF index is not trained"); return TS_ERR_INVALID; }
  if (nq == 0) return TS_OK;
  TsDeviceGuard g(h->device);
  return ts_index_search(h->quant, queries, nq, q_dtype, nprobe, out_scores, out_lists, 0, stream);
}

// dense redo / small index: every slot scored, ids of the slots a query may see (else -1), exact select
static int ivf_dense(ts_ivf* h, int nq, int qh, int k, float* out_s, int64_t* out_i, hipStream_t s) {
  const int64_t N = h->nblocks * 32;
  const int64_t chunk_rows = std::min<int64_t>(kIvfDenseChunkRows, N);
  const int64_t nch = (N + chunk_rows - 1) / chunk_rows;
  TS_CHECK(ts_buf_ensure(h->dense, (size_t)nq * chunk_rows * 4));
  TS_CHECK(ts_buf_ensure(h->mids, (size_t)nq * chunk_rows * 4));
  if (nch > 1) {
    TS_CHECK(ts_buf_ensure(h->list_score, (size_t)nq * nch * k * 4));
    TS_CHECK(ts_buf_ensure(h->list_id, (size_t)nq * nch * k * 4));
  }
  for (int64_t c = 0; c < nch; ++c) {
    const int64_t row0 = c * chunk_rows;
    const int64_t rows = std::min(chunk_rows, N - row0);
    ScanParams sp{};
    sp.corpus = (const uint4*)h->corpus.p;
    sp.qimg = (const uint4*)h->qimg.p;
    sp.kg = h->L.kg;
    sp.nq = nq;
    sp.nwork = rows / 32;
    sp.blk0 = row0 / 32;
    sp.blk_stride = 1;
    sp.ntotal = N;
    sp.dense = (float*)h->dense.p;
    sp.dense_ld = chunk_rows;
    TS_CHECK(ts_launch_scan(h->L, SCAN_DENSE, qh, sp, h->num_cus, s));
    hipLaunchKernelGGL(ivf_dense_ids_kernel, dim3((unsigned)((rows + 255) / 256), nq), dim3(256), 0, s,
                       (const int32_t*)h->blk_list.p, (const int64_t*)h->slot2id.p, (const uint32_t*)h->bits.p,
                       h->pwords, nq, row0, (uint32_t)rows, chunk_rows, (int32_t*)h->mids.p);
    TS_HIP(hipGetLastError());
    SelParams p{};
    p.mode = SEL_PAIRS32;
    p.scores = (const float*)h->dense.p;
    p.ids32 = (const int32_t*)h->mids.p;
    p.stride = chunk_rows;
    p.n = (uint32_t)rows;
    p.k = k;
    if (nch == 1) {
      p.out_scores = out_s;
      p.out_ids64 = out_i;
      p.out_stride = k;
      p.id_offset = h->id_offset;
    } else {
      p.out_scores = (float*)h->list_score.p + c * k;
      p.out_ids32 = (int32_t*)h->list_id.p + c * k;
      p.out_stride = nch * k;
    }
    TS_CHECK(ts_launch_select(p, nq, s));
  }
  if (nch > 1) {
    SelParams p{};
    p.mode = SEL_PAIRS32;
    p.scores = (const float*)h->list_score.p;
    p.ids32 = (const int32_t*)h->list_id.p;
    p.stride = nch * k;
    p.n = (uint32_t)(nch * k);
    p.k = k;
    p.out_scores = out_s;
    p.out_ids64 = out_i;
    p.out_stride = k;
    p.id_offset = h->id_offset;
    TS_CHECK(ts_launch_select(p, nq, s));
  }
  return TS_OK;
}

static int ivf_pass(ts_ivf* h, const void* dq, int nq, int q_dtype, int k, int nprobe, float* out_s, int64_t* out_i,
                    hipStream_t s) {
  const int qh = nq > 32 ? 2 : 1;
  const int pw = h->pwords;
  // (1) the probed lists (the quantizer's exact top-nprobe), the probe bitmaps and their union
  TS_CHECK(ts_buf_ensure(h->pid, (size_t)TS_MAX_Q * nprobe * 8));
  TS_CHECK(ts_buf_ensure(h->pscore, (size_t)TS_MAX_Q * nprobe * 4));
  TS_CHECK(ts_buf_ensure(h->bits, (size_t)(TS_MAX_Q + 1) * pw * 4));
  TS_CHECK(ts_index_search(h->quant, dq, nq, q_dtype, nprobe, (float*)h->pscore.p, (int64_t*)h->pid.p, 0, s));
  TS_HIP(hipMemsetAsync(h->bits.p, 0, (size_t)(TS_MAX_Q + 1) * pw * 4, s));
  TS_HIP(hipMemsetAsync(h->nlive(), 0, 4, s));
  const int64_t np = (int64_t)nq * nprobe;
  hipLaunchKernelGGL(ivf_probe_bits_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s,
                     (const int64_t*)h->pid.p, nq, nprobe, pw, (uint32_t*)h->bits.p);
  TS_HIP(hipGetLastError());
  TS_CHECK(ts_buf_ensure(h->qimg, (size_t)h->L.kg * 2 * 1024));
  TS_CHECK(ts_launch_qprep(h->L, dq, q_dtype, nq, qh, (uint4*)h->qimg.p, h->cand_cnt(), h->status(), s));
  const int64_t N = h->nblocks * 32;
  const bool filter = k <= kIvfMaxFilterK && N >= kIvfMinFilterSlots;
  if (!filter) {
    TS_CHECK(ivf_dense(h, nq, qh, k, out_s, out_i, s));
    TS_HIP(hipStreamSynchronize(s));
    h->info[0] += 1;
    return TS_OK;
  }
  // (2) the live list: occupied blocks of a list some query of the pass probes
  TS_CHECK(ts_buf_ensure(h->live, (size_t)h->nblocks * 4));
  hipLaunchKernelGGL(ivf_live_kernel, dim3((unsigned)((h->nblocks + 255) / 256)), dim3(256), 0, s,
                     (const int32_t*)h->blk_list.p, (const uint32_t*)h->blk_valid.p, h->nblocks,
                     (const uint32_t*)h->bits.p + (size_t)TS_MAX_Q * pw, (int32_t*)h->live.p, h->nlive());
  TS_HIP(hipGetLastError());
  // (3) dense scores of a strided sample of the live list, (4) per-query thresholds from its probed rows
  const int64_t sitems = std::min<int64_t>(h->nblocks, std::max<int64_t>(kIvfMinSampleBlocks, h->nblocks / kIvfSampleDiv));
  const int64_t sld = sitems * 32;   // (bounds the device-side item count: nlive <= nblocks)
  TS_CHECK(ts_buf_ensure(h->sample, (size_t)nq * sld * 4));
  IvfScanParams ip{};
  ip.corpus = (const uint4*)h->corpus.p;
  ip.qimg = (const uint4*)h->qimg.p;
  ip.kg = h->L.kg;
  ip.nq = nq;
  ip.ntotal = N;
  ip.dense = (float*)h->sample.p;
  ip.dense_ld = sld;
  ip.live = (const int32_t*)h->live.p;
  ip.nlive = h->nlive();
  ip.blk_list = (const int32_t*)h->blk_list.p;
  ip.blk_valid = (const uint32_t*)h->blk_valid.p;
  ip.probe_bits = (const uint32_t*)h->bits.p;
  ip.pwords = pw;
  ip.sample_min = kIvfMinSampleBlocks;
  ip.sample_div = kIvfSampleDiv;
  TS_CHECK(launch_ivf_scan(h->L, SCAN_DENSE, qh, ip, (int)std::min<int64_t>((sitems + SCAN_WAVES - 1) / SCAN_WAVES, 2 * h->num_cus), s));
  const int64_t oversample = k > 1024 ? 3 : 4;
  uint32_t* rep = h->host_rep;
  for (int i = 0; i < 66; ++i) rep[i] = 0;
  hipLaunchKernelGGL(ivf_tau_kernel, dim3(TS_MAX_Q), dim3(IVF_TAU_THREADS), 0, s, (float*)h->sample.p, sld,
                     (int32_t)kIvfMinSampleBlocks, (int32_t)kIvfSampleDiv, (const int32_t*)h->live.p, (const uint32_t*)h->nlive(),
                     (const int32_t*)h->blk_list.p, (const uint32_t*)h->blk_valid.p, (const uint32_t*)h->bits.p, pw,
                     (const int64_t*)h->pid.p, nprobe, (const int64_t*)h->dlist_size.p, nq, k, (uint32_t)oversample,
                     kIvfMinSampleRank, h->tau(), h->need(), h->host_rep_dev + 65);
  TS_HIP(hipGetLastError());
  // (5) the filter scan over the live list
  TS_CHECK(ts_buf_ensure(h->cand_score, (size_t)TS_MAX_Q * kIvfCandCap * 4));
  TS_CHECK(ts_buf_ensure(h->cand_id, (size_t)TS_MAX_Q * kIvfCandCap * 4));
  ip.dense = nullptr;
  ip.tau = h->tau();
  ip.cand_cnt = h->cand_cnt();
  ip.cand_score = (float*)h->cand_score.p;
  ip.cand_id = (int32_t*)h->cand_id.p;
  ip.cand_cap = kIvfCandCap;
  const int scan_cus = h->num_cus - h->num_cus / 8;
  TS_CHECK(launch_ivf_scan(h->L, SCAN_FILTER, qh, ip, (int)std::min<int64_t>((h->nblocks + SCAN_WAVES - 1) / SCAN_WAVES, scan_cus), s));
  // (6) slot -> id, (7) exactness check and exact top-k of the candidates
  hipLaunchKernelGGL(ivf_remap_kernel, dim3(16, nq), dim3(256), 0, s, (int32_t*)h->cand_id.p,
                     (const uint32_t*)h->cand_cnt(), kIvfCandCap, nq, (const int64_t*)h->slot2id.p);
  TS_HIP(hipGetLastError());
  TS_CHECK(ts_launch_need_check(h->cand_cnt(), h->need(), nq, h->status(), h->host_rep_dev, s));
  SelParams p{};
  p.mode = SEL_PAIRS32;
  p.scores = (const float*)h->cand_score.p;
  p.ids32 = (const int32_t*)h->cand_id.p;
  p.stride = kIvfCandCap;
  p.n_per_q = h->cand_cnt();
  p.n_cap = kIvfCandCap;
  p.k = k;
  p.out_scores = out_s;
  p.out_ids64 = out_i;
  p.out_stride = k;
  p.id_offset = h->id_offset;
  p.status = h->status();
  p.host_report = h->host_rep_dev;
  TS_CHECK(ts_launch_select(p, nq, s));
  TS_HIP(hipStreamSynchronize(s));
  const bool redo = rep[64] != 0;
  h->info[0] += 1;
  h->info[1] += 1;
  h->info[3] = rep[65];
  if (redo) {
    // too few survivors for some query, or a candidate list overflowed (score ties): this pass again, exactly
    h->info[2] += 1;
    TS_CHECK(ivf_dense(h, nq, qh, k, out_s, out_i, s));
    TS_HIP(hipStreamSynchronize(s));
  }
  return TS_OK;
}

extern "C" int ts_ivf_search(ts_ivf* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t k, int32_t nprobe,
                             float* out_scores, int64_t* out_ids, void* stream) {
  if (!h || !queries || !out_scores || !out_ids || nq < 0 || k <= 0 || nprobe <= 0 ||
      (q_dtype != TS_F32 && q_dtype != TS_F16 && q_dtype != TS_BF16)) {
    ts_set_error("bad arguments to search");
    return TS_ERR_INVALID;
  }
  if (k > TS_SEL_LDS_KEYS) { ts_set_error("k=%d exceeds the supported maximum %d", k, TS_SEL_LDS_KEYS); return TS_ERR_UNSUPPORTED; }
  if (!h->trained) { ts_set_error("the IVF index is not trained"); return TS_ERR_INVALID; }
  if (nq == 0) return TS_OK;
  if (h->ntotal == 0) { ts_set_error("No documents indexed. Call add_documents() first."); return TS_ERR_EMPTY; }
  nprobe = std::min(nprobe, h->nlist);
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < 4; ++i) h->info[i] = 0;
  const int qp = ts_queries_per_pass(h->L);
  const size_t qrow = (size_t)h->L.dim * (q_dtype == TS_F32 ? 4 : 2);
  for (int q0 = 0; q0 < nq; q0 += qp) {
    const int c = std::min(qp, nq - q0);
    TS_CHECK(ivf_pass(h, (const char*)queries + (size_t)q0 * qrow, c, q_dtype, k, nprobe,
                      out_scores + (size_t)q0 * k, out_ids + (size_t)q0 * k, s));
  }
  return TS_OK;
}
