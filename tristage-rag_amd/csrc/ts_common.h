// Internal declarations shared by the HIP translation units of libtristage.so.
// Not part of the public ABI (that is include/tristage.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/tristage.h"

// ---------------------------------------------------------------- errors
void ts_set_error(const char* fmt, ...);

#define TS_HIP(call)                                                        \
  do {                                                                      \
    hipError_t e_ = (call);                                                 \
    if (e_ != hipSuccess) {                                                 \
      ts_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),   \
                   __FILE__, __LINE__);                                     \
      return (e_ == hipErrorOutOfMemory) ? TS_ERR_OOM : TS_ERR_HIP;         \
    }                                                                       \
  } while (0)

#define TS_CHECK(call)            \
  do {                            \
    int s_ = (call);              \
    if (s_ != TS_OK) return s_;   \
  } while (0)

// ---------------------------------------------------------------- once per device
// hipFuncSetAttribute (MaxDynamicSharedMemorySize) is a PER-DEVICE property of a kernel: a
// process that drives several GPUs (ts_index_create / ts_maxsim / ts_merge_topk all take a
// `device`) has to set it on each of them, and two host threads may reach the first launch at
// the same time.  One TsDeviceOnce per kernel instantiation: a bit per device, set under a
// mutex after the action succeeded (a failed action is retried by the next caller).
#include <atomic>
#include <mutex>
#include <vector>
#define TS_MAX_DEVICES 64
struct TsDeviceOnce {
  std::mutex mu;
  std::atomic<uint64_t> done{0};
};
template <class F>
static inline int ts_once_per_device(TsDeviceOnce& o, int dev, F&& action) {
  if (dev < 0 || dev >= TS_MAX_DEVICES) return action();  // untracked device: the action is idempotent
  const uint64_t bit = 1ull << dev;
  if (o.done.load(std::memory_order_acquire) & bit) return TS_OK;
  std::lock_guard<std::mutex> lk(o.mu);
  if (o.done.load(std::memory_order_relaxed) & bit) return TS_OK;
  const int st = action();
  if (st == TS_OK) o.done.fetch_or(bit, std::memory_order_release);
  return st;
}
#define TS_LDS_BYTES (160 * 1024)   // the LDS of a CU (gfx950)
// the 96-160 KiB LDS kernels: allow the full 160 KiB of dynamic LDS on the CURRENT device
static inline int ts_allow_max_lds(TsDeviceOnce& o, const void* kernel) {
  int dev = -1;
  TS_HIP(hipGetDevice(&dev));
  return ts_once_per_device(o, dev, [&]() -> int {
    TS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TS_LDS_BYTES));
    return TS_OK;
  });
}

// ---------------------------------------------------------------- host plumbing of the entry points
// Makes `dev` the calling thread's device for the guard's lifetime.  ok: hipSetDevice took it.  (Internal linkage: the
// library exports no symbol of it.)
namespace {
struct TsDeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit TsDeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~TsDeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};
}  // namespace

// A device buffer that only grows (its contents are not kept when it does).
struct TsDevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
static inline int ts_buf_ensure(TsDevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return TS_OK;
  if (b.p) {
    TS_HIP(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
  }
  // round up so slowly growing requests do not reallocate every time
  const size_t want = (bytes + 0xFFFFF) & ~(size_t)0xFFFFF;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) {
    b.p = nullptr;
    ts_set_error("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
    return TS_ERR_OOM;
  }
  b.bytes = want;
  return TS_OK;
}
static inline void ts_buf_release(TsDevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
}

// The caller's element type (TS_F32 / TS_F16 / TS_BF16) as a type: f(p) with p a pointer to it.
template <class F>
static inline int ts_typed(const void* p, int dtype, const char* bad_fmt, F&& f) {
  switch (dtype) {
    case TS_F32: return f((const float*)p);
    case TS_F16: return f((const _Float16*)p);
    case TS_BF16: return f((const __bf16*)p);
  }
  ts_set_error(bad_fmt, dtype);
  return TS_ERR_INVALID;
}
template <class F> static inline int ts_typed_rows(const void* rows, int dtype, F&& f) {
  return ts_typed(rows, dtype, "bad rows dtype %d", f);
}
template <class F> static inline int ts_typed_queries(const void* q, int dtype, F&& f) {
  return ts_typed(q, dtype, "bad query dtype %d", f);
}
// the element type of such a pointer
template <class P> struct TsPointee;
template <class T> struct TsPointee<const T*> { typedef T type; };

// ---------------------------------------------------------------- layout
//
// The corpus is NOT kept row-major.  It is stored in the order the MFMA A
// operand wants it, so that every wave-level load of the scan kernel is one
// fully contiguous 1 KiB read (64 lanes x 16 B):
//
//   row block  b = row / 32            (32 rows share one MFMA tile)
//   k group    g = 0 .. KG-1           (one 16-byte fragment per lane)
//   lane       l = h*32 + r,  r = row % 32,  h = 0/1
//
//   16-byte unit index = (b*KG + g)*64 + l
//
//   f16/bf16: the unit holds 8 elements, k = 16*g + 8*h + j   (j = 0..7)
//             -> exactly the A fragment of v_mfma_f32_32x32x16_{f16,bf16}
//   f32:      the unit holds 4 elements, k = 8*g + 2*t + h    (t = 0..3)
//             -> element t is the A operand of the t-th v_mfma_f32_32x32x2_f32
//   e4m3:     the unit holds 16 elements, k = 32*g + 16*m + 8*h + j   (m = 0/1, j = 0..7): bytes 0-7 and 8-15
//             are, once converted to bf16, the A fragments of k steps 2g and 2g+1 of the 16-bit map
//             (ts_scan_fp8.hip); its Q image is the bf16 image of the same padded dimension
//   mxfp4:    a row block is NS scale units, then NG code units (KG = NS + NG, NG = dpad / 64, NS = ceil(NG / 16)).
//             Code unit g holds 32 e2m1 nibbles, k = 64*g + 16*m + 8*h + j (m = 0..3, j = 0..7; nibble j of dword m):
//             dword m, once converted to bf16, is the A fragment of k step 4g + m of the 16-bit map.  Byte g % 16 of
//             the lane's unit in scale unit g / 16 is the E8M0 scale of those 32 elements (ts_scan_fp4.hip,
//             DESIGN.md 4.23); its Q image is the bf16 image of the same padded dimension
//
// The query batch is laid out the same way (the "Q image"): unit index
// (g*QH + hq)*64 + l holds, for query 32*hq + (l & 31), the same k's.
// dim is zero-padded to a multiple of TS_RING groups so the scan kernel's
// register ring never straddles a partial group.
#ifndef TS_RING
#define TS_RING 8          // k groups kept in flight per wave (1 KiB each)
#endif
#define TS_ROWS_PER_BLOCK 32
#define TS_MAX_Q 64        // queries per scan pass (2 MFMA column halves)

struct TsLayout {
  int dtype;   // ts_dtype of the stored corpus
  int esize;   // bytes per element
  int epl;     // elements per lane per group (8 or 4)
  int gk;      // k values covered by one group (16 or 8)
  int dim;     // logical dimension
  int dpad;    // padded dimension (multiple of gk*TS_RING: 128 for 16-bit storage, 256 for e4m3 and mxfp4)
  int kg;      // 1 KiB units per row block = dpad / gk (mxfp4: plus the scale units at its head)
  int qkg;     // 1 KiB units of the Q image per 32 queries: kg, or that of a bf16 image for e4m3 and mxfp4 storage
  int fp8_scale_log2;   // e4m3 storage: element x is stored as e4m3(x * 2^s) (ts_index_set_fp8_scale_log2)
};

// (A translation unit with a ring depth of its own, ts_scan_fp4.hip, defines TS_NO_LAYOUT_BUILDER: the padding below
// depends on TS_RING, so such a unit takes the layouts it is handed and cannot build one that disagrees.)
#ifndef TS_NO_LAYOUT_BUILDER
static inline TsLayout ts_make_layout(int dim, int dtype) {
  TsLayout L;
  L.dtype = dtype;
  L.esize = (dtype == TS_F32) ? 4 : (dtype == TS_FP8_E4M3 ? 1 : 2);
  L.epl = 16 / L.esize;
  L.gk = 2 * L.epl;
  L.dim = dim;
  int q = L.gk * TS_RING;
  L.dpad = ((dim + q - 1) / q) * q;
  L.kg = L.dpad / L.gk;
  L.qkg = (dtype == TS_FP8_E4M3) ? 2 * L.kg : L.kg;
  L.fp8_scale_log2 = 8;
  if (dtype == TS_MXFP4_E2M1) {
    // 64 elements per lane pair and code unit; a ring of four code units (ts_scan_fp4.hip), so dpad % 256 == 0 and
    // d = 768 keeps its 12 code units; the scale units at the head of the row block count as groups of it
    L.esize = 1;   // (unused: two elements per byte)
    L.epl = 32;
    L.gk = 64;
    L.dpad = ((dim + 255) / 256) * 256;
    const int ng = L.dpad / 64;
    L.kg = ng + (ng + 15) / 16;
    L.qkg = 4 * ng;
  }
  return L;
}
#endif

static inline size_t ts_block_bytes(const TsLayout& L) {
  return (size_t)L.kg * 1024;  // 32 rows * dpad * esize
}

// ---------------------------------------------------------------- scan
struct ScanParams {
  const uint4* corpus;   // tiled corpus
  const uint4* qimg;     // Q image (KG*QH KiB)
  int kg;
  int nq;                // valid queries in this pass
  int64_t nwork;         // row blocks to process
  int64_t blk0;          // block index of work item w = blk0 + w*blk_stride
  int64_t blk_stride;
  int64_t ntotal;        // valid rows in the index
  // dense mode: dense[q*dense_ld + w*32 + i]
  float* dense;
  int64_t dense_ld;
  // filter mode
  const float* tau;       // [64] per-query lower bound (score >= tau passes)
  uint32_t* cand_cnt;     // [64]
  float* cand_score;      // [64][cand_cap]
  int32_t* cand_id;       // [64][cand_cap] local row ids
  uint32_t cand_cap;
};

enum { SCAN_DENSE = 0, SCAN_FILTER = 1 };

// The masked filter scan of filtered searches (scan_kernel over WalkLive, ts_scan_dev.h; parameters of its own, so
// that ScanParams stays as it is): work item w is row block live[w], w < *nlive (nwork is
// then only the grid's upper bound), and a survivor of query q also needs bit (row % 32) of word
// allow_bits[qmask[q] * allow_words + row / 32]; qmask[q] < 0 allows every row.
struct MaskedScanParams : ScanParams {
  const int32_t* live;
  const uint32_t* nlive;
  const uint32_t* allow_bits;
  int64_t allow_words;
  const int32_t* qmask;   // [64]
};
int ts_launch_scan_masked(const TsLayout& L, int qh, const MaskedScanParams& p, int num_cus, hipStream_t stream);

// Prefix scans (ts_scan_prefix.hip): the first `kg` k groups of every row block, whose starts are
// `kg_row` groups apart; qimg is the image of a kg-group layout.  Parameters of their own, derived, so that the structs
// of the scans above keep their layout.  f16 / bf16 storage.
struct PrefixScanParams : ScanParams {
  int kg_row;
};
struct PrefixMaskedScanParams : MaskedScanParams {
  int kg_row;
};
int ts_launch_scan_prefix(const TsLayout& L, int mode, int qh, const PrefixScanParams& p, int num_cus, hipStream_t stream);
int ts_launch_scan_prefix_masked(const TsLayout& L, int qh, const PrefixMaskedScanParams& p, int num_cus,
                                 hipStream_t stream);

// Boosted scans (ts_scan_bias.hip): the masked filter scan on score + bias[row].  bias: ntotal floats,
// 16-byte aligned, of which the whole row blocks are read; the partial last block tail_blk (-1: ntotal is a multiple of
// 32) reads the 32 floats of bias_tail instead.  Parameters of their own, derived.  f16 / bf16 storage.
struct BiasScanParams : MaskedScanParams {
  const float* bias;
  const float* bias_tail;
  int64_t tail_blk;
};
int ts_launch_scan_biased(const TsLayout& L, int qh, const BiasScanParams& p, int num_cus, hipStream_t stream);

// Coalesced passes (TS_FLAG_COALESCE, scan_multi_kernel): one filter scan over every row block for G 32-query
// groups that may come from different batches.  Group g is the query columns 32*ghalf[g] .. +32 of the Q image
// gimg[g] (laid out with gqh[g] halves per k group), with its batch's thresholds and candidate lists at the same
// query offset: gtau[g][j], gcnt[g][j], gscore[g][j*cand_cap + slot], gid[g][j*cand_cap + slot] for query j of
// the group.  The base's qimg / nq / tau / cand_cnt / cand_score / cand_id are unused; blk0 / blk_stride /
// nwork / ntotal / cand_cap mean what they mean for scan_kernel.  stage_cap: LDS staging entries (8 B each).
#define TS_MAX_GROUPS 4
struct MultiScanParams : ScanParams {
  const uint4* gimg[TS_MAX_GROUPS];
  int gqh[TS_MAX_GROUPS];
  int ghalf[TS_MAX_GROUPS];
  const float* gtau[TS_MAX_GROUPS];
  uint32_t* gcnt[TS_MAX_GROUPS];
  float* gscore[TS_MAX_GROUPS];
  int32_t* gid[TS_MAX_GROUPS];
  uint32_t stage_cap;
};
// The largest group count (<= TS_MAX_GROUPS) whose query images and a minimal staging area fit the LDS; 0 for fp32
// storage (no multi-group kernel).  Host-only arithmetic.
int ts_scan_multi_groups(const TsLayout& L);
// staging entries the kernel gets for G groups (0: G groups do not fit)
uint32_t ts_scan_multi_stage_cap(const TsLayout& L, int G);
// false where a workgroup's survivor keys could not encode a wave's iteration count (the grid is too small for nblk)
bool ts_scan_multi_fits(int64_t nblk, int num_cus);
int ts_launch_scan_multi(const TsLayout& L, int G, const MultiScanParams& p, int num_cus, hipStream_t stream);

// Wide coalesced passes (scan_wide_kernel): the groups of MultiScanParams, up to TS_MAX_WIDE_GROUPS of them.  The
// query image is not kept resident: LDS holds a double-buffered window of TS_RING k groups for all G groups
// (2 * G * TS_RING KiB), gathered from the batches' images one window ahead, so G does not depend on the dimension.
#define TS_MAX_WIDE_GROUPS 8
struct WideScanParams : ScanParams {
  const uint4* gimg[TS_MAX_WIDE_GROUPS];
  int gqh[TS_MAX_WIDE_GROUPS];
  int ghalf[TS_MAX_WIDE_GROUPS];
  const float* gtau[TS_MAX_WIDE_GROUPS];
  uint32_t* gcnt[TS_MAX_WIDE_GROUPS];
  float* gscore[TS_MAX_WIDE_GROUPS];
  int32_t* gid[TS_MAX_WIDE_GROUPS];
  uint32_t stage_cap;
};
// groups per wide pass (0 for fp32 storage: no wide kernel); host-only arithmetic
int ts_scan_wide_groups(const TsLayout& L);
// staging entries the wide kernel gets for G groups (0: G is not a wide group count)
uint32_t ts_scan_wide_stage_cap(const TsLayout& L, int G);
// as ts_scan_multi_fits, for the wide kernel's survivor keys (one query bit more, one iteration bit less)
bool ts_scan_wide_fits(int64_t nblk, int num_cus);
int ts_launch_scan_wide(const TsLayout& L, int G, const WideScanParams& p, int num_cus, hipStream_t stream);

// Query-stationary coalesced passes (scan_qstat_kernel, ts_scan_qstat.hip): the groups of WideScanParams, up to 8, one
// per wave, each wave holding its group's image in registers while the corpus goes through an LDS ring shared by the
// workgroup.  Padded dimensions 640 and 768, f16 / bf16 storage; no tombstone form.
// groups per stationary pass (0: no kernel for the layout); host-only arithmetic
int ts_scan_qstat_groups(const TsLayout& L);
// staging entries the kernel gets (what the ring leaves of the LDS; 0: no kernel for the layout)
uint32_t ts_scan_qstat_stage_cap(const TsLayout& L);
// false where the survivor keys could not encode a workgroup's step count
bool ts_scan_qstat_fits(int64_t nblk, int num_cus);
// the kernel's LDS attribute on the current device, ahead of the first launch
int ts_scan_qstat_prepare(const TsLayout& L);
int ts_launch_scan_qstat(const TsLayout& L, int G, const WideScanParams& p, int num_cus, hipStream_t stream);
// Sample mode (scan_qstat_sample_kernel): the dense scan of one strided sample of the corpus for up to 8 groups of
// several batches at once, instead of one ts_launch_scan(SCAN_DENSE) per batch.  Group g is the query columns
// 32 * ghalf[g] .. of the image gimg[g] (gqh[g] halves per k group); its gnq[g] valid queries write what scan_kernel's
// dense mode writes for them, gdense[g][(32 * ghalf[g] + j) * dense_ld + w * 32 + i] for row i of work item w (row
// block blk0 + w * blk_stride).  Same chain of MFMAs per score, so the same bits.
struct QstatSampleParams {
  const uint4* corpus;
  int kg;
  int64_t nwork, blk0, blk_stride, ntotal;
  int64_t dense_ld;
  const uint4* gimg[TS_MAX_WIDE_GROUPS];
  int gqh[TS_MAX_WIDE_GROUPS];
  int ghalf[TS_MAX_WIDE_GROUPS];
  int gnq[TS_MAX_WIDE_GROUPS];
  float* gdense[TS_MAX_WIDE_GROUPS];
};
int ts_launch_scan_qstat_sample(const TsLayout& L, int G, const QstatSampleParams& p, int num_cus, hipStream_t stream);

// Tombstone passes: the coalesced passes of an index with removed rows.  live: its live words (bit
// r % 32 of word r / 32 = row r live); each wave reads its block's word as a scalar load and its survivor epilogue
// drops the rows whose bit is clear.  Derived structs, so that the existing instantiations keep their arguments.
struct MultiTombParams : MultiScanParams {
  const uint32_t* live;
};
struct WideTombParams : WideScanParams {
  const uint32_t* live;
};
int ts_launch_scan_multi_tomb(const TsLayout& L, int G, const MultiTombParams& p, int num_cus, hipStream_t stream);
int ts_launch_scan_wide_tomb(const TsLayout& L, int G, const WideTombParams& p, int num_cus, hipStream_t stream);

int ts_launch_scan(const TsLayout& L, int mode, int qh, const ScanParams& p,
                   int num_cus, hipStream_t stream);

// ---------------------------------------------------------------- filtered search (masks)
// One pass of a filtered search: the distinct masks its queries use and each query's mask.
struct TsMaskPass {
  int32_t nd;              // distinct masks of the pass
  int32_t all_live;        // a query of the pass has no mask: every row block is live
  int32_t dist[TS_MAX_Q];  // mask index of distinct mask d
  int32_t qmask[TS_MAX_Q]; // mask index of query q (-1: no mask, also for q >= nq)
  int32_t qd[TS_MAX_Q];    // distinct-mask slot of query q (-1: no mask)
};
// Device tables of a filtered pass (ts_index.hip keeps one per workspace set).
struct TsMaskDev {
  int32_t qmask[TS_MAX_Q];
  int32_t qd[TS_MAX_Q];
  uint32_t popc[TS_MAX_Q];   // allowed rows (< ntotal) of distinct mask d
  uint32_t need[TS_MAX_Q];   // min(k, allowed rows) of query q: the exactness check (need_check_kernel)
  uint32_t nlive;            // live row blocks
  uint32_t pad[63];
  // followed by int32_t live[nblk]
};
// live[] = row blocks whose OR over the pass's masks is non-zero (every block if mp.all_live), *nlive their
// number, popc[d] = allowed rows of each distinct mask; also writes qmask[] / qd[].  nlive and popc must be
// zero on entry.
int ts_launch_live_blocks(const uint32_t* bits, int64_t words, const TsMaskPass& mp, int64_t nblk,
                          int64_t ntotal, TsMaskDev* md, hipStream_t stream);
// Thresholds of a filtered pass from the (unfiltered, strided) sample: per query the m_q-th best ALLOWED
// sample score, m_q = max(min_rank, ceil(over * k * S_q / N_q)), or -FLT_MAX when S_q < m_q; need[q] =
// min(k, N_q); +FLT_MAX for nq <= q < 64.  Block 0 copies *nlive to *report when report is non-null.
int ts_launch_tau_masked(const float* sample, int64_t S, int64_t sstride, int64_t ntotal, const uint32_t* bits,
                         int64_t words, TsMaskDev* md, int nq, int k, uint32_t over, uint32_t min_rank,
                         float* tau, uint32_t* report, hipStream_t stream);
// Boosted passes (ts_scan_bias.hip): ts_launch_tau_masked on sample score + bias[row]; and the dense path's chunk,
// dense[q][i] += bias[row0 + i] with the ids of ts_launch_mask_ids (-1 also where the sum is NaN)
int ts_launch_tau_biased(const float* sample, int64_t S, int64_t sstride, int64_t ntotal, const uint32_t* bits,
                         int64_t words, const float* bias, TsMaskDev* md, int nq, int k, uint32_t over,
                         uint32_t min_rank, float* tau, uint32_t* report, hipStream_t stream);
int ts_launch_bias_ids(const uint32_t* bits, int64_t words, const TsMaskPass& mp, const float* bias, int nq,
                       int64_t row0, uint32_t rows, int64_t ld, float* dense, int32_t* ids, hipStream_t stream);
// LDS bytes the scan kernel needs for qh*32 queries (Q image + candidate staging)
size_t ts_scan_lds_bytes(const TsLayout& L, int qh);
// queries per pass: 64 where the image of 64 fits the LDS, else 32
static inline int ts_queries_per_pass(const TsLayout& L) { return ts_scan_lds_bytes(L, 2) <= TS_LDS_BYTES ? 64 : 32; }
// fp32 storage, 32-query passes, 512 < d <= 768: the bf16x3 split scan (ts_scan_f32s.hip) instead of the exact-f32 MFMA
bool ts_use_f32_split(const TsLayout& L, int qh);
size_t ts_scan_f32s_lds_bytes(const TsLayout& L);
int ts_launch_scan_f32s(const TsLayout& L, int mode, const ScanParams& p, int num_cus, hipStream_t stream);
int ts_launch_qprep_f32s(const TsLayout& L, const void* q, int q_dtype, int nq, uint4* qimg, uint32_t* cand_cnt,
                         uint32_t* status, hipStream_t stream);
// e4m3 storage (ts_scan_fp8.hip): the scans, the Q image (the queries rounded to bf16, times
// 2^-fp8_scale_log2), the quantising relayout and the decoding reconstruct.  ts_launch_scan / _scan_masked / _qprep /
// _relayout / _reconstruct hand an e4m3 layout to these.
size_t ts_scan_fp8_lds_bytes(const TsLayout& L, int qh);
int ts_launch_scan_fp8(const TsLayout& L, int mode, int qh, const ScanParams& p, int num_cus, hipStream_t stream);
int ts_launch_scan_masked_fp8(const TsLayout& L, int qh, const MaskedScanParams& p, int num_cus, hipStream_t stream);
int ts_launch_qprep_fp8(const TsLayout& L, const void* q, int q_dtype, int nq, int qh, uint4* qimg, uint32_t* cand_cnt,
                        uint32_t* status, hipStream_t stream);
int ts_launch_relayout_fp8(const TsLayout& L, const void* rows, int in_dtype, int64_t n, int64_t row0, uint4* tiled,
                           bool normalize, float* den_scratch, hipStream_t stream);
// den[i] = |row_i| + 1e-8 (ts_scan.hip: the kernel every normalising relayout uses)
int ts_launch_row_den(const void* rows, int in_dtype, int64_t n, int dim, float* den, hipStream_t stream);
int ts_launch_reconstruct_fp8(const TsLayout& L, const uint4* tiled, int64_t row0, int64_t n, float* out,
                              hipStream_t stream);
// 4-bit MX storage (ts_scan_fp4.hip): the same set for TS_MXFP4_E2M1, whose Q image is the plain bf16
// image.  ts_launch_update_rows hands its layout to ts_launch_update_rows_fp4 (a row block of it is not a multiple of
// TS_RING units).
static inline int ts_fp4_code_groups(const TsLayout& L) { return L.dpad / 64; }
static inline int ts_fp4_scale_units(const TsLayout& L) { return L.kg - L.dpad / 64; }
size_t ts_scan_fp4_lds_bytes(const TsLayout& L, int qh);
int ts_launch_scan_fp4(const TsLayout& L, int mode, int qh, const ScanParams& p, int num_cus, hipStream_t stream);
int ts_launch_scan_masked_fp4(const TsLayout& L, int qh, const MaskedScanParams& p, int num_cus, hipStream_t stream);
int ts_launch_qprep_fp4(const TsLayout& L, const void* q, int q_dtype, int nq, int qh, uint4* qimg, uint32_t* cand_cnt,
                        uint32_t* status, hipStream_t stream);
int ts_launch_relayout_fp4(const TsLayout& L, const void* rows, int in_dtype, int64_t n, int64_t row0, uint4* tiled,
                           bool normalize, float* den_scratch, hipStream_t stream);
int ts_launch_reconstruct_fp4(const TsLayout& L, const uint4* tiled, int64_t row0, int64_t n, float* out,
                              hipStream_t stream);
int ts_launch_update_rows_fp4(const TsLayout& L, const uint4* stage, uint4* corpus, const int32_t* blk,
                              const int32_t* first, const int32_t* item, int64_t n_entries, hipStream_t stream);

// rows [n, dim] (row-major, in_dtype) -> tiled storage at rows [row0, row0+n)
int ts_launch_relayout(const TsLayout& L, const void* rows, int in_dtype,
                       int64_t n, int64_t row0, uint4* tiled, bool normalize,
                       float* den_scratch, hipStream_t stream);
// tiled -> row-major float32
int ts_launch_reconstruct(const TsLayout& L, const uint4* tiled, int64_t row0,
                          int64_t n, float* out, hipStream_t stream);
// queries [nq, dim] (q_dtype) -> Q image in the storage dtype; also clears
// cand_cnt[64] and status[0] when they are non-null
int ts_launch_qprep(const TsLayout& L, const void* q, int q_dtype, int nq,
                    int qh, uint4* qimg, uint32_t* cand_cnt, uint32_t* status,
                    hipStream_t stream);

// ---------------------------------------------------------------- one-launch search (ts_fused.hip)
// query preparation + threshold estimation + fused scan/filter in one kernel; see ts_fused.hip
struct TsFusedArgs {
  const uint4* corpus;
  const void* queries;      // [nq, dim] rows of q_dtype (device)
  int q_dtype;
  int nq;
  int64_t nblk, ntotal;
  int scan_wgs, tau_wgs;    // workgroups streaming the corpus / estimating the thresholds
  int64_t n_sample;         // row blocks that feed the threshold sample: sample item s is block s*sample_stride
  int64_t sample_stride;    // sample item s is row block s*sample_stride
  uint32_t m;               // wanted rank among the sample's 16-row group maxima
  uint32_t expect;          // sample slots per query (two per sample block; a multiple of 4, <= TS_FUSED_MAX_KEYS)
  uint32_t gen;             // generation tag of the launch (non-zero, unique per workspace set)
  uint32_t arrive_goal;     // value of *arrive once every sample wave has reported
  uint32_t wait_iters;      // bound of every in-kernel spin
  uint32_t* skeys;          // ts_fused_keys_bytes(): [64][TS_FUSED_MAX_KEYS] sample keys, all-zero between launches
  uint32_t* arrive;
  unsigned long long* tau64;   // [64]
  uint32_t* cand_cnt;       // [64], zero at launch
  float* cand_score;
  int32_t* cand_id;
  uint32_t cand_cap;
};
#define TS_FUSED_MAX_KEYS 12288   // per query; the threshold role selects among two queries' keys in LDS (96 KiB)
size_t ts_fused_keys_bytes();
int ts_launch_fused(const TsLayout& L, int qh, const TsFusedArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- select
enum { SEL_DENSE = 0, SEL_PAIRS32 = 1, SEL_MERGE64 = 2 };

#define TS_SEL_LDS_KEYS 16384   // 64-bit keys held in LDS by the select kernel
#define TS_STATUS_OVERFLOW 1u
#define TS_STATUS_SHORT 2u

struct SelParams {
  int mode;
  const float* scores;     // [nq][stride]
  const int32_t* ids32;    // PAIRS32: [nq][stride]
  const int64_t* ids64;    // MERGE64: [nq][stride] (entries with id<0 ignored)
  int64_t stride;          // elements between consecutive queries
  uint32_t seg_len;        // 0, or length of each concatenated list
  int64_t seg_stride;      // distance between consecutive lists of a query (scores)
  int64_t seg_stride_ids;  // same for the int64 ids (MERGE64; 0 = same as seg_stride)
  uint32_t n;              // entries per query (if n_per_q == null)
  const uint32_t* n_per_q; // optional device counts, clamped to n_cap
  uint32_t n_cap;
  int32_t id_base;         // DENSE: id = index + id_base
  int k;                   // entries to output per query
  uint32_t need;           // status SHORT if available < need (0 = no check)
  float* out_scores;       // [nq][out_stride]
  int64_t* out_ids64;      // final output (id + id_offset), or null
  int32_t* out_ids32;      // intermediate output (local ids), or null
  int64_t out_stride;
  int64_t id_offset;
  uint32_t* status;        // optional device status word (TS_STATUS_* bits are OR-ed in)
  uint32_t* host_report;   // optional, device view of pinned host memory:
                           // [q] = candidate count of query q, [64] |= status bits
  uint32_t* clear_counts;  // optional: n_per_q is given back as zeros (the one-launch search has no
                           // preparation kernel that would clear it)
};
// filtered searches: the dense path's per-chunk ids (row, or -1 outside the query's mask) for SEL_PAIRS32 over
// the dense scores, and the exactness check of a masked pass (TS_STATUS_SHORT if cand_cnt[q] < need[q])
int ts_launch_mask_ids(const uint32_t* bits, int64_t words, const TsMaskPass& mp, int nq, int64_t row0,
                       uint32_t rows, int64_t ld, int32_t* ids, hipStream_t stream);
int ts_launch_need_check(const uint32_t* cand_cnt, const uint32_t* need, int nq, uint32_t* status,
                         uint32_t* host_report, hipStream_t stream);

int ts_launch_select(const SelParams& p, int nq, hipStream_t stream);

// tau[q] = (approximately) the m-th largest of sample[q][0..n) for q < nq,
// +FLT_MAX for nq <= q < 64
int ts_launch_tau(const float* sample, int64_t ld, uint32_t n, uint32_t m,
                  int nq, float* tau, hipStream_t stream);

// Thresholds and selects of a coalesced pass in one launch each ("pass prologue"): entry b is what
// batch b's own ts_launch_tau / ts_launch_select call would take, and gets exactly that call's results.
#define TS_PASS_BATCHES 8   // batches with a group in one pass of 8 groups
struct TauBatch {
  const float* sample[TS_PASS_BATCHES];
  int64_t ld[TS_PASS_BATCHES];
  uint32_t n[TS_PASS_BATCHES];
  uint32_t m[TS_PASS_BATCHES];
  int nq[TS_PASS_BATCHES];
  float* tau[TS_PASS_BATCHES];
};
// batches share a launch where this agrees (the kernel ts_launch_tau picks for m)
int ts_tau_batch_key(uint32_t m);
int ts_launch_tau_batch(const TauBatch& t, int nb, hipStream_t stream);
struct SelBatch {
  SelParams p[TS_PASS_BATCHES];   // SEL_PAIRS32
  int nq[TS_PASS_BATCHES];
};
// batches share a launch where this agrees (the LDS keys ts_launch_select gives the batch)
int ts_select_batch_key(const SelParams& p, uint32_t* lds_keys);
int ts_launch_select_batch(const SelBatch& t, int nb, hipStream_t stream);

// ---------------------------------------------------------------- range search (ts_range.hip)
// Results in CSR form: query q of the pass owns out[off[q] .. off[q + 1]) of the call's result buffers (`capacity`
// entries), rows in ascending id order.  off[] comes from counts the host has read before the launch.
#define TS_RANGE_TILE 1024   // rows per tile of the dense path
// Small path: the filter scan's lists (cand_cap entries per query, cnt[q] <= cand_cap of them valid) sorted by id.
struct TsRangeSortParams {
  const float* cand_score;
  const int32_t* cand_id;
  uint32_t cand_cap;
  uint32_t cnt[TS_MAX_Q];
  int64_t off[TS_MAX_Q + 1];
  float* out_scores;
  int64_t* out_ids;
  int64_t capacity;
  int64_t id_offset;
};
int ts_launch_range_sort(const TsRangeSortParams& p, int nq, uint32_t max_count, hipStream_t stream);
// Dense path, one chunk of dense scores: dense[q * ld + i] is the score of row row0 + i, i < rows; mids (may be null)
// holds >= 0 where the row is allowed for the query (ts_launch_mask_ids).  The chunk's tiles are tile0 .. tile0 +
// chunk_tiles of the pass's ntiles; tilecnt[q * ntiles + t]: the count kernel writes the survivors of tile t, the
// prefix kernel turns a query's line into its exclusive prefix (total[q] = the sum), the fill kernel reads that.
struct TsRangeDenseParams {
  const float* dense;
  const int32_t* mids;
  int64_t ld;
  int64_t row0;
  uint32_t rows;
  uint32_t chunk_tiles;
  int64_t tile0;
  int64_t ntiles;
  uint32_t* tilecnt;
  float radius[TS_MAX_Q];
  // fill only
  int64_t off[TS_MAX_Q + 1];
  float* out_scores;
  int64_t* out_ids;
  int64_t capacity;
  int64_t id_offset;
};
int ts_launch_range_count(const TsRangeDenseParams& p, int nq, hipStream_t stream);
int ts_launch_range_prefix(uint32_t* tilecnt, int64_t ntiles, int nq, uint32_t* total, hipStream_t stream);
int ts_launch_range_fill(const TsRangeDenseParams& p, int nq, hipStream_t stream);

// ---------------------------------------------------------------- maxsim
int ts_launch_maxsim(const void* q, int Lq, const void* docs,
                     const int32_t* doc_off, const int64_t* starts, const int32_t* lens,
                     int n_docs, int H, int dtype, int mode, float* out, hipStream_t stream);
// HBM-bound streaming form for f16/bf16/f32 token matrices and e4m3 token stores (ts_maxsim16.hip).  Returns
// TS_ERR_UNSUPPORTED without an error string for shapes it does not take.  dtype is the store's element type;
// q_dtype the query's (< 0: the store's; an e4m3 store takes a TS_F16 / TS_BF16 query).
int ts_launch_maxsim16(const void* q, int Lq, const void* docs, const int32_t* doc_off,
                       const int64_t* starts, const int32_t* lens, int n_docs, int H, int dtype,
                       int mode, float* out, int device, hipStream_t stream, int q_dtype = -1);
int ts_launch_maxsim16_batch(const void* q, const int32_t* q_off, int nq, const void* store,
                             const int64_t* starts, const int32_t* lens, const int32_t* cand_off,
                             int H, int dtype, int mode, float* out, int device, hipStream_t stream,
                             int q_dtype = -1);
// rows x H elements of x (x_dtype TS_F32 / TS_F16 / TS_BF16, H % 16 == 0, 16-byte aligned) -> the e4m3 token-store
// rows of include/tristage.h (ts_fp8.hip)
int ts_launch_quantize_rows_fp8(const void* x, int x_dtype, int64_t rows, int H, void* out, hipStream_t stream);

// ---------------------------------------------------------------- removal (ts_remove.hip)
// Tombstone bitmap of a flat index: bit r % 32 of word r / 32 set = row r live (the filtered-search layout).
// sets the bits of rows [row0, row1) (the other bits of the words they share are kept)
int ts_launch_live_set(uint32_t* live, int64_t row0, int64_t row1, hipStream_t stream);
// clears the bits of ids - id_offset in [0, ntotal) and adds to *cleared how many bits went from set to clear
int ts_launch_live_clear(uint32_t* live, const int64_t* ids, int64_t n, int64_t id_offset, int64_t ntotal,
                         unsigned long long* cleared, hipStream_t stream);
// out [n_masks + 1][words]: mask m ANDed with live (bits has bit_words words per mask), then live itself
int ts_launch_and_live(const uint32_t* bits, int64_t bit_words, int n_masks, const uint32_t* live, int64_t words,
                       uint32_t* out, hipStream_t stream);
// Moves the live rows of the tiled corpus down in place (order kept), zeroes what lies behind them up to the old
// last block, and writes old2new_dev[ntotal] (-1 = removed) when it is non-null.  scratch: at least
// ts_compact_scratch_bytes(ntotal); stage: the staging buffer of the ascending chunks (whole row blocks).
int ts_compact_corpus(const TsLayout& L, uint4* corpus, const uint32_t* live, int64_t ntotal, void* scratch,
                      size_t scratch_bytes, uint4* stage, size_t stage_bytes, int64_t* old2new_dev, int64_t* nlive_out,
                      hipStream_t stream);
size_t ts_compact_scratch_bytes(int64_t ntotal);

// ---------------------------------------------------------------- update in place (ts_update.hip)
// rows[i] = ids[i] - id_offset (HOST arrays); TS_ERR_INVALID and a message naming the first id of the call that lies
// outside [0, ntotal) or repeats an earlier one.  keys: rows[i] << 32 | i, ordered by row (ts_update_sort_rows); left
// empty when the rows are strictly ascending as given (a bulk update need not pay for them).
int ts_update_check_ids(const int64_t* ids, int64_t n, int64_t id_offset, int64_t ntotal, int64_t* rows,
                        std::vector<uint64_t>* keys);
// keys[i] = rows[i] << 32 | i ordered by row, positions of equal rows ascending (rows < 2^31, n < 2^31)
void ts_update_sort_rows(const int64_t* rows, int64_t n, std::vector<uint64_t>* keys);
// The row blocks a staging chunk touches: staging row j replaces row r for each key r << 32 | j of the chunk's n keys
// (ordered by row, rows distinct; HOST).
// A block all 32 of whose rows are replaced: full_blk[e], full_src[e * 32 + r] = staging row of its row r.  Any other
// block: part_blk[e] with the items part_first[e] .. part_first[e + 1) of part_item, item = staging row * 32 + r.
struct TsUpdateTables {
  std::vector<int32_t> full_blk, full_src, part_blk, part_first, part_item;
};
void ts_update_group_blocks(const uint64_t* keys, int64_t n, TsUpdateTables* t);
// out[0] += ids whose row is not live, out[1] = min(out[1], position of such an id); rows: DEVICE, after the offset
int ts_launch_update_live_check(const uint32_t* live, const int64_t* rows, int64_t n, unsigned long long* out,
                                hipStream_t stream);
// moves the staging tile's rows to their places (DEVICE tables of ts_update_group_blocks): whole unit rows of the
// fully replaced blocks / the 16-byte pieces of the replaced rows of the other blocks
int ts_launch_update_blocks(const TsLayout& L, const uint4* stage, uint4* corpus, const int32_t* blk,
                            const int32_t* src, int64_t n_entries, hipStream_t stream);
int ts_launch_update_rows(const TsLayout& L, const uint4* stage, uint4* corpus, const int32_t* blk,
                          const int32_t* first, const int32_t* item, int64_t n_entries, hipStream_t stream);
int ts_launch_update_ivf_check(const int64_t* rows, int64_t n, const int64_t* id2slot, const int64_t* slot2id,
                               const uint32_t* blk_valid, unsigned long long* out, hipStream_t stream);
int ts_launch_update_ivf_place(const TsLayout& L, const uint4* src, uint4* corpus, const int64_t* dst,
                               const int64_t* ids, int64_t n, int64_t* slot2id, int64_t* id2slot, uint32_t* blk_valid,
                               hipStream_t stream);

// ---------------------------------------------------------------- IVF compaction (ts_ivf_compact.hip)
// lists[id] (DEVICE int32[ntotal]) = the list of id's row, or -1 when the id was removed
int ts_launch_ivf_compact_classify(const int64_t* id2slot, const int64_t* slot2id, const int32_t* blk_list,
                                   int64_t ntotal, int32_t* lists, hipStream_t stream);
// Writes the new index beside the old one: new id j is old id new2old[j] and takes slot dst[j] (DEVICE int32[nlive],
// the host's placement).  new_corpus (new_blocks row blocks, every byte written: padding slots are zero rows),
// new_slot2id[32 * new_blocks] (-1 = padding), new_id2slot[nlive], new_valid[new_blocks]; src_slot: workspace,
// int32[32 * new_blocks].
int ts_launch_ivf_compact_move(const TsLayout& L, const uint4* old_corpus, const int64_t* old_id2slot,
                               const int32_t* new2old, const int32_t* dst, int64_t nlive, int64_t new_blocks,
                               uint4* new_corpus, int32_t* src_slot, int64_t* new_slot2id, int64_t* new_id2slot,
                               uint32_t* new_valid, hipStream_t stream);

// ---------------------------------------------------------------- MMR (ts_mmr.hip)
// Per-handle state of ts_index_mmr / ts_mmr_ivf: nothing is allocated before the first call; ts_mmr_release frees it
// with the handle.  scratch: candidate tiles, Gram matrices and validity words of one chunk of queries (at most
// 384 MiB, whatever the batch); stage: the staging of host-pointer calls; ev orders a call behind the previous one.
struct TsMmrWork {
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  void* stage = nullptr;
  size_t stage_bytes = 0;
  hipEvent_t ev = nullptr;
  bool used = false;
  // ts_index_mmr_set_timing: timed events around the three kernels of every chunk; such a call synchronises
  bool timing = false;
  hipEvent_t tev[4] = {};
  double phase_ms[3] = {0.0, 0.0, 0.0};   // gather, gram, greedy
  int64_t timed_calls = 0;
};
// where the candidates' rows live: a flat index (live: its tombstone words, or null while nothing is removed) or an
// IVF index (ivf: ids go through id2slot, a slot is live while its bit of blk_valid is set)
struct TsMmrSource {
  bool ivf;
  const uint4* corpus;
  TsLayout L;
  int64_t ntotal, id_offset;
  const uint32_t* live;
  const int64_t* id2slot;
  const uint32_t* blk_valid;
};
// argument checks of both entry points, before any HIP call
int ts_mmr_check_args(const void* h, const void* cand_ids, const void* cand_rel, int32_t nq, int32_t fetch_k,
                      int32_t k, float lambda, const void* out_rel, const void* out_ids);
int ts_mmr_run(const TsMmrSource& src, TsMmrWork& w, const int64_t* cand_ids, const float* cand_rel, int32_t nq,
               int32_t C, int32_t k, float lambda, float* out_rel, int64_t* out_ids, uint32_t flags, hipStream_t s);
void ts_mmr_release(TsMmrWork& w);
// MMR's gather on its own: candidates ids[q * C + c] (-1, unknown and removed ids: zero rows, valid = 0) of nq queries
// -> tile[q][cbp][kg][64] in fragment order and valid[q][32 * cbp]; cbp >= ceil(C / 32)
int ts_launch_gather_tiles(const TsMmrSource& src, const int64_t* ids, int C, int cbp, int nq, uint4* tile,
                           int32_t* valid, hipStream_t s);

// ---------------------------------------------------------------- rescore (ts_rescore.hip)
// Exact scores of gathered candidates: query q of the chunk is column col0 + q of the pass's query image (qh halves per
// k group); scores[q * C + c] = its inner product with candidate c over all kg groups in ascending order (the scan's
// numbers), ids_out[q * C + c] = ids[q * C + c]; an invalid candidate gets -FLT_MAX and -1.  f16 / bf16 storage.
struct TsRescoreParams {
  const uint4* tile;       // [nq][cbp][kg][64]
  const int32_t* valid;    // [nq][32 * cbp]
  const int64_t* ids;      // [nq][C]
  const uint4* qimg;
  int kg, qh, C, cbp, col0;
  float* scores;           // [nq][C]
  int64_t* ids_out;        // [nq][C]
};
int ts_launch_rescore(const TsLayout& L, const TsRescoreParams& p, int nq, hipStream_t stream);
