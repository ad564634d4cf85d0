// libtristage.so — index handle, search orchestration and the C ABI
// (include/tristage.h).  The handle plays the role of the FAISS index object
// the reference keeps in Stage1Retriever.faiss_index
// (reference src/stage1_retriever.py:126, 256-283, 313, 380).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "ts_common.h"

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

void ts_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* ts_last_error(void) { return g_err; }
extern "C" int ts_abi_version(void) { return TS_ABI_VERSION; }

#define TS_NPHASE 8
#define TS_NSETS 8         // workspace sets = synchronous searches that may run at once on one handle; also the
                           // coalesced queue's held batches (at most TS_MAX_WIDE_GROUPS - 1) plus the one it acquires
#define TS_ASYNC_SLOTS 1024   // report slots; at most a quarter of them (256 passes) may belong to unfinished asynchronous searches
#define TS_SLOT_WORDS 80   // 64 counts + status word, padded
namespace {
// tuning constants of the filter path (DESIGN.md "threshold sampling")
constexpr int64_t kMinFilterRows = 32768;   // below this the dense path is used
constexpr int kMaxFilterK = 2048;
constexpr uint32_t kCandCap = 16384;        // candidate slots per query
constexpr int64_t kMinSampleRows = 8192;
constexpr int64_t kSampleDiv = 128;         // sample >= N/128 rows
constexpr uint32_t kMinSampleRank = 24;
constexpr uint32_t kOversample = 4;         // expected candidates ~ 4k per query
constexpr int64_t kDenseChunkRows = 1 << 20;
constexpr int64_t kOneLaunchMaxRows = 4 << 20;   // default use of the one-launch search (search_pass_on)
constexpr int kHeadStartUs = 12;           // pipelined mode: delay of the select behind the next scan (search_pass)
// coalesced passes (co_submit): expected survivors ~ 3k per query instead of 4k, so that three groups' survivors
// fit the staging area the query images leave at d = 768 (about 1.3 k per workgroup and pass against 1.9 k slots)
constexpr int64_t kCoalesceOversample = 3;
// wide coalesced passes (scan_wide_kernel) by default only where the corpus is larger than the 256 MiB Infinity Cache
// (only there does a pass saved save HBM bytes) and the LDS-resident passes take at most 3 groups: a wide pass of 6
// costs 0.62 ms per group at 10 M x 768, a resident pass of 3 0.74, and one of 4 (padded d <= 512) runs at the read
// ceiling too
constexpr int64_t kWideMinCorpusBytes = 256ll << 20;
constexpr int kWideMaxResidentGroups = 3;
// query-stationary passes (scan_qstat_kernel) wherever the policy above picks a wide pass and their kernel exists
// (DESIGN.md 4.2c has the measurement that decides this)
constexpr bool kStationaryByDefault = true;

}  // namespace

struct ts_index {
  int device = 0;
  int num_cus = 256;
  TsLayout L{};
  int64_t ntotal = 0;
  int64_t cap_blocks = 0;
  uint4* corpus = nullptr;
  int64_t id_offset = 0;
  int64_t info[4] = {0, 0, 0, 0};
  // the last filtered search (ts_index_last_filter_info): live row blocks read, row blocks, masked passes,
  // passes on the dense path; fseq numbers filtered calls, so that ts_index_finish adds the live counts of
  // the last one only
  int64_t finfo[4] = {0, 0, 0, 0};
  int64_t fseq = 0;
  // Per-search workspace, double-buffered so that consecutive pipelined searches never
  // share a buffer that is still being read (see search_pass).
  struct WSet {
    TsDevBuf qimg, small, cand_score, cand_id, sample;
    TsDevBuf dense, list_score, list_id;   // the dense path's score chunk and per-chunk lists
    TsDevBuf hist, spill;                  // one-launch search (ts_fused.hip): threshold histogram, parked score tiles
    TsDevBuf mask, mids;                   // filtered searches: TsMaskDev + live-block list; the dense path's masked ids
    uint32_t gen = 0;                    // generation tag of the last one-launch search on this set
    uint32_t arrive_total = 0;           // running goal of the set's arrival hint counter
    bool hist_dirty = false;             // a launch may have left entries behind: cleared before the next one
    unsigned long long* tau64() { return (unsigned long long*)((char*)small.p + 1024); }
    uint32_t* arrive() { return (uint32_t*)((char*)small.p + 2048); }
    hipEvent_t ev_pro = nullptr, ev_scan = nullptr, ev_sel = nullptr, ev_in = nullptr;  // timing disabled
    bool used = false;  // ev_sel has been recorded at least once
    bool busy = false;  // held by a search that is being enqueued / a synchronous search in flight (h->mu)
    float* tau() { return (float*)small.p; }
    uint32_t* cand_cnt() { return (uint32_t*)small.p + 64; }
    uint32_t* status() { return (uint32_t*)small.p + 128; }
    TsMaskDev* mask_dev() { return (TsMaskDev*)mask.p; }   // a masked pass's tables, its live-block list behind them
  };
  WSet ws[TS_NSETS];
  uint64_t set_next = 0;
  // Concurrency (include/tristage.h "threading"): searches from several host threads on ONE
  // handle are safe.  `mu` guards the set pool, the slot ring, the pending list, tickets and
  // `info`; a search owns its WSet from acquire_set() to release_set() — a synchronous one until
  // its result is verified (its exact fallback re-reads the set's query image), an asynchronous
  // one only while it is being enqueued (later users are ordered behind it by ev_sel).
  std::mutex mu;
  std::condition_variable cv;
  std::mutex host_mu;   // host-pointer searches share one staging area: serialised
  std::mutex prof_mu;   // per-phase timing uses one set of events: profiled searches are serialised
  bool slot_busy[TS_ASYNC_SLOTS] = {};
  hipStream_t s_pro = nullptr, s_scan = nullptr, s_sel = nullptr;  // TS_FLAG_PIPELINE only
  // staging of host-pointer calls (add / reconstruct need exclusive access anyway; searches: host_mu)
  TsDevBuf stage, den, qstage, out_s, out_i, mstage;
  uint32_t* host_status = nullptr;  // pinned + mapped: written by the select kernel
  uint32_t* host_status_dev = nullptr;  // device view of host_status
  // asynchronous searches (TS_FLAG_ASYNC): each pass reports into its own slot of
  // the mapped host ring; ts_index_finish() syncs once and inspects them all
  struct Pending { int64_t ticket; int slot; int nq; uint32_t S; uint32_t m; hipEvent_t e0, e1; int set; int64_t fseq; };
  Pending pending[TS_ASYNC_SLOTS];
  int npending = 0;
  uint64_t slot_next = 0;
  int64_t next_ticket = 0;
  hipEvent_t async_ev[2 * TS_ASYNC_SLOTS] = {};
  // coalesced passes (TS_FLAG_COALESCE): batches whose query prep, sample scan and thresholds are
  // enqueued but whose filter scan and select wait for co_width 32-query groups to share one scan.  A held batch
  // keeps its workspace set busy until its select is enqueued.  co_mu serialises coalesced submissions and
  // flushes; it is taken before `mu`, never while `mu` is held.
  // With the queue's pass prologue (co_prologue) a batch's sample scan and thresholds are not enqueued at submission
  // but in front of the first pass that holds one of its groups (co_pass_prologue): m, S, sstride, nsb are what those
  // launches take, tau_done marks a batch that has them, failed one whose deferred launches could not be enqueued.
  struct CoBatch {
    WSet* W; int nq, qh, k, slot, groups_left; float* out_s; int64_t* out_i;
    uint32_t m; int64_t S, sstride, nsb; bool tau_done, failed;
  };
  struct CoGroup { int batch, half; };
  std::mutex co_mu;
  int co_gmax = 0;                       // groups per LDS-resident pass (ts_coalesce_groups)
  int co_gwide = 0;                      // groups per wide pass (ts_coalesce_groups_wide)
  int co_gstat = 0;                      // groups per query-stationary pass (ts_coalesce_groups_stationary)
  int co_width = 0;                      // groups per pass of the queue's pending groups (co_pass_width)
  bool co_stat_forced = false;           // the queue's last search set TS_FLAG_STATIONARY_PASSES (co_launch_pass)
  bool co_prologue = false;              // the queue's batches get their sample scores and thresholds with their pass,
                                         // and a pass's thresholds / selects share a launch (co_pass_prologue)
  hipStream_t co_stream = nullptr;       // the stream of the held batches
  CoBatch co_batch[TS_MAX_WIDE_GROUPS] = {};  // held batches in submission order
  int co_nbatch = 0;
  CoGroup co_group[TS_MAX_WIDE_GROUPS] = {};  // pending groups of the next pass
  int co_ngroup = 0;
  uint64_t co_pass_seq = 0;              // timed passes: every prof_every-th
  hipEvent_t co_ev = nullptr;            // recorded on co_stream after every pass and its selects (co_launch_pass)
  bool co_ev_live = false;               // co_ev may still be pending: work on another stream must wait for it
  // optional per-phase timing with HIP events on the caller's stream
  // `profiling` / `prof_every` change only under exclusive access (ts_index_set_profiling); a profiled search holds
  // prof_mu for its whole duration, which is what makes the ONE set of events `ev` safe; everything that varies
  // per search lives in the search's own ProfCtx, and the accumulators are updated under `mu`.
  bool profiling = false;
  int prof_every = 1;        // time every prof_every-th search (timing events cost ~5 us each in-stream)
  std::atomic<uint64_t> prof_seq{0};
  hipEvent_t ev[TS_NPHASE + 1] = {};
  double phase_ms[TS_NPHASE] = {};
  int64_t phase_cnt[TS_NPHASE] = {};
  // tombstones (ts_index_remove): bit r % 32 of word r / 32 of `live` set = row r live.  The bitmap
  // is written at the first removal; while nremoved == 0 no search reads it and every path is the one without it.
  TsDevBuf live;
  int64_t live_cap_words = 0;
  int64_t nremoved = 0;
  // a search of an index with removed rows is a filtered one: its masks ANDed with `live` go to `eff`, one call at a
  // time (eff_mu); eff_ev, recorded behind the call's passes, orders the next writer of `eff` or `live` after them
  TsDevBuf eff, rids, compact_scratch, compact_stage;
  // update in place (ts_index_update): the staging tile of a chunk and its block tables
  TsDevBuf upd_tile, upd_tab;
  std::mutex eff_mu;
  hipEvent_t eff_ev = nullptr;
  bool eff_used = false;
  // range search (ts_index_range_search): the packed result of the last call (rng_cap entries
  // allocated, rng_total valid), kept for ts_index_range_fetch until the next range search or a change of the index;
  // rng_tiles: the dense path's per-query totals and tile counts.  range_mu serialises range calls on the handle.
  TsDevBuf rng_s, rng_i, rng_tiles;
  int64_t rng_cap = 0, rng_total = 0;
  bool rng_valid = false;
  std::mutex range_mu;
  // MMR (ts_index_mmr): scratch and staging, allocated at the first call
  TsMmrWork mmr;
  // rescore (ts_index_rescore): candidate tiles, scores and ids of one chunk of queries, allocated at
  // the first call; rescore_mu serialises the calls on the handle
  TsDevBuf rescore_scratch;
  std::mutex rescore_mu;
  // boosted search (ts_index_search_biased): the staged bias of a host-pointer call followed by the
  // 32-float padded copy of the last, partial row block's entries, allocated at the first call; bias_mu serialises
  // the calls on the handle; binfo: ts_index_last_bias_info
  TsDevBuf bias_stage;
  std::mutex bias_mu;
  int64_t binfo[4] = {0, 0, 0, 0};
};

static int co_flush(ts_index* h, hipStream_t s);

// Per-search profiling state (round 2 kept these three in the handle, written by every search: a data race
// between concurrent callers of one handle even with profiling off).
struct ProfCtx {
  bool now = false;         // this search is being timed (implies h->profiling, i.e. prof_mu is held)
  bool scan_only = false;   // asynchronous searches: only the scan+filter interval
  int nev = 0;
  int ev_phase[TS_NPHASE + 1] = {};
};

// profiling: mark(h, pc, phase, s) records an event; the time between two marks is
// charged to the phase of the FIRST mark.  Collected after the search's sync.
static void prof_mark(ts_index* h, ProfCtx& pc, int phase, hipStream_t s) {
  if (!pc.now || pc.nev > TS_NPHASE) return;
  if (pc.scan_only && phase != 3 && phase != 4) return;
  if (hipEventRecord(h->ev[pc.nev], s) != hipSuccess) return;
  pc.ev_phase[pc.nev] = phase;
  ++pc.nev;
}
static void prof_collect(ts_index* h, ProfCtx& pc) {
  if (!pc.now) return;
  std::lock_guard<std::mutex> lk(h->mu);
  for (int i = 0; i + 1 < pc.nev; ++i) {
    float ms = 0.f;
    const int ph = pc.ev_phase[i];
    if (ph >= 0 && ph < TS_NPHASE && hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]) == hipSuccess) {
      h->phase_ms[ph] += ms;
      h->phase_cnt[ph] += 1;
    }
  }
  pc.nev = 0;
}

static int grow_corpus(ts_index* h, int64_t need_blocks, bool exact, hipStream_t s) {
  if (need_blocks <= h->cap_blocks) return TS_OK;
  int64_t new_cap = need_blocks;
  if (!exact && h->cap_blocks > 0) new_cap = std::max(need_blocks, h->cap_blocks + h->cap_blocks / 2);
  const size_t bb = ts_block_bytes(h->L);
  void* np = nullptr;
  hipError_t e = hipMalloc(&np, (size_t)new_cap * bb);
  if (e != hipSuccess) {
    ts_set_error("cannot allocate %zu bytes for the corpus: %s", (size_t)new_cap * bb,
                 hipGetErrorString(e));
    return TS_ERR_OOM;
  }
  const int64_t used_blocks = (h->ntotal + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  if (used_blocks > 0)
    TS_HIP(hipMemcpyAsync(np, h->corpus, (size_t)used_blocks * bb, hipMemcpyDeviceToDevice, s));
  TS_HIP(hipMemsetAsync((char*)np + (size_t)used_blocks * bb, 0,
                        (size_t)(new_cap - used_blocks) * bb, s));
  TS_HIP(hipStreamSynchronize(s));
  if (h->corpus) TS_HIP(hipFree(h->corpus));
  h->corpus = (uint4*)np;
  h->cap_blocks = new_cap;
  return TS_OK;
}

extern "C" int ts_index_create(int32_t dim, int32_t storage_dtype, int32_t metric,
                               int32_t device, ts_index** out) {
  if (!out) { ts_set_error("out is null"); return TS_ERR_INVALID; }
  *out = nullptr;
  if (dim <= 0 || dim > 65536) { ts_set_error("bad dim %d", dim); return TS_ERR_INVALID; }
  if (storage_dtype != TS_F32 && storage_dtype != TS_F16 && storage_dtype != TS_BF16 &&
      storage_dtype != TS_FP8_E4M3 && storage_dtype != TS_MXFP4_E2M1) {
    ts_set_error("bad storage dtype %d", storage_dtype);
    return TS_ERR_INVALID;
  }
  if (metric != TS_METRIC_INNER_PRODUCT) {
    ts_set_error("only the inner-product metric is supported (reference uses IndexFlatIP)");
    return TS_ERR_UNSUPPORTED;
  }
  int ndev = 0;
  TS_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) {
    ts_set_error("device %d not present (%d HIP devices)", device, ndev);
    return TS_ERR_INVALID;
  }
  TsLayout L = ts_make_layout(dim, storage_dtype);
  if (storage_dtype == TS_MXFP4_E2M1 && dim > 2048) {   // (32 scale bytes per lane: two scale units, ts_scan_fp4.hip)
    ts_set_error("dim %d exceeds the 2048 dimensions of 4-bit MX (mxfp4) storage", dim);
    return TS_ERR_UNSUPPORTED;
  }
  if (ts_scan_lds_bytes(L, 1) > TS_LDS_BYTES) {
    ts_set_error("dim %d with dtype %d needs %zu bytes of LDS for 32 queries (max 163840)", dim,
                 storage_dtype, ts_scan_lds_bytes(L, 1));
    return TS_ERR_UNSUPPORTED;
  }
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  ts_index* h = new (std::nothrow) ts_index();
  if (!h) { ts_set_error("out of host memory"); return TS_ERR_OOM; }
  h->device = device;
  h->L = L;
  h->co_gmax = ts_coalesce_groups(dim, storage_dtype);
  h->co_gwide = ts_coalesce_groups_wide(dim, storage_dtype);
  h->co_gstat = ts_coalesce_groups_stationary(dim, storage_dtype);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    h->num_cus = prop.multiProcessorCount;
  // (the stationary pass's LDS attribute now: no first-launch cost inside a caller's timed pass)
  int st = ts_scan_qstat_prepare(L);
  for (ts_index::WSet& w : h->ws) {
    if (st == TS_OK) st = ts_buf_ensure(w.small, 4096);
    if (st == TS_OK && hipMemset(w.small.p, 0, 4096) != hipSuccess) { ts_set_error("hipMemset failed"); st = TS_ERR_HIP; }
    if (st == TS_OK) st = ts_buf_ensure(w.qimg, (size_t)L.qkg * 2 * 1024);
    if (st == TS_OK && (hipEventCreateWithFlags(&w.ev_pro, hipEventDisableTiming) != hipSuccess ||
                        hipEventCreateWithFlags(&w.ev_scan, hipEventDisableTiming) != hipSuccess ||
                        hipEventCreateWithFlags(&w.ev_sel, hipEventDisableTiming) != hipSuccess ||
                        hipEventCreateWithFlags(&w.ev_in, hipEventDisableTiming) != hipSuccess)) {
      ts_set_error("hipEventCreate failed");
      st = TS_ERR_HIP;
    }
  }
  // the workspaces' scratch pages are zeroed on the null stream: done before any stream's first search reads them
  if (st == TS_OK && hipStreamSynchronize(nullptr) != hipSuccess) { ts_set_error("hipStreamSynchronize failed"); st = TS_ERR_HIP; }
  if (st == TS_OK && (hipEventCreateWithFlags(&h->co_ev, hipEventDisableTiming) != hipSuccess ||
                      hipEventCreateWithFlags(&h->eff_ev, hipEventDisableTiming) != hipSuccess)) {
    ts_set_error("hipEventCreate failed");
    st = TS_ERR_HIP;
  }
  if (st == TS_OK &&
      (hipHostMalloc((void**)&h->host_status, (size_t)(TS_ASYNC_SLOTS + 1) * TS_SLOT_WORDS * 4, hipHostMallocMapped) != hipSuccess ||
       hipHostGetDevicePointer((void**)&h->host_status_dev, h->host_status, 0) != hipSuccess)) {
    ts_set_error("hipHostMalloc(mapped) failed");
    st = TS_ERR_HIP;
  }
  if (st != TS_OK) {
    ts_index_destroy(h);
    return st;
  }
  *out = h;
  return TS_OK;
}

extern "C" int ts_index_destroy(ts_index* h) {
  if (!h) return TS_OK;
  TsDeviceGuard g(h->device);
  (void)co_flush(h, nullptr);
  (void)hipDeviceSynchronize();
  if (h->corpus) (void)hipFree(h->corpus);
  TsDevBuf* bufs[] = {&h->stage, &h->den, &h->qstage, &h->out_s, &h->out_i, &h->mstage};
  for (TsDevBuf* b : bufs) ts_buf_release(*b);
  for (ts_index::WSet& w : h->ws) {
    TsDevBuf* wb[] = {&w.qimg, &w.small, &w.cand_score, &w.cand_id, &w.sample, &w.dense, &w.list_score, &w.list_id,
                      &w.hist, &w.spill, &w.mask, &w.mids};
    for (TsDevBuf* b : wb) ts_buf_release(*b);
    hipEvent_t evs[] = {w.ev_pro, w.ev_scan, w.ev_sel, w.ev_in};
    for (hipEvent_t e : evs)
      if (e) (void)hipEventDestroy(e);
  }
  hipStream_t strs[] = {h->s_pro, h->s_scan, h->s_sel};
  for (hipStream_t st_ : strs)
    if (st_) (void)hipStreamDestroy(st_);
  if (h->host_status) (void)hipHostFree(h->host_status);
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->async_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->co_ev) (void)hipEventDestroy(h->co_ev);
  TsDevBuf* rb[] = {&h->live, &h->eff, &h->rids, &h->compact_scratch, &h->compact_stage, &h->upd_tile, &h->upd_tab,
                    &h->rng_s, &h->rng_i, &h->rng_tiles, &h->rescore_scratch, &h->bias_stage};
  for (TsDevBuf* b : rb) ts_buf_release(*b);
  if (h->eff_ev) (void)hipEventDestroy(h->eff_ev);
  ts_mmr_release(h->mmr);
  delete h;
  return TS_OK;
}

extern "C" int ts_index_reset(ts_index* h) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  { TsDeviceGuard g(h->device); TS_CHECK(co_flush(h, nullptr)); }   // held passes search the corpus they were submitted against
  h->rng_valid = false;
  h->ntotal = 0;
  h->nremoved = 0;
  return TS_OK;
}

extern "C" int ts_index_reserve(ts_index* h, int64_t nrows) {
  if (!h || nrows < 0) { ts_set_error("bad arguments"); return TS_ERR_INVALID; }
  if (nrows >= (1LL << 31)) { ts_set_error("at most 2^31-1 rows per index"); return TS_ERR_UNSUPPORTED; }
  TsDeviceGuard g(h->device);
  TS_CHECK(co_flush(h, nullptr));   // (grow_corpus frees the old corpus after a sync of the null stream)
  return grow_corpus(h, (nrows + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK, true, nullptr);
}

extern "C" int64_t ts_index_ntotal(const ts_index* h) { return h ? h->ntotal : -1; }
extern "C" int32_t ts_index_dim(const ts_index* h) { return h ? h->L.dim : -1; }
extern "C" int32_t ts_index_dtype(const ts_index* h) { return h ? h->L.dtype : -1; }

// e4m3 storage: element x is stored as e4m3(x * 2^s).  s belongs to the stored bytes, so it can
// change only while there are none.
extern "C" int ts_index_set_fp8_scale_log2(ts_index* h, int32_t s) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  if (h->L.dtype != TS_FP8_E4M3) { ts_set_error("the index does not store e4m3"); return TS_ERR_INVALID; }
  if (s < 0 || s > 15) { ts_set_error("fp8 scale exponent %d is outside 0 .. 15", s); return TS_ERR_INVALID; }
  if (h->ntotal > 0) {
    ts_set_error("the fp8 scale exponent can be set only while the index is empty (%lld rows)", (long long)h->ntotal);
    return TS_ERR_INVALID;
  }
  h->L.fp8_scale_log2 = s;
  return TS_OK;
}

extern "C" int32_t ts_index_fp8_scale_log2(const ts_index* h) {
  return (h && h->L.dtype == TS_FP8_E4M3) ? h->L.fp8_scale_log2 : -1;
}

extern "C" int ts_index_set_id_offset(ts_index* h, int64_t offset) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  { TsDeviceGuard g(h->device); TS_CHECK(co_flush(h, nullptr)); }   // a held batch's ids carry the offset of its submission
  h->id_offset = offset;
  return TS_OK;
}

extern "C" int ts_index_last_search_info(const ts_index* h, int64_t info[4]) {
  if (!h || !info) { ts_set_error("bad arguments"); return TS_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(const_cast<ts_index*>(h)->mu);
  for (int i = 0; i < 4; ++i) info[i] = h->info[i];
  return TS_OK;
}

static size_t dtype_size(int dt) { return dt == TS_F32 ? 4 : 2; }

// the tombstone bitmap holds the words of `rows` rows; its content so far is kept
static int live_reserve(ts_index* h, int64_t rows, hipStream_t s) {
  const int64_t words = (rows + 31) / 32;
  if (words <= h->live_cap_words) return TS_OK;
  const int64_t cap = std::max<int64_t>(words, h->live_cap_words + h->live_cap_words / 2);
  TsDevBuf nb;
  TS_CHECK(ts_buf_ensure(nb, (size_t)cap * 4));
  TS_HIP(hipMemsetAsync(nb.p, 0, (size_t)cap * 4, s));
  if (h->live_cap_words > 0)
    TS_HIP(hipMemcpyAsync(nb.p, h->live.p, (size_t)h->live_cap_words * 4, hipMemcpyDeviceToDevice, s));
  TS_HIP(hipStreamSynchronize(s));
  ts_buf_release(h->live);
  h->live = nb;
  h->live_cap_words = cap;
  return TS_OK;
}
static bool dtype_ok(int dt) { return dt == TS_F32 || dt == TS_F16 || dt == TS_BF16; }

extern "C" int ts_index_add(ts_index* h, const void* rows, int64_t n, int32_t rows_dtype,
                            uint32_t flags, void* stream) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  if (n == 0) return TS_OK;
  if (!rows || n < 0 || !dtype_ok(rows_dtype)) { ts_set_error("bad arguments to add"); return TS_ERR_INVALID; }
  if (h->ntotal + n >= (1LL << 31)) { ts_set_error("at most 2^31-1 rows per index"); return TS_ERR_UNSUPPORTED; }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));   // held passes search the corpus they were submitted against
  h->rng_valid = false;       // a stored range result describes the index as it was
  const int64_t need_blocks = (h->ntotal + n + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  TS_CHECK(grow_corpus(h, need_blocks, false, s));
  const bool norm = (flags & TS_FLAG_NORMALIZE) != 0;
  const size_t row_bytes = (size_t)h->L.dim * dtype_size(rows_dtype);
  if (flags & TS_FLAG_HOST_PTR) {
    // chunked upload through a device staging buffer
    int64_t chunk = std::max<int64_t>(1, (int64_t)((64u << 20) / row_bytes));
    chunk = std::min(chunk, n);
    TS_CHECK(ts_buf_ensure(h->stage, (size_t)chunk * row_bytes));
    if (norm) TS_CHECK(ts_buf_ensure(h->den, (size_t)chunk * 4));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
      const int64_t c = std::min(chunk, n - r0);
      TS_HIP(hipMemcpyAsync(h->stage.p, (const char*)rows + (size_t)r0 * row_bytes,
                            (size_t)c * row_bytes, hipMemcpyHostToDevice, s));
      TS_CHECK(ts_launch_relayout(h->L, h->stage.p, rows_dtype, c, h->ntotal + r0, h->corpus,
                                  norm, (float*)h->den.p, s));
      // the staging buffer is reused by the next chunk
      TS_HIP(hipStreamSynchronize(s));
    }
  } else {
    if (norm) TS_CHECK(ts_buf_ensure(h->den, (size_t)n * 4));
    TS_CHECK(ts_launch_relayout(h->L, rows, rows_dtype, n, h->ntotal, h->corpus, norm,
                                (float*)h->den.p, s));
    TS_HIP(hipStreamSynchronize(s));
  }
  if (h->nremoved > 0) {   // the new rows are live
    TS_CHECK(live_reserve(h, h->ntotal + n, s));
    TS_CHECK(ts_launch_live_set((uint32_t*)h->live.p, h->ntotal, h->ntotal + n, s));
    TS_HIP(hipStreamSynchronize(s));
  }
  h->ntotal += n;
  return TS_OK;
}

extern "C" int ts_index_reconstruct(ts_index* h, int64_t row0, int64_t n, float* out,
                                    uint32_t flags, void* stream) {
  if (!h || !out || row0 < 0 || n < 0 || row0 + n > h->ntotal) {
    ts_set_error("bad arguments to reconstruct");
    return TS_ERR_INVALID;
  }
  if (n == 0) return TS_OK;
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));
  if (flags & TS_FLAG_HOST_PTR) {
    const size_t row_bytes = (size_t)h->L.dim * 4;
    int64_t chunk = std::max<int64_t>(1, (int64_t)((64u << 20) / row_bytes));
    chunk = std::min(chunk, n);
    TS_CHECK(ts_buf_ensure(h->stage, (size_t)chunk * row_bytes));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
      const int64_t c = std::min(chunk, n - r0);
      TS_CHECK(ts_launch_reconstruct(h->L, h->corpus, row0 + r0, c, (float*)h->stage.p, s));
      TS_HIP(hipMemcpyAsync((char*)out + (size_t)r0 * row_bytes, h->stage.p,
                            (size_t)c * row_bytes, hipMemcpyDeviceToHost, s));
      TS_HIP(hipStreamSynchronize(s));
    }
  } else {
    TS_CHECK(ts_launch_reconstruct(h->L, h->corpus, row0, n, out, s));
    TS_HIP(hipStreamSynchronize(s));
  }
  return TS_OK;
}

// ------------------------------------------------------------------ MMR (kernels: ts_mmr.hip)
extern "C" int ts_index_mmr(ts_index* h, const int64_t* cand_ids, const float* cand_rel, int32_t nq, int32_t fetch_k,
                            int32_t k, float lambda, float* out_rel, int64_t* out_ids, uint32_t flags, void* stream) {
  TS_CHECK(ts_mmr_check_args(h, cand_ids, cand_rel, nq, fetch_k, k, lambda, out_rel, out_ids));
  if (nq == 0) return TS_OK;
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));   // a held search's results are what the caller chains this call behind
  TsMmrSource src;
  src.corpus = h->corpus;
  src.L = h->L;
  src.ntotal = h->ntotal;
  src.id_offset = h->id_offset;
  src.live = h->nremoved > 0 ? (const uint32_t*)h->live.p : nullptr;
  src.ivf = false;
  src.id2slot = nullptr;
  src.blk_valid = nullptr;
  return ts_mmr_run(src, h->mmr, cand_ids, cand_rel, nq, fetch_k, k, lambda, out_rel, out_ids, flags, s);
}

extern "C" int ts_index_mmr_set_timing(ts_index* h, int32_t on) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  h->mmr.timing = on != 0;
  return TS_OK;
}

extern "C" int ts_index_mmr_get_timings(ts_index* h, double ms[3], int64_t* calls, int32_t reset) {
  if (!h || !ms || !calls) { ts_set_error("bad arguments"); return TS_ERR_INVALID; }
  for (int i = 0; i < 3; ++i) ms[i] = h->mmr.phase_ms[i];
  *calls = h->mmr.timed_calls;
  if (reset) {
    for (double& m : h->mmr.phase_ms) m = 0.0;
    h->mmr.timed_calls = 0;
  }
  return TS_OK;
}

// ------------------------------------------------------------------ search
static int queries_per_pass(const ts_index* h) { return ts_queries_per_pass(h->L); }

static int err_empty() {
  ts_set_error("No documents indexed. Call add_documents() first.");
  return TS_ERR_EMPTY;
}

// The CUs of an HBM-bound filter scan, 7/8 of them: 224 CUs stream 1.5 % FASTER than 256 (tools/cus.sh), and the free
// eighth is where the threshold workgroups of the one-launch search and the neighbouring searches' small kernels run.
static int filter_scan_cus(const ts_index* h) {
  int cus = h->num_cus - h->num_cus / 8;
#ifdef TS_TUNING  // ablation builds only: how many CUs a filter scan may occupy
  static const int dbg_cus = getenv("TS_SCAN_CUS") ? atoi(getenv("TS_SCAN_CUS")) : 0;
  if (dbg_cus > 0) cus = dbg_cus;
#endif
  return cus;
}

// One pass of a filtered search (ts_index_search_filtered): the masks (device) and the pass's tables.
struct MaskCtx {
  const uint32_t* bits;
  int64_t words;
  TsMaskPass mp;
  // boosted passes (ts_index_search_biased): the per-row bias and the padded copy of its last partial row block
  const float* bias;
  const float* bias_tail;
};

// The tables of a pass of c queries, query j on mask moq[j] (-1: none): each query's mask and the distinct masks among
// them.  Returns whether a query has a mask.
static bool build_mask_pass(const int32_t* moq, int c, TsMaskPass& mp) {
  mp = TsMaskPass{};
  bool masked = false;
  for (int j = 0; j < TS_MAX_Q; ++j) {
    const int32_t m = j < c ? moq[j] : -1;
    mp.qmask[j] = m;
    mp.qd[j] = -1;
    if (j >= c) continue;
    if (m < 0) { mp.all_live = 1; continue; }
    masked = true;
    int d = 0;
    while (d < mp.nd && mp.dist[d] != m) ++d;
    if (d == mp.nd) mp.dist[mp.nd++] = m;
    mp.qd[j] = d;
  }
  return masked;
}

// The mask arguments of the filtered entry points, in two parts: what needs no handle (a null mask_of_query, no query
// with a mask, is the caller's to accept or refuse), then what needs the row count.
static int check_mask_args(const char* entry, int32_t nq, const uint32_t* allow_bits, int64_t allow_words,
                           int32_t n_masks, const int32_t* mask_of_query) {
  if (n_masks < 0 || allow_words < 0) { ts_set_error("%s: negative n_masks / allow_words", entry); return TS_ERR_INVALID; }
  if (n_masks > 0 && !allow_bits) { ts_set_error("%s: n_masks > 0 but allow_bits is null", entry); return TS_ERR_INVALID; }
  for (int32_t q = 0; mask_of_query && q < nq; ++q) {
    if (mask_of_query[q] < -1 || mask_of_query[q] >= n_masks) {
      ts_set_error("%s: mask_of_query[%d] = %d is outside [-1, %d)%s", entry, q, mask_of_query[q], n_masks,
                   allow_bits ? "" : " (allow_bits is null)");
      return TS_ERR_INVALID;
    }
  }
  return TS_OK;
}
static int check_mask_words(const char* entry, int32_t n_masks, int64_t allow_words, int64_t ntotal) {
  const int64_t need_words = (ntotal + 31) / 32;
  if (n_masks > 0 && allow_words < need_words) {
    ts_set_error("%s: allow_words = %lld < ceil(ntotal / 32) = %lld", entry, (long long)allow_words, (long long)need_words);
    return TS_ERR_INVALID;
  }
  return TS_OK;
}

// The parameters every scan of a pass takes; scan_window() or scan_filter() add those of its mode.
static ScanParams scan_base(const ts_index* h, const ts_index::WSet& W, int nq) {
  ScanParams sp{};
  sp.corpus = h->corpus;
  sp.qimg = (const uint4*)W.qimg.p;
  sp.kg = h->L.kg;
  sp.nq = nq;
  sp.ntotal = h->ntotal;
  return sp;
}
// dense mode: the scores of nwork row blocks, `stride` apart from blk0 on, to dense[q * ld + ..]
static void scan_window(ScanParams& sp, int64_t blk0, int64_t nwork, int64_t stride, float* dense, int64_t ld) {
  sp.blk0 = blk0;
  sp.nwork = nwork;
  sp.blk_stride = stride;
  sp.dense = dense;
  sp.dense_ld = ld;
}
// filter mode: every row block against the set's thresholds, the survivors to its candidate lists
static void scan_filter(ScanParams& sp, ts_index::WSet& W, int64_t nblk) {
  scan_window(sp, 0, nblk, 1, nullptr, 0);
  sp.tau = W.tau();
  sp.cand_cnt = W.cand_cnt();
  sp.cand_score = (float*)W.cand_score.p;
  sp.cand_id = (int32_t*)W.cand_id.p;
  sp.cand_cap = kCandCap;
}

// A scan of the whole rows (pkg == 0) or of the first pkg k groups of every row (ts_index_search_prefix): the same
// parameters, the prefix scans add the pitch of the row blocks.
static int scan_rows(ts_index* h, int pkg, int mode, int qh, const ScanParams& sp, int cus, hipStream_t s) {
  if (!pkg) return ts_launch_scan(h->L, mode, qh, sp, cus, s);
  PrefixScanParams pp{};
  static_cast<ScanParams&>(pp) = sp;
  pp.kg = pkg;
  pp.kg_row = h->L.kg;
  return ts_launch_scan_prefix(h->L, mode, qh, pp, cus, s);
}

// The live-block list of a masked pass into the set's TsMaskDev (W.mask_dev()), on `s`.
static int launch_live_blocks(ts_index* h, ts_index::WSet& W, const MaskCtx& mc, hipStream_t s) {
  const int64_t nblk = (h->ntotal + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  TS_CHECK(ts_buf_ensure(W.mask, sizeof(TsMaskDev) + (size_t)nblk * 4));
  TS_HIP(hipMemsetAsync(W.mask_dev(), 0, sizeof(TsMaskDev), s));
  return ts_launch_live_blocks(mc.bits, mc.words, mc.mp, nblk, h->ntotal, W.mask_dev(), s);
}
// the masked form of a filter scan: its work items are the blocks of that list
static MaskedScanParams masked_scan_params(const ScanParams& sp, ts_index::WSet& W, const MaskCtx& mc) {
  const TsMaskDev* md = W.mask_dev();
  MaskedScanParams mp{};
  static_cast<ScanParams&>(mp) = sp;
  mp.live = reinterpret_cast<const int32_t*>(md + 1);
  mp.nlive = &md->nlive;
  mp.allow_bits = mc.bits;
  mp.allow_words = mc.words;
  mp.qmask = md->qmask;
  return mp;
}

// The dense path scores the corpus in chunks of at most kDenseChunkRows rows (whole row blocks).
struct DenseChunks { int64_t chunk_rows, nch; };
static DenseChunks dense_chunks(int64_t ntotal) {
  const int64_t nblk = (ntotal + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  const int64_t chunk_rows = std::min<int64_t>(kDenseChunkRows, nblk * TS_ROWS_PER_BLOCK);
  return DenseChunks{chunk_rows, (nblk * TS_ROWS_PER_BLOCK + chunk_rows - 1) / chunk_rows};
}
// one chunk: the scores of rows [row0, row0 + rows) into W.dense
static int dense_chunk_scan(ts_index* h, ts_index::WSet& W, int nq, int qh, int pkg, int64_t row0, int64_t rows,
                            int64_t chunk_rows, hipStream_t s) {
  ScanParams sp = scan_base(h, W, nq);
  scan_window(sp, row0 / TS_ROWS_PER_BLOCK, (rows + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK, 1, (float*)W.dense.p,
              chunk_rows);
  return scan_rows(h, pkg, SCAN_DENSE, qh, sp, h->num_cus, s);
}

static int dense_path(ts_index* h, ts_index::WSet& W, int nq, int qh, int k, float* out_s,
                      int64_t* out_i, hipStream_t s, const MaskCtx* mc = nullptr, int pkg = 0) {
  const int64_t N = h->ntotal;
  const auto [chunk_rows, nch] = dense_chunks(N);
  TS_CHECK(ts_buf_ensure(W.dense, (size_t)nq * chunk_rows * 4));
  if (mc) TS_CHECK(ts_buf_ensure(W.mids, (size_t)nq * chunk_rows * 4));
  if (nch > 1) {
    TS_CHECK(ts_buf_ensure(W.list_score, (size_t)nq * nch * k * 4));
    TS_CHECK(ts_buf_ensure(W.list_id, (size_t)nq * nch * k * 4));
  }
  for (int64_t c = 0; c < nch; ++c) {
    const int64_t row0 = c * chunk_rows;
    const int64_t rows = std::min(chunk_rows, N - row0);
    TS_CHECK(dense_chunk_scan(h, W, nq, qh, pkg, row0, rows, chunk_rows, s));
    SelParams p{};
    p.mode = SEL_DENSE;
    p.scores = (const float*)W.dense.p;
    p.stride = chunk_rows;
    p.n = (uint32_t)rows;
    p.id_base = (int32_t)row0;
    p.k = k;
    if (mc) {
      // filtered: the rows outside a query's mask get id -1 and with it no rank (SEL_PAIRS32 skips them),
      // so the result is padded with -1 / -FLT_MAX, never with disallowed rows
      if (mc->bias)   // boosted: the same ids, and the chunk's scores become score + bias
        TS_CHECK(ts_launch_bias_ids(mc->bits, mc->words, mc->mp, mc->bias, nq, row0, (uint32_t)rows, chunk_rows,
                                    (float*)W.dense.p, (int32_t*)W.mids.p, s));
      else
        TS_CHECK(ts_launch_mask_ids(mc->bits, mc->words, mc->mp, nq, row0, (uint32_t)rows, chunk_rows,
                                    (int32_t*)W.mids.p, s));
      p.mode = SEL_PAIRS32;
      p.ids32 = (const int32_t*)W.mids.p;
    }
    if (nch == 1) {
      p.out_scores = out_s;
      p.out_ids64 = out_i;
      p.out_stride = k;
      p.id_offset = h->id_offset;
    } else {
      p.out_scores = (float*)W.list_score.p + c * k;
      p.out_ids32 = (int32_t*)W.list_id.p + c * k;
      p.out_stride = nch * k;
    }
    TS_CHECK(ts_launch_select(p, nq, s));
  }
  if (nch > 1) {
    SelParams p{};
    p.mode = SEL_PAIRS32;
    p.scores = (const float*)W.list_score.p;
    p.ids32 = (const int32_t*)W.list_id.p;
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

// One wave that does nothing for ~`us` microseconds (bounded: at most `max_iter` short sleeps).
// Put in front of a helper kernel that becomes runnable at the same instant as the next scan, it
// lets the scan's workgroups be placed first (see search_pass).
__global__ void head_start_kernel(int us, int max_iter) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
  for (int i = 0; i < max_iter; ++i) {
    if (__builtin_amdgcn_s_memrealtime() - t0 >= (unsigned long long)us * 100ull) break;
    __builtin_amdgcn_s_sleep(32);
  }
}

static int ensure_streams(ts_index* h) {
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->s_pro) return TS_OK;
  // The scan stream outranks the two helper streams: when a scan and the previous
  // search's select become runnable at the same instant (both wait for the same scan
  // to end), the scan's workgroups must be placed first — a scan workgroup that starts
  // late finishes late, because every workgroup owns a fixed share of the rows.
  int lo = 0, hi = 0;  // numerically lower = higher priority
  TS_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
  TS_HIP(hipStreamCreateWithPriority(&h->s_scan, hipStreamNonBlocking, hi));
  TS_HIP(hipStreamCreateWithPriority(&h->s_sel, hipStreamNonBlocking, lo));
  TS_HIP(hipStreamCreateWithPriority(&h->s_pro, hipStreamNonBlocking, lo));   // (last: it is the "created" flag)
  return TS_OK;
}

// ---- geometry of the one-launch search
struct FusedPlan {
  int scan_wgs, tau_wgs;
  int64_t n_sample, sample_stride, sample_rows;
  uint32_t m, expect, sample_waves;
};
static bool plan_fused(const ts_index* h, int64_t N, int64_t nblk, int k, bool pipe, FusedPlan* fp) {
  // the scan takes 7/8 of the CUs (the kernel is HBM-bound: 224 CUs stream as fast as 256, tools/cus.sh); the
  // threshold workgroups, and in pipelined mode the neighbours' select and the exchange, use the rest.  The next
  // search's kernel follows on the SAME stream, so its workgroups are dispatched the moment this one ends, ahead
  // of the select that waits for this kernel through an event on another stream: no placement race.
  (void)pipe;
  const int scan_wgs = filter_scan_cus(h);
  if (scan_wgs < 1) return false;
  const int tau_wgs = std::max(1, std::min(64, h->num_cus - scan_wgs));
  const int64_t nwaves = (int64_t)scan_wgs * 8;
  if (nblk < nwaves) return false;                         // fewer row blocks than waves: a latency-bound corpus
  const int64_t want_rows = std::max(kMinSampleRows, N / kSampleDiv);
  int64_t R = (want_rows + nwaves * TS_ROWS_PER_BLOCK - 1) / (nwaves * TS_ROWS_PER_BLOCK);
  R = std::max<int64_t>(1, std::min<int64_t>(R, 16));
  int64_t n_sample = std::min(nblk, R * nwaves);
  // A scan wave can deliver at most THREE sample rounds before it needs the thresholds: it parks two score tiles
  // and blocks in tau_wait() behind the third block's key store (ts_fused.hip).  A fourth round's keys would never
  // be written, the threshold waves and the scan waves would wait for each other until both time out, and the
  // batch would fall back to the dense path — correct but 40-60 ms (round 2: any corpus above ~22 M rows on 256 CUs).
  n_sample = std::min<int64_t>(n_sample, 3 * nwaves);
  n_sample = std::min<int64_t>(n_sample, TS_FUSED_MAX_KEYS / 2) & ~(int64_t)255;   // two slots per block; groups of 8 blocks;
  if (n_sample < 256) return false;                                                 // slots a multiple of 512
  int64_t stride = nblk / (n_sample / 8);                   // between the first blocks of consecutive 8-block groups (>= 8)
#ifdef TS_TUNING   // experiment: the sample is the first n_sample blocks of the corpus (biased for grouped corpora)
  static const bool dbg_prefix = getenv("TS_FUSED_PREFIX_SAMPLE") != nullptr;
  if (dbg_prefix) stride = 8;
#endif
  const int64_t rows = n_sample * TS_ROWS_PER_BLOCK;
  const int64_t oversample = k > 1024 ? 3 : kOversample;
  uint32_t m = (uint32_t)((oversample * (int64_t)k * rows + N - 1) / N);
  m = std::max(m, kMinSampleRank);
  const uint32_t expect = (uint32_t)(2 * n_sample);        // one group maximum per (wave, round, lane half)
  if ((uint64_t)m * 4 > expect) return false;              // group maxima would no longer stand in for scores
  fp->scan_wgs = scan_wgs;
  fp->tau_wgs = tau_wgs;
  fp->n_sample = n_sample;
  fp->sample_stride = stride;
  fp->sample_rows = rows;
  fp->m = m;
  fp->expect = expect;
  fp->sample_waves = (uint32_t)std::min<int64_t>(scan_wgs, n_sample / 8);   // WORKGROUPS that report: one arrival each
  return true;
}

// ---- the set pool and the report-slot ring (both under h->mu)
static ts_index::WSet* acquire_set(ts_index* h) {
  std::unique_lock<std::mutex> lk(h->mu);
  for (;;) {
    for (int t = 0; t < TS_NSETS; ++t) {
      ts_index::WSet& w = h->ws[(h->set_next + t) % TS_NSETS];
      if (!w.busy) {
        h->set_next = (h->set_next + t + 1) % TS_NSETS;   // round robin: pipelined searches alternate sets
        w.busy = true;
        return &w;
      }
    }
    h->cv.wait(lk);   // TS_NSETS synchronous searches in flight: wait for one to return
  }
}
static void release_set(ts_index* h, ts_index::WSet* w) {
  {
    std::lock_guard<std::mutex> lk(h->mu);
    w->busy = false;
  }
  h->cv.notify_one();
}
namespace {
// A workspace set held for one pass: taken from the pool, given back on every exit.  wait_previous() orders a stream
// behind the set's last user, done() records the end of this one for the next.
struct SetLease {
  ts_index* h;
  ts_index::WSet* W;
  explicit SetLease(ts_index* h_) : h(h_), W(acquire_set(h_)) {}
  ~SetLease() { if (W) release_set(h, W); }
  SetLease(const SetLease&) = delete;
  SetLease& operator=(const SetLease&) = delete;
  // the set may still be in use on the GPU by the (asynchronous) search that had it last, possibly on another stream
  // (asked first whether that search is already over — with eight sets in rotation it normally is: a wait on
  // another stream's event in front of every scan, even a satisfied one, costs the scan stream 10-20 us)
  int wait_previous(hipStream_t s) {
    if (W->used && hipEventQuery(W->ev_sel) != hipSuccess) TS_HIP(hipStreamWaitEvent(s, W->ev_sel, 0));
    return TS_OK;
  }
  int done(hipStream_t s) {
    TS_HIP(hipEventRecord(W->ev_sel, s));
    W->used = true;
    return TS_OK;
  }
  // the set stays busy in its new holder's hands (co_submit: until co_launch_pass has enqueued the batch's select)
  ts_index::WSet* detach() {
    ts_index::WSet* w = W;
    W = nullptr;
    return w;
  }
};
}  // namespace
// a free slot of the mapped host ring (at most 64 asynchronous passes + TS_NSETS synchronous ones hold one)
static int alloc_slot(ts_index* h) {
  std::lock_guard<std::mutex> lk(h->mu);
  for (int t = 0; t < TS_ASYNC_SLOTS; ++t) {
    const int sl = (int)((h->slot_next + t) % TS_ASYNC_SLOTS);
    if (!h->slot_busy[sl]) {
      h->slot_busy[sl] = true;
      h->slot_next = (uint64_t)sl + 1;
      return sl;
    }
  }
  return -1;
}
static void free_slot(ts_index* h, int sl) {
  std::lock_guard<std::mutex> lk(h->mu);
  if (sl >= 0 && sl < TS_ASYNC_SLOTS) h->slot_busy[sl] = false;
}
// a report slot is given back on every exit of a search unless its ownership has moved to pending[]
struct SlotGuard {
  ts_index* h;
  int slot;
  SlotGuard(ts_index* h_, int slot_) : h(h_), slot(slot_) {}
  ~SlotGuard() { if (slot >= 0) free_slot(h, slot); }
  void handed_over() { slot = -1; }
  SlotGuard(const SlotGuard&) = delete;
  SlotGuard& operator=(const SlotGuard&) = delete;
};
static void set_info(ts_index* h, int64_t a, int64_t b, int64_t c, int64_t d) {
  std::lock_guard<std::mutex> lk(h->mu);
  h->info[0] = a; h->info[1] = b; h->info[2] = c; h->info[3] = d;
}

// An unfinished asynchronous pass, verified by ts_index_finish().  Caller holds h->mu.
static ts_index::Pending& push_pending(ts_index* h, int slot, int nq, int64_t S, uint32_t m, int set, int64_t fseq) {
  ts_index::Pending& pe = h->pending[h->npending++];
  pe.ticket = h->next_ticket; pe.slot = slot; pe.nq = nq; pe.S = (uint32_t)S; pe.m = m;
  pe.e0 = pe.e1 = nullptr;
  pe.set = set;
  pe.fseq = fseq;
  return pe;
}

// ts_index_last_filter_info: one pass of the filtered call `fseq` (a later call has reset the counters)
static void add_filter_info(ts_index* h, int64_t fseq, int64_t live, int64_t blocks, bool dense) {
  std::lock_guard<std::mutex> lk(h->mu);
  if (fseq != h->fseq) return;
  h->finfo[0] += live;
  h->finfo[1] += blocks;
  h->finfo[dense ? 3 : 2] += 1;
}

// ts_index_last_bias_info: one pass of a boosted call (bias_mu is held: one call at a time)
static void add_bias_info(ts_index* h, bool fused, bool redone, int64_t blocks) {
  std::lock_guard<std::mutex> lk(h->mu);
  h->binfo[0] += 1;
  h->binfo[1] += fused ? 1 : 0;
  h->binfo[2] += redone ? 1 : 0;
  h->binfo[3] += blocks;
}

// ---- geometry of the five-launch path: the strided sample of row blocks whose scores give the thresholds, and the
// rank m of the sample score that becomes one, for about oversample * k expected survivors per query
struct SampleGeom {
  int64_t nsb, sstride, S;   // sample blocks, the stride between them, sample rows
  uint32_t m;
};
static SampleGeom sample_geometry(const ts_index* h, int k, int64_t oversample) {
  const int64_t N = h->ntotal;
  const int64_t nblk = (N + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  int64_t nsb = std::max(kMinSampleRows, N / kSampleDiv) / TS_ROWS_PER_BLOCK;
  // one sample block per scan wave (8 waves per CU): a ragged last round would
  // make the short sample scan ~1.7x longer than it has to be
  const int64_t round = (int64_t)h->num_cus * 8;
  if (nsb > round) nsb -= nsb % round;
  nsb = std::min(nsb, nblk);
  SampleGeom g{nsb, nblk / nsb, nsb * TS_ROWS_PER_BLOCK, 0};
  g.m = std::max((uint32_t)((oversample * (int64_t)k * g.S + N - 1) / N), kMinSampleRank);
  return g;
}

// The exact top-k of a set's candidates.  The select kernel verifies that `need` of them exist (0: need_check_kernel
// has the per-query figure) and reports the candidate counts and the status word straight into mapped host memory: no
// copy kernel between it and the sync; every search in flight has its own slot of the ring.
static SelParams cand_select_params(const ts_index* h, ts_index::WSet& W, int k, uint32_t need, float* out_s,
                                    int64_t* out_i, int slot) {
  SelParams p{};
  p.mode = SEL_PAIRS32;
  p.scores = (const float*)W.cand_score.p;
  p.ids32 = (const int32_t*)W.cand_id.p;
  p.stride = kCandCap;
  p.n_per_q = W.cand_cnt();
  p.n_cap = kCandCap;
  p.need = need;
  p.k = k;
  p.out_scores = out_s;
  p.out_ids64 = out_i;
  p.out_stride = k;
  p.id_offset = h->id_offset;
  p.status = W.status();
  p.clear_counts = W.cand_cnt();   // counts go back to zero: the one-launch search has no preparation kernel to do it
  p.host_report = h->host_status_dev + (size_t)slot * TS_SLOT_WORDS;
  return p;
}

namespace {
// ---- one pass of <= 32*qh queries (device pointers): what its phases share.  search_pass_on fixes the first part;
// the phases write the second.
struct Pass {
  ts_index* const h;
  SetLease& set;
  const void* const dq;
  const int nq, q_dtype, qh, k, pkg;
  float* const out_s;
  int64_t* const out_i;
  const MaskCtx* const mc;
  const int64_t N, nblk, fseq;
  const bool async, pipe, fused;
  const hipStream_t s, sP, sS, sL;   // the caller's stream; those of the phases P, S and Sel
  SlotGuard slot;                    // the report slot: every early return gives it back
  ProfCtx pc{};
  int64_t S = 0;                     // sample rows and the rank behind the thresholds (ts_index_last_search_info)
  uint32_t m = 0;
};
}  // namespace

// The dense pass (no filter: small corpora, large k, TS_FLAG_NO_FILTER, masked fp32 storage), all on the caller's stream.
static int pass_dense(Pass& p) {
  ts_index* h = p.h;
  set_info(h, 0, 0, 0, 0);
  if (p.mc) add_filter_info(h, p.fseq, p.nblk, p.nblk, true);
  if (p.mc && p.mc->bias) add_bias_info(h, false, false, p.nblk);
  prof_mark(h, p.pc, 5, p.s);
  TS_CHECK(dense_path(h, *p.set.W, p.nq, p.qh, p.k, p.out_s, p.out_i, p.s, p.mc, p.pkg));
  prof_mark(h, p.pc, -1, p.s);
  TS_CHECK(p.set.done(p.s));
  if (p.async) return TS_OK;  // exact by construction: nothing to verify
  TS_HIP(hipStreamSynchronize(p.s));
  prof_collect(h, p.pc);
  return TS_OK;
}

// ONE launch: query image, thresholds and scan+filter (see ts_fused.hip)
static int pass_one_launch(Pass& p, const FusedPlan& fp) {
  ts_index* h = p.h;
  ts_index::WSet& W = *p.set.W;
  if (!W.hist.p) {
    TS_CHECK(ts_buf_ensure(W.hist, ts_fused_keys_bytes()));
    W.hist_dirty = true;
  }
  if (W.hist_dirty) {
    // a launch on this set gave up somewhere: slots may hold stale keys, and sample workgroups that left before
    // reporting have put the arrival counter behind its running goal for good — start all three from zero
    TS_HIP(hipMemsetAsync(W.hist.p, 0, ts_fused_keys_bytes(), p.sS));
    TS_HIP(hipMemsetAsync(W.cand_cnt(), 0, 256, p.sS));
    TS_HIP(hipMemsetAsync(W.arrive(), 0, 4, p.sS));
    W.arrive_total = 0;
    W.hist_dirty = false;
  }
  if (++W.gen == 0) W.gen = 1;
  W.arrive_total += fp.sample_waves;
  TsFusedArgs a{};
  a.corpus = h->corpus;
  a.queries = p.dq;
  a.q_dtype = p.q_dtype;
  a.nq = p.nq;
  a.nblk = p.nblk;
  a.ntotal = p.N;
  a.scan_wgs = fp.scan_wgs;
  a.tau_wgs = fp.tau_wgs;
  a.n_sample = fp.n_sample;
  a.sample_stride = fp.sample_stride;
  a.m = fp.m;
  a.expect = fp.expect;
  a.gen = W.gen;
  a.arrive_goal = W.arrive_total;
  a.wait_iters = 40000;
  a.skeys = (uint32_t*)W.hist.p;
  a.arrive = W.arrive();
  a.tau64 = W.tau64();
  a.cand_cnt = W.cand_cnt();
  a.cand_score = (float*)W.cand_score.p;
  a.cand_id = (int32_t*)W.cand_id.p;
  a.cand_cap = kCandCap;
  prof_mark(h, p.pc, 3, p.sS);
  TS_CHECK(ts_launch_fused(h->L, p.qh, a, p.sS));
  prof_mark(h, p.pc, 4, p.sS);
  p.S = fp.sample_rows;
  p.m = fp.m;
  return TS_OK;
}

// Five launches: sample -> thresholds -> scan+filter (-> select: pass_select).  Filtered passes (mc != null) take the
// live-block list and the masked scan, boosted ones its biased form, prefix passes the prefix kernels.
static int pass_five_launch(Pass& p) {
  ts_index* h = p.h;
  ts_index::WSet& W = *p.set.W;
  const MaskCtx* mc = p.mc;
  // expected survivors per query ~ oversample * k; 3x for large k keeps the worst query of a
  // batch (about 1.5x the mean) well inside the 16384 candidate slots
  const int64_t oversample = p.k > 1024 ? 3 : kOversample;
  const SampleGeom g = sample_geometry(h, p.k, oversample);
  p.S = g.S;
  p.m = g.m;
  TS_CHECK(ts_buf_ensure(W.sample, (size_t)p.nq * g.S * 4));
  ScanParams sp = scan_base(h, W, p.nq);
  // (1) dense scores of a strided sample of row blocks
  scan_window(sp, 0, g.nsb, g.sstride, (float*)W.sample.p, g.S);
  prof_mark(h, p.pc, 1, p.sP);
  TS_CHECK(scan_rows(h, p.pkg, SCAN_DENSE, p.qh, sp, h->num_cus, p.sP));
  prof_mark(h, p.pc, 2, p.sP);
  // (2) per-query threshold = ~m-th best sample score
  if (mc) {
    // (2') the live-block list of the pass, then per query the m_q-th best ALLOWED sample score (+ bias: boosted); the
    // threshold kernel also reports the live-block count (word 65 of the slot)
    TS_CHECK(launch_live_blocks(h, W, *mc, p.sP));
    uint32_t* report = h->host_status_dev + (size_t)p.slot.slot * TS_SLOT_WORDS + 65;
    if (mc->bias)
      TS_CHECK(ts_launch_tau_biased((const float*)W.sample.p, g.S, g.sstride, p.N, mc->bits, mc->words, mc->bias,
                                    W.mask_dev(), p.nq, p.k, (uint32_t)oversample, kMinSampleRank, W.tau(), report, p.sP));
    else
      TS_CHECK(ts_launch_tau_masked((const float*)W.sample.p, g.S, g.sstride, p.N, mc->bits, mc->words, W.mask_dev(),
                                    p.nq, p.k, (uint32_t)oversample, kMinSampleRank, W.tau(), report, p.sP));
  } else {
#ifdef TS_TUNING  // ablation builds only (tools/variants.sh): thresholds = +inf, nothing survives
    static const bool dbg_tau_inf = getenv("TS_DEBUG_TAU_INF") != nullptr;
#else
    constexpr bool dbg_tau_inf = false;
#endif
    TS_CHECK(ts_launch_tau((const float*)W.sample.p, g.S, dbg_tau_inf ? 0xFFFFFFFFu : (uint32_t)g.S, g.m, p.nq, W.tau(),
                           p.sP));
  }
  if (p.pipe) {
    TS_HIP(hipEventRecord(W.ev_pro, p.sP));
    TS_HIP(hipStreamWaitEvent(p.sS, W.ev_pro, 0));
  }
  // (3) the full scan; only scores >= tau leave the registers
  scan_filter(sp, W, p.nblk);
  const int scan_cus = filter_scan_cus(h);
  prof_mark(h, p.pc, 3, p.sS);
  if (!mc) {
    TS_CHECK(scan_rows(h, p.pkg, SCAN_FILTER, p.qh, sp, scan_cus, p.sS));
  } else if (mc->bias) {
    BiasScanParams bp{};
    static_cast<MaskedScanParams&>(bp) = masked_scan_params(sp, W, *mc);
    bp.bias = mc->bias;
    bp.bias_tail = mc->bias_tail;
    bp.tail_blk = (p.N % TS_ROWS_PER_BLOCK) ? p.N / TS_ROWS_PER_BLOCK : -1;
    TS_CHECK(ts_launch_scan_biased(h->L, p.qh, bp, scan_cus, p.sS));
  } else if (p.pkg) {
    PrefixMaskedScanParams pp{};
    static_cast<MaskedScanParams&>(pp) = masked_scan_params(sp, W, *mc);
    pp.kg = p.pkg;
    pp.kg_row = h->L.kg;
    TS_CHECK(ts_launch_scan_prefix_masked(h->L, p.qh, pp, scan_cus, p.sS));
  } else {
    TS_CHECK(ts_launch_scan_masked(h->L, p.qh, masked_scan_params(sp, W, *mc), scan_cus, p.sS));
  }
  prof_mark(h, p.pc, 4, p.sS);
  return TS_OK;
}

// Select and report: (4) the exact top-k of the candidates on the select stream, which verifies that >= k of them
// exist; the set's next user and, pipelined, the caller's stream are ordered behind it.
static int pass_select(Pass& p) {
  ts_index* h = p.h;
  ts_index::WSet& W = *p.set.W;
  if (p.pipe) {
    TS_HIP(hipEventRecord(W.ev_scan, p.sS));
    TS_HIP(hipStreamWaitEvent(p.sL, W.ev_scan, 0));
    TS_HIP(hipStreamWaitEvent(p.sL, W.ev_in, 0));
    // This select and the NEXT search's scan wait for the same event.  If the select's 64
    // workgroups (128 KiB of LDS each: they cannot share a CU with a scan workgroup) are placed
    // first they take 64 CUs, 32 of the scan's 224 persistent workgroups have to wait for them,
    // and the whole scan ends that much later — stream priority does not prevent it (measured:
    // overlapped scans of 0.305-0.326 ms instead of 0.289 at 1.25 M rows, 2.263 instead of 2.207
    // at 10 M).  A head start of a few microseconds for the scan does: the select then finds the
    // 32 CUs the scan grid leaves free.
#ifdef TS_TUNING
    static const int head_us = getenv("TS_HEAD_START_US") ? atoi(getenv("TS_HEAD_START_US")) : kHeadStartUs;
#else
    constexpr int head_us = kHeadStartUs;
#endif
    // (the one-launch scan occupies 3/4 of the CUs: the select's 64 workgroups always fit beside it)
    if (head_us > 0 && !p.fused) hipLaunchKernelGGL(head_start_kernel, dim3(1), dim3(64), 0, p.sL, head_us, 4096);
  }
  // (a filtered pass has its slot already: its threshold kernel reports into it)
  if (!p.mc) {
    p.slot.slot = alloc_slot(h);
    if (p.slot.slot < 0) { ts_set_error("no free report slot"); return TS_ERR_INVALID; }
  }
  // (filtered: need_check_kernel, min(k, N_q))
  const SelParams sel = cand_select_params(h, W, p.k, p.mc ? 0u : (uint32_t)std::min<int64_t>(p.k, p.N), p.out_s,
                                           p.out_i, p.slot.slot);
  if (p.mc) {
    TS_CHECK(ts_launch_need_check(W.cand_cnt(), W.mask_dev()->need, p.nq, W.status(), sel.host_report, p.sL));
  } else {
    uint32_t* rep = h->host_status + (size_t)p.slot.slot * TS_SLOT_WORDS;
    for (int i = 0; i < 65; ++i) rep[i] = 0;
  }
  TS_CHECK(ts_launch_select(sel, p.nq, p.sL));
  TS_CHECK(p.set.done(p.sL));
  if (p.pipe) TS_HIP(hipStreamWaitEvent(p.s, W.ev_sel, 0));  // later work on the caller's stream sees the result
  return TS_OK;
}

// The synchronous end of a filter pass: wait, read the report, and redo the pass exactly where a threshold was too
// high (fewer than k survivors) or too low (candidate list overflowed, e.g. massive score ties).
static int pass_verify(Pass& p) {
  ts_index* h = p.h;
  ts_index::WSet& W = *p.set.W;
  const MaskCtx* mc = p.mc;
  const uint32_t* rep = h->host_status + (size_t)p.slot.slot * TS_SLOT_WORDS;
  prof_mark(h, p.pc, -1, p.s);
  TS_HIP(hipStreamSynchronize(p.s));
  prof_collect(h, p.pc);
  uint32_t maxc = 0;
  for (int i = 0; i < p.nq; ++i) maxc = std::max(maxc, rep[i]);
  const bool redo = rep[64] != 0;
  set_info(h, (redo ? 2 : 1) | (p.fused ? 16 : 0), maxc, p.S, p.m);
  if (mc) add_filter_info(h, p.fseq, rep[65], p.nblk, false);
  if (mc && mc->bias) add_bias_info(h, true, redo, (int64_t)rep[65] + (redo ? p.nblk : 0));
  if (!redo) return TS_OK;
  if (p.fused) {   // (no prepared query image yet; a threshold workgroup that gave up may have left entries behind)
    W.hist_dirty = true;
    TS_CHECK(ts_launch_qprep(h->L, p.dq, p.q_dtype, p.nq, p.qh, (uint4*)W.qimg.p, W.cand_cnt(), W.status(), p.s));
  }
  prof_mark(h, p.pc, 5, p.s);
  TS_CHECK(dense_path(h, W, p.nq, p.qh, p.k, p.out_s, p.out_i, p.s, mc, p.pkg));
  prof_mark(h, p.pc, -1, p.s);
  TS_HIP(hipStreamSynchronize(p.s));
  prof_collect(h, p.pc);
  return TS_OK;
}

// A pass has three phases, each touching one workspace set W:
//   P   query prep, sample scan, thresholds      writes W.qimg, W.sample, W.tau; clears W.cand_cnt
//   S   fused scan+filter over the whole shard   reads W.qimg, W.tau; writes W.cand_*
//   Sel exact top-k of the candidates            reads W.cand_*; writes the caller's outputs + host slot
// Normally all three are enqueued on the caller's stream.  With TS_FLAG_PIPELINE they go to
// three internal streams chained by events (P -> S -> Sel), and the caller's stream only waits
// for Sel: P of the NEXT search and Sel of the PREVIOUS one then run beside the current S, which
// leaves an eighth of the CUs free and is HBM-bound anyway.  Passes alternate between two
// workspace sets; a set is reused only after the Sel that last read it (its ev_sel).
//
// Filtered passes (mc != null) take the five-launch path with the live-block list and the masked scan
// (f16 / bf16 storage), or the dense path with masked selection (fp32 storage, small corpora, large k,
// TS_FLAG_NO_FILTER, fallback).
static int search_pass_on(ts_index* h, SetLease& set, const void* dq, int nq, int q_dtype, int k, float* out_s,
                          int64_t* out_i, uint32_t flags, hipStream_t s, const MaskCtx* mc, int pkg) {
  ts_index::WSet& W = *set.W;
  const int64_t N = h->ntotal;
  const int64_t nblk = (N + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  const int qh = nq > 32 ? 2 : 1;
  int64_t fseq = 0;
  if (mc) {
    // the one-launch kernel has no masked form, and the pipelined schedule is not worth a second copy of it
    flags &= ~(uint32_t)(TS_FLAG_ONE_LAUNCH | TS_FLAG_PIPELINE);
    flags |= TS_FLAG_CLASSIC;
    std::lock_guard<std::mutex> lk(h->mu);
    fseq = h->fseq;
  }
  if (h->L.dtype == TS_FP8_E4M3 || h->L.dtype == TS_MXFP4_E2M1 || pkg) {
    // e4m3 and 4-bit MX storage and the prefix scans have the five-launch kernels only (ts_scan_fp8.hip,
    // ts_scan_prefix.hip): as for a masked pass
    flags &= ~(uint32_t)(TS_FLAG_ONE_LAUNCH | TS_FLAG_PIPELINE);
    flags |= TS_FLAG_CLASSIC;
  }
  // the layout of the pass's query image: the index's, or that of the prefix's dimensions
  const TsLayout QL = pkg ? ts_make_layout(16 * pkg, h->L.dtype) : h->L;
  // (a boosted pass takes the filter path for every k <= kMaxFilterK of a corpus of kMinFilterRows rows: at the floor
  // of both, k = 2048 of 32768 rows, the rank 3 k S / N = 1536 of 8192 sample rows still lies inside the threshold
  // kernel's 4096 kept keys and the ~6 k expected candidates inside the 16384 slots)
  const bool filter = !(flags & TS_FLAG_NO_FILTER) && k <= kMaxFilterK && N >= kMinFilterRows &&
                      (N >= 32 * (int64_t)k || (mc && mc->bias)) && !(mc && h->L.dtype == TS_F32);
  const bool async = (flags & TS_FLAG_ASYNC) != 0;
  const bool pipe = filter && async && (flags & TS_FLAG_PIPELINE) != 0;
  if (pipe) TS_CHECK(ensure_streams(h));
  // ---- one-launch search (ts_fused.hip) whenever its threshold estimate is valid: the sample's 16-row
  // group maxima stand in for the scores, which holds while the wanted rank is far below the group count
  FusedPlan fp{};
  // Where it is taken by default: unpipelined searches of up to kOneLaunchMaxRows rows, the regime in which the three
  // launches it removes are a visible share of the batch (1.25 M x 768: 0.343 vs 0.359 ms per batch back to back,
  // 0.376 vs 0.391 synchronous).  At 10 M rows both paths take 2.27 ms and the plain scan kernel is the cleaner
  // roofline object; pipelined (TS_FLAG_PIPELINE) the five-launch path already hides its preparation under the
  // previous scan and is 3 % ahead (0.335 vs 0.345 ms with the exchange).  TS_FLAG_ONE_LAUNCH forces it anywhere.
  const bool want_fused = (flags & TS_FLAG_ONE_LAUNCH) || (!pipe && N <= kOneLaunchMaxRows);
  const bool fused = filter && !(flags & TS_FLAG_CLASSIC) && want_fused && !ts_use_f32_split(h->L, qh) &&
                     plan_fused(h, N, nblk, k, pipe, &fp);   // (fp32 storage at 32 queries per pass: the split scan, five launches)
  // (the one-launch search has no preparation phase: what remains of "P" rides on the scan stream)
  hipStream_t sP = pipe ? (fused ? h->s_scan : h->s_pro) : s, sS = pipe ? h->s_scan : s, sL = pipe ? h->s_sel : s;
  TS_CHECK(set.wait_previous(sP));
  // the output buffers may be memory the caller's stream is still reading (a recycled
  // allocation): the final phase must not start before the stream's work issued so far
  if (pipe) TS_HIP(hipEventRecord(W.ev_in, s));

  Pass p{h, set, dq, nq, q_dtype, qh, k, pkg, out_s, out_i, mc, N, nblk, fseq, async, pipe, fused, s, sP, sS, sL, {h, -1}};
  p.pc.now = h->profiling && (h->prof_seq.fetch_add(1, std::memory_order_relaxed) % (uint64_t)h->prof_every == 0);
  p.pc.scan_only = async;
  prof_mark(h, p.pc, 0, sP);
  if (!fused) TS_CHECK(ts_launch_qprep(QL, dq, q_dtype, nq, qh, (uint4*)W.qimg.p, W.cand_cnt(), W.status(), sP));
  if (!filter) return pass_dense(p);
  // the report slot: the select kernel writes the candidate counts and the status word into it, a filtered
  // pass's threshold kernel also the live-block count (word 65)
  if (mc) {
    p.slot.slot = alloc_slot(h);
    if (p.slot.slot < 0) { ts_set_error("no free report slot"); return TS_ERR_INVALID; }
    for (int i = 0; i < 66; ++i) h->host_status[(size_t)p.slot.slot * TS_SLOT_WORDS + i] = 0;
  }
  TS_CHECK(ts_buf_ensure(W.cand_score, (size_t)TS_MAX_Q * kCandCap * 4));
  TS_CHECK(ts_buf_ensure(W.cand_id, (size_t)TS_MAX_Q * kCandCap * 4));
  if (fused) TS_CHECK(pass_one_launch(p, fp));
  else TS_CHECK(pass_five_launch(p));
  TS_CHECK(pass_select(p));
  if (!async) return pass_verify(p);
  // verified later, by ts_index_finish(); nothing here waits for the GPU
  std::lock_guard<std::mutex> lk(h->mu);
  ts_index::Pending& pe = push_pending(h, p.slot.slot, nq, p.S, p.m, fused ? (int)(&W - h->ws) : -1, mc ? fseq : -1);
  if (mc) { h->finfo[1] += (fseq == h->fseq) ? nblk : 0; h->finfo[2] += (fseq == h->fseq) ? 1 : 0; }
  if (p.pc.now && p.pc.nev == 2) {  // the scan+filter interval of this pass (prof_mu is held: h->ev is ours)
    pe.e0 = h->ev[0]; pe.e1 = h->ev[1];
    // hand the two events over and give the handle fresh ones
    hipEvent_t n0 = nullptr, n1 = nullptr;
    if (hipEventCreate(&n0) == hipSuccess && hipEventCreate(&n1) == hipSuccess) { h->ev[0] = n0; h->ev[1] = n1; }
    else { pe.e0 = pe.e1 = nullptr; }
  }
  p.slot.handed_over();   // ts_index_finish() frees it
  return TS_OK;
}

// pkg > 0 (ts_index_search_prefix): the pass ranks on the first pkg k groups of every row; dq holds 16 * pkg elements
// per query
static int search_pass(ts_index* h, const void* dq, int nq, int q_dtype, int k, float* out_s,
                       int64_t* out_i, uint32_t flags, hipStream_t s, const MaskCtx* mc = nullptr, int pkg = 0) {
  // per-phase timing shares one set of events per handle: profiled searches run one at a time
  std::unique_lock<std::mutex> plk(h->prof_mu, std::defer_lock);
  if (h->profiling) plk.lock();
  SetLease set(h);
  return search_pass_on(h, set, dq, nq, q_dtype, k, out_s, out_i, flags, s, mc, pkg);
}

// ---- coalesced passes (TS_FLAG_COALESCE)
extern "C" int32_t ts_coalesce_groups(int32_t dim, int32_t storage_dtype) {
  if (dim <= 0 || (storage_dtype != TS_F16 && storage_dtype != TS_BF16)) return 0;
  return ts_scan_multi_groups(ts_make_layout(dim, storage_dtype));
}

extern "C" int32_t ts_coalesce_groups_wide(int32_t dim, int32_t storage_dtype) {
  if (dim <= 0 || (storage_dtype != TS_F16 && storage_dtype != TS_BF16)) return 0;
  return ts_scan_wide_groups(ts_make_layout(dim, storage_dtype));
}

extern "C" int64_t ts_coalesce_wide_min_bytes() { return kWideMinCorpusBytes; }

extern "C" int32_t ts_coalesce_groups_stationary(int32_t dim, int32_t storage_dtype) {
  if (dim <= 0 || (storage_dtype != TS_F16 && storage_dtype != TS_BF16)) return 0;
  return ts_scan_qstat_groups(ts_make_layout(dim, storage_dtype));
}

// Groups per pass of an unfiltered pass of a search with these flags, or 0 where it does not join the pending-pass
// queue: asynchronous, not pipelined, on the five-launch filter path (the one-launch kernel has no multi-group form),
// and at least three groups per pass (at two, one pass per 64-query batch is what the plain scan already does).
// Wide passes where the corpus (padded rows x padded dimension) is larger than kWideMinCorpusBytes and the resident
// passes take at most kWideMaxResidentGroups groups, or where TS_FLAG_WIDE_PASSES asks for them;
// TS_FLAG_NO_WIDE_PASSES keeps the LDS-resident ones.
// Query-stationary passes (scan_qstat_kernel, 8 groups) where their kernel exists for the layout, nothing is removed
// (there is no tombstone form) and either TS_FLAG_STATIONARY_PASSES asks for them or the policy above, left to itself
// (neither wide-pass flag), picks a wide pass; TS_FLAG_NO_STATIONARY_PASSES, and a forced wide-pass flag without
// TS_FLAG_STATIONARY_PASSES, keep the widths above.
static int co_pass_width(const ts_index* h, int k, uint32_t flags) {
  const int64_t N = h->ntotal;
  const int64_t nblk = (N + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  const uint32_t need = TS_FLAG_ASYNC | TS_FLAG_COALESCE;
  if ((flags & need) != need || (flags & (TS_FLAG_PIPELINE | TS_FLAG_NO_FILTER | TS_FLAG_HOST_PTR | TS_FLAG_ONE_LAUNCH)))
    return 0;
  if (k > kMaxFilterK || N < kMinFilterRows || N < 32 * (int64_t)k) return 0;
  if (!(flags & TS_FLAG_CLASSIC) && N <= kOneLaunchMaxRows) return 0;   // the one-launch search's regime
  const int grid = filter_scan_cus(h);
  bool wide = (int64_t)nblk * (int64_t)ts_block_bytes(h->L) > kWideMinCorpusBytes &&
              h->co_gmax <= kWideMaxResidentGroups;
  if (h->co_gstat > 0 && h->nremoved == 0 && !(flags & TS_FLAG_NO_STATIONARY_PASSES) &&
      ts_scan_qstat_fits(nblk, h->num_cus)) {
    const bool auto_wide = wide && !(flags & (TS_FLAG_WIDE_PASSES | TS_FLAG_NO_WIDE_PASSES));
    if ((flags & TS_FLAG_STATIONARY_PASSES) || (kStationaryByDefault && auto_wide)) return h->co_gstat;
  }
  if (flags & TS_FLAG_WIDE_PASSES) wide = true;
  if (flags & TS_FLAG_NO_WIDE_PASSES) wide = false;
  if (wide && h->co_gwide >= 3 && ts_scan_wide_fits(nblk, h->num_cus)) return h->co_gwide;   // (co_launch_pass: every CU)
  if (h->co_gmax >= 3 && ts_scan_multi_fits(nblk, grid)) return h->co_gmax;
  return 0;
}

// the pass's geometry and groups, for MultiScanParams / WideScanParams
template <class P>
static void co_fill_params(const ts_index* h, int G, P& mp) {
  const int64_t N = h->ntotal;
  mp.corpus = h->corpus;
  mp.kg = h->L.kg;
  mp.nwork = (N + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  mp.blk0 = 0;
  mp.blk_stride = 1;
  mp.ntotal = N;
  mp.cand_cap = kCandCap;
  for (int g = 0; g < G; ++g) {
    const ts_index::CoBatch& b = h->co_batch[h->co_group[g].batch];
    const int half = h->co_group[g].half;
    mp.gimg[g] = (const uint4*)b.W->qimg.p;
    mp.gqh[g] = b.qh;
    mp.ghalf[g] = half;
    mp.gtau[g] = b.W->tau() + 32 * half;
    mp.gcnt[g] = b.W->cand_cnt() + 32 * half;
    mp.gscore[g] = (float*)b.W->cand_score.p + (size_t)32 * half * kCandCap;
    mp.gid[g] = (int32_t*)b.W->cand_id.p + (size_t)32 * half * kCandCap;
  }
}

// the dense scan of a batch's sample by scan_kernel (one launch per batch)
static int co_sample_scan(ts_index* h, const ts_index::CoBatch& b, hipStream_t s) {
  ScanParams sp = scan_base(h, *b.W, b.nq);
  scan_window(sp, 0, b.nsb, b.sstride, (float*)b.W->sample.p, b.S);
  return ts_launch_scan(h->L, SCAN_DENSE, b.qh, sp, h->num_cus, s);
}

// The pass prologue: every batch with a group among the G pending ones that has no thresholds yet (a
// batch whose groups straddle two passes gets them with the first) gets its sample scores and thresholds now, on the
// queue's stream, ahead of the filter pass.  Two batches or more: one sample-mode launch of the stationary kernel per
// 8 groups (the sample is read once for all of them) and one threshold launch per kernel ts_launch_tau would pick; a
// single batch keeps scan_kernel's dense scan and its own ts_launch_tau.  Every batch gets the sample buffer and so
// the thresholds of its own launches.  On a failure the batches are marked, and reported for a redo with their pass.
static int co_pass_prologue(ts_index* h, int G) {
  int owed[TS_MAX_WIDE_GROUPS], no = 0;
  for (int g = 0; g < G; ++g) {
    const int bi = h->co_group[g].batch;
    if (!h->co_batch[bi].tau_done && (no == 0 || owed[no - 1] != bi)) owed[no++] = bi;   // (groups are in batch order)
  }
  if (no == 0) return TS_OK;
  hipStream_t s = h->co_stream;
  int st = TS_OK;
  if (no == 1) {
    const ts_index::CoBatch& b = h->co_batch[owed[0]];
    st = co_sample_scan(h, b, s);
    if (st == TS_OK) st = ts_launch_tau((const float*)b.W->sample.p, b.S, (uint32_t)b.S, b.m, b.nq, b.W->tau(), s);
  } else {
    // sample scores: groups of batches with one sample geometry share a launch (in one queue they all have it)
    QstatSampleParams sp{};
    int ng = 0;
    auto flush = [&]() {
      if (ng > 0 && st == TS_OK) st = ts_launch_scan_qstat_sample(h->L, ng, sp, h->num_cus, s);
      ng = 0;
    };
    for (int i = 0; i < no; ++i) {
      const ts_index::CoBatch& b = h->co_batch[owed[i]];
      for (int half = 0; half < b.qh; ++half) {
        if (ng == TS_MAX_WIDE_GROUPS || (ng > 0 && (sp.nwork != b.nsb || sp.blk_stride != b.sstride || sp.dense_ld != b.S)))
          flush();
        if (ng == 0) {
          sp.corpus = h->corpus;
          sp.kg = h->L.kg;
          sp.nwork = b.nsb;
          sp.blk0 = 0;
          sp.blk_stride = b.sstride;
          sp.ntotal = h->ntotal;
          sp.dense_ld = b.S;
        }
        sp.gimg[ng] = (const uint4*)b.W->qimg.p;
        sp.gqh[ng] = b.qh;
        sp.ghalf[ng] = half;
        sp.gnq[ng] = std::min(32, b.nq - 32 * half);
        sp.gdense[ng] = (float*)b.W->sample.p;
        ++ng;
      }
    }
    flush();
    // thresholds: one launch per kernel
    for (int key = 1; key <= 4 && st == TS_OK; key += 3) {
      TauBatch tb{};
      int n = 0;
      for (int i = 0; i < no; ++i) {
        const ts_index::CoBatch& b = h->co_batch[owed[i]];
        if (ts_tau_batch_key(b.m) != key) continue;
        tb.sample[n] = (const float*)b.W->sample.p;
        tb.ld[n] = b.S;
        tb.n[n] = (uint32_t)b.S;
        tb.m[n] = b.m;
        tb.nq[n] = b.nq;
        tb.tau[n] = b.W->tau();
        ++n;
      }
      if (n == 1) st = ts_launch_tau(tb.sample[0], tb.ld[0], tb.n[0], tb.m[0], tb.nq[0], tb.tau[0], s);
      else if (n > 1) st = ts_launch_tau_batch(tb, n, s);
    }
  }
  for (int i = 0; i < no; ++i) {
    h->co_batch[owed[i]].tau_done = true;
    h->co_batch[owed[i]].failed = st != TS_OK;
  }
  return st;
}

// One filter scan over the pending groups; then the select of every batch whose last group was in it.  Groups whose
// images all fit the LDS take scan_multi_kernel, more take scan_wide_kernel, or scan_qstat_kernel in a queue of
// query-stationary passes.  Caller holds co_mu.
static int co_launch_pass(ts_index* h) {
  if (h->co_ngroup == 0) return TS_OK;
  const int G = h->co_ngroup;
  const int64_t N = h->ntotal;
  hipStream_t s = h->co_stream;
  // the sample scores and thresholds its batches still owe (a queue with the pass prologue), ahead of the timed scan
  int st = co_pass_prologue(h, G);
  // per-launch timing of the scan (ts_index_get_timings "filter_scan"), handed to a batch that ends in this pass
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h->profiling && h->co_pass_seq++ % (uint64_t)h->prof_every == 0) {
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, s) != hipSuccess) {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
      e0 = e1 = nullptr;
    }
  }
  // removed rows: the tombstone instantiations (the queue is flushed whenever removals change)
  const bool tomb = h->nremoved > 0;
  // A queue of query-stationary passes (co_pass_width): its full passes and the partial ones of 7 groups take
  // scan_qstat_kernel.  A partial pass that a wide pass can take goes there (6 groups: 3.08 ms against 3.53 ms at
  // 10 M x 768), one the LDS-resident kernel can take goes there, as in a wide queue.  With
  // TS_FLAG_STATIONARY_PASSES every pass above co_gmax groups is a stationary one (tests, A/B runs).
  const int stat_above = h->co_stat_forced ? h->co_gmax : std::max(h->co_gmax, h->co_gwide);
  if (st != TS_OK) {
    // no thresholds: no scan; the pass's batches are reported for a redo below
  } else if (!tomb && h->co_gstat > 0 && h->co_width == h->co_gstat && G > stat_above) {
    // one group per wave, any G up to 8; every CU, like the wide pass
    WideScanParams wp{};
    co_fill_params(h, G, wp);
    wp.stage_cap = ts_scan_qstat_stage_cap(h->L);
    int stat_cus = h->num_cus;
#ifdef TS_TUNING   // A/B only: how many CUs the stationary pass may occupy
    static const int dbg_stat_cus = getenv("TS_QSTAT_CUS") ? atoi(getenv("TS_QSTAT_CUS")) : 0;
    if (dbg_stat_cus > 0) stat_cus = dbg_stat_cus;
#endif
    st = ts_launch_scan_qstat(h->L, G, wp, stat_cus, s);
  } else if (G <= h->co_gmax) {
    MultiTombParams mp{};
    co_fill_params(h, G, mp);
    mp.stage_cap = ts_scan_multi_stage_cap(h->L, G);
    mp.live = (const uint32_t*)h->live.p;
    st = tomb ? ts_launch_scan_multi_tomb(h->L, G, mp, filter_scan_cus(h), s)
              : ts_launch_scan_multi(h->L, G, mp, filter_scan_cus(h), s);
  } else {
    WideTombParams wp{};
    co_fill_params(h, G, wp);
    wp.stage_cap = ts_scan_wide_stage_cap(h->L, G);
    wp.live = (const uint32_t*)h->live.p;
    // every CU: the wide pass is co-bound by the matrix pipe, so the 7/8 of scan_kernel (HBM-bound) gives up 1/8
    // of its MFMA throughput (3.53-3.54 against 3.72-3.79 ms per 6-group pass at 10 M x 768).  The
    // free eighth serves the one-launch search's threshold workgroups and pipelined neighbours; a coalesced pass has
    // neither (co_pass_width), and its selects follow it on this stream.
    int wide_cus = h->num_cus;
#ifdef TS_TUNING   // A/B only: how many CUs the wide pass may occupy
    static const int dbg_wide_cus = getenv("TS_WIDE_CUS") ? atoi(getenv("TS_WIDE_CUS")) : 0;
    if (dbg_wide_cus > 0) wide_cus = dbg_wide_cus;
#endif
    st = tomb ? ts_launch_scan_wide_tomb(h->L, G, wp, wide_cus, s) : ts_launch_scan_wide(h->L, G, wp, wide_cus, s);
  }
  if (e0 && (st != TS_OK || hipEventRecord(e1, s) != hipSuccess)) {
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    e0 = e1 = nullptr;
  }
  for (int g = 0; g < G; ++g) --h->co_batch[h->co_group[g].batch].groups_left;
  h->co_ngroup = 0;
  // the selects of the finished batches, in submission order; unfinished ones move to the front
  int keep = 0, nfin = 0;
  const int nb = h->co_nbatch;
  ts_index::CoBatch fin[TS_MAX_WIDE_GROUPS];
  for (int i = 0; i < nb; ++i) {
    const ts_index::CoBatch b = h->co_batch[i];
    if (b.groups_left > 0) h->co_batch[keep++] = b;
    else fin[nfin++] = b;
  }
  auto sel_params = [&](const ts_index::CoBatch& b) {   // (tomb: need_check_kernel, min(k, live rows))
    return cand_select_params(h, *b.W, b.k, tomb ? 0u : (uint32_t)std::min<int64_t>(b.k, N), b.out_s, b.out_i, b.slot);
  };
  // A queue with the pass prologue: the selects of the pass in one launch (select_batch_kernel), where
  // ts_launch_select would give the batches the same LDS; a batch that differs keeps a launch of its own below.
  bool launched[TS_MAX_WIDE_GROUPS] = {};
  if (h->co_prologue && !tomb && st == TS_OK && nfin >= 2) {
    SelBatch sb{};
    int idx[TS_MAX_WIDE_GROUPS], n = 0;
    uint32_t key0 = 0;
    for (int i = 0; i < nfin && st == TS_OK; ++i) {
      if (fin[i].failed) continue;
      const SelParams p = sel_params(fin[i]);
      uint32_t key = 0;
      if (ts_select_batch_key(p, &key) != TS_OK) continue;   // (its own launch reports the error)
      if (n == 0) key0 = key;
      if (key != key0) continue;
      sb.p[n] = p;
      sb.nq[n] = fin[i].nq;
      idx[n++] = i;
    }
    if (n >= 2) {
      st = ts_launch_select_batch(sb, n, s);
      for (int j = 0; j < n; ++j) launched[idx[j]] = true;
    }
  }
  for (int i = 0; i < nfin; ++i) {
    const ts_index::CoBatch& b = fin[i];
    bool ok = st == TS_OK && !b.failed;
    if (ok) {
      if (!launched[i]) {
        const SelParams p = sel_params(b);
        if (tomb) st = ts_launch_need_check(b.W->cand_cnt(), b.W->mask_dev()->need, b.nq, b.W->status(), p.host_report, s);
        if (st == TS_OK) st = ts_launch_select(p, b.nq, s);
      }
      if (st == TS_OK) {
        if (hipEventRecord(b.W->ev_sel, s) == hipSuccess) b.W->used = true;   // (the set's next user waits for it)
        else { ts_set_error("hipEventRecord failed"); st = TS_ERR_HIP; }
      }
      ok = st == TS_OK;
    }
    if (!ok) {
      // nothing verifies a batch whose select is missing: finish() must report it for a redo
      h->host_status[(size_t)b.slot * TS_SLOT_WORDS + 64] = TS_STATUS_OVERFLOW;
    }
    if (e0) {
      std::lock_guard<std::mutex> lk(h->mu);
      for (int j = 0; j < h->npending; ++j)
        if (h->pending[j].slot == b.slot) { h->pending[j].e0 = e0; h->pending[j].e1 = e1; e0 = e1 = nullptr; break; }
    }
    release_set(h, b.W);
  }
  if (e0) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); }
  h->co_nbatch = keep;
  // the end of this pass and its selects, for work that later arrives on another stream (co_flush_locked)
  if (hipEventRecord(h->co_ev, s) != hipSuccess) {
    (void)hipStreamSynchronize(s);   // no event: nothing of this pass may be left running behind a later wait
    h->co_ev_live = false;
    if (st == TS_OK) { ts_set_error("hipEventRecord failed"); st = TS_ERR_HIP; }
  } else {
    h->co_ev_live = true;
  }
  return st;
}

// Enqueue every held batch: the pending groups make a (partial) pass, which holds the last group of every held
// batch (co_submit queues all groups of a batch before it returns).  Then `s` is ordered behind every pass and
// select enqueued so far on the queue's stream, so that work the caller puts on `s` next — a search, an add, the
// sync of ts_index_finish — sees them, as it saw an unheld search that was enqueued before it.  Caller holds co_mu.
static int co_flush_locked(ts_index* h, hipStream_t s) {
  const int st = co_launch_pass(h);
  if (h->co_ev_live && s != h->co_stream) {
    // (asked first: a wait on another stream's event, even a satisfied one, costs the waiting stream 10-20 us)
    if (hipEventQuery(h->co_ev) == hipSuccess) h->co_ev_live = false;
    else TS_HIP(hipStreamWaitEvent(s, h->co_ev, 0));
  }
  return st;
}

static int co_flush(ts_index* h, hipStream_t s) {
  std::lock_guard<std::mutex> lk(h->co_mu);
  return co_flush_locked(h, s);
}

// One coalesced batch of <= 64 queries: query prep on the caller's stream now (it reads the caller's queries), then
// the sample scan and the thresholds, or with the queue's pass prologue neither (they read only the set's own image
// and sample buffer: co_pass_prologue); its groups into the pending-pass queue.  Caller holds co_mu; the stream is the
// queue's.
static int co_submit(ts_index* h, const void* dq, int nq, int q_dtype, int k, float* out_s, int64_t* out_i,
                     hipStream_t s) {
  const int qh = nq > 32 ? 2 : 1;
  // the pass prologue: the sample scan and the thresholds read only the set's own image and sample buffer, and go in
  // front of the batch's first pass (co_pass_prologue)
  const bool defer = h->co_prologue && h->nremoved == 0;
  SetLease set(h);   // (at most co_width - 1 < TS_NSETS sets are held by the queue here)
  ts_index::WSet* W = set.W;
  SlotGuard slot_guard(h, alloc_slot(h));
  if (slot_guard.slot < 0) { ts_set_error("no free report slot"); return TS_ERR_INVALID; }
  TS_CHECK(set.wait_previous(s));
  TS_CHECK(ts_launch_qprep(h->L, dq, q_dtype, nq, qh, (uint4*)W->qimg.p, W->cand_cnt(), W->status(), s));
  TS_CHECK(ts_buf_ensure(W->cand_score, (size_t)TS_MAX_Q * kCandCap * 4));
  TS_CHECK(ts_buf_ensure(W->cand_id, (size_t)TS_MAX_Q * kCandCap * 4));
  // the five-launch geometry with a lower survivor target: three groups share the staging area that two have in
  // scan_kernel (ts_scan.hip, scan_multi_kernel)
  const SampleGeom g = sample_geometry(h, k, kCoalesceOversample);
  TS_CHECK(ts_buf_ensure(W->sample, (size_t)nq * g.S * 4));
  ts_index::CoBatch cb{W, nq, qh, k, slot_guard.slot, qh, out_s, out_i, g.m, g.S, g.sstride, g.nsb, !defer, false};
  if (defer) {
    // (co_pass_prologue)
  } else if (h->nremoved > 0) {
    // removed rows: the thresholds of the filtered path (tau_masked_kernel) with the live words as the
    // batch's one mask: the m_q-th best LIVE sample score with N_q = the live rows; need[q] = min(k, live rows)
    TS_CHECK(co_sample_scan(h, cb, s));
    MaskCtx live{};
    live.bits = (const uint32_t*)h->live.p;
    live.words = (h->ntotal + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;   // one word per row block
    const int32_t mask0[TS_MAX_Q] = {};
    build_mask_pass(mask0, nq, live.mp);
    TS_CHECK(launch_live_blocks(h, *W, live, s));
    TS_CHECK(ts_launch_tau_masked((const float*)W->sample.p, g.S, g.sstride, h->ntotal, live.bits, live.words,
                                  W->mask_dev(), nq, k, (uint32_t)kCoalesceOversample, kMinSampleRank, W->tau(), nullptr,
                                  s));
  } else {
    TS_CHECK(co_sample_scan(h, cb, s));
    TS_CHECK(ts_launch_tau((const float*)W->sample.p, g.S, (uint32_t)g.S, g.m, nq, W->tau(), s));
  }
  uint32_t* rep = h->host_status + (size_t)slot_guard.slot * TS_SLOT_WORDS;
  for (int i = 0; i < 65; ++i) rep[i] = 0;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    push_pending(h, slot_guard.slot, nq, g.S, g.m, -1, -1);
  }
  h->co_batch[h->co_nbatch++] = cb;
  slot_guard.handed_over();
  set.detach();   // released by co_launch_pass once its select is enqueued
  int st = TS_OK;
  for (int half = 0; half < qh; ++half) {
    h->co_group[h->co_ngroup++] = ts_index::CoGroup{h->co_nbatch - 1, half};
    if (h->co_ngroup == h->co_width) {
      const int s1 = co_launch_pass(h);
      if (st == TS_OK) st = s1;
    }
  }
  return st;
}

extern "C" int ts_index_flush(ts_index* h, void* stream) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  TsDeviceGuard g(h->device);
  std::lock_guard<std::mutex> lk(h->co_mu);
  return co_flush_locked(h, (hipStream_t)stream);   // later work on `stream` is ordered behind the flushed passes
}

// TS_FLAG_ASYNC: a call takes at most 4 passes, and at most a quarter of the report slots hold unfinished passes
static int admit_async(ts_index* h, int nq, int qp, hipStream_t s) {
  const int passes = (nq + qp - 1) / qp;
  if (passes > 4) { ts_set_error("TS_FLAG_ASYNC: at most %d queries per call", 4 * qp); return TS_ERR_INVALID; }
  bool full = false;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    full = h->npending + passes > TS_ASYNC_SLOTS / 4;
  }
  if (!full) return TS_OK;
  (void)co_flush(h, s);   // nothing stays held behind the error (a filtered search has flushed already)
  ts_set_error("too many unfinished asynchronous searches; call ts_index_finish()");
  return TS_ERR_INVALID;
}

namespace {
// The device side of a call's queries, masks and results: the caller's own pointers, or with TS_FLAG_HOST_PTR the
// handle's one staging area, held under host_mu until the call ends.
struct CallBuffers {
  ts_index* h;
  std::unique_lock<std::mutex> lk;
  explicit CallBuffers(ts_index* h_) : h(h_), lk(h_->host_mu, std::defer_lock) {}
  const void* dq = nullptr;
  const uint32_t* bits = nullptr;
  float* ds = nullptr;
  int64_t* di = nullptr;
  // mbytes == 0: no masks; nout == 0: no results of nout scores and ids
  int in(bool host, const void* queries, size_t qbytes, const uint32_t* allow_bits, size_t mbytes,
         float* out_scores, int64_t* out_ids, size_t nout, hipStream_t s) {
    dq = queries;
    bits = allow_bits;
    ds = out_scores;
    di = out_ids;
    if (!host) return TS_OK;
    lk.lock();
    TS_CHECK(ts_buf_ensure(h->qstage, qbytes));
    if (nout) {
      TS_CHECK(ts_buf_ensure(h->out_s, nout * 4));
      TS_CHECK(ts_buf_ensure(h->out_i, nout * 8));
      ds = (float*)h->out_s.p;
      di = (int64_t*)h->out_i.p;
    }
    TS_HIP(hipMemcpyAsync(h->qstage.p, queries, qbytes, hipMemcpyHostToDevice, s));
    dq = h->qstage.p;
    if (mbytes) {
      TS_CHECK(ts_buf_ensure(h->mstage, mbytes));
      TS_HIP(hipMemcpyAsync(h->mstage.p, allow_bits, mbytes, hipMemcpyHostToDevice, s));
      bits = (const uint32_t*)h->mstage.p;
    }
    return TS_OK;
  }
  // the results back to the caller's host arrays; returns with the stream drained
  int out(float* out_scores, int64_t* out_ids, size_t nout, hipStream_t s) {
    if (!lk.owns_lock()) return TS_OK;
    TS_HIP(hipMemcpyAsync(out_scores, ds, nout * 4, hipMemcpyDeviceToHost, s));
    TS_HIP(hipMemcpyAsync(out_ids, di, nout * 8, hipMemcpyDeviceToHost, s));
    TS_HIP(hipStreamSynchronize(s));
    return TS_OK;
  }
};

// Removed rows: every mask of a filtered call is ANDed with the tombstone bitmap on the device, and a
// query without a mask gets the bitmap itself, so the call is the filtered call of the live rows.  The masks go to
// h->eff, one call at a time: eff_mu is held until the call ends, and done() records eff_ev behind the call's passes.
struct LiveMasks {
  ts_index* h;
  std::unique_lock<std::mutex> lk;
  std::vector<int32_t> moq;
  explicit LiveMasks(ts_index* h_) : h(h_), lk(h_->eff_mu, std::defer_lock) {}
  int apply(int nq, const uint32_t*& bits, int64_t& allow_words, int32_t& n_masks,
            const int32_t*& mask_of_query, hipStream_t s) {
    if (h->nremoved == 0) return TS_OK;
    const int64_t need_words = (h->ntotal + 31) / 32;
    lk.lock();
    TS_CHECK(ts_buf_ensure(h->eff, (size_t)(n_masks + 1) * (size_t)need_words * 4));
    if (h->eff_used) TS_HIP(hipStreamWaitEvent(s, h->eff_ev, 0));   // the previous call's passes have read `eff`
    TS_CHECK(ts_launch_and_live(bits, allow_words, n_masks, (const uint32_t*)h->live.p, need_words,
                                (uint32_t*)h->eff.p, s));
    moq.assign(mask_of_query, mask_of_query + nq);
    for (int32_t& m : moq)
      if (m < 0) m = n_masks;
    mask_of_query = moq.data();
    bits = (const uint32_t*)h->eff.p;
    allow_words = need_words;
    n_masks += 1;
    return TS_OK;
  }
  int done(hipStream_t s) {
    if (!lk.owns_lock()) return TS_OK;
    TS_HIP(hipEventRecord(h->eff_ev, s));
    h->eff_used = true;
    return TS_OK;
  }
  // the same record behind a call that has failed, which keeps its own error text
  void done_after_failure(hipStream_t s) {
    if (lk.owns_lock() && hipEventRecord(h->eff_ev, s) == hipSuccess) h->eff_used = true;
  }
};
}  // namespace

extern "C" int ts_index_search(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype,
                               int32_t k, float* out_scores, int64_t* out_ids, uint32_t flags,
                               void* stream) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  if (nq == 0) return TS_OK;
  if (!queries || !out_scores || !out_ids || nq < 0 || k <= 0 || !dtype_ok(q_dtype)) {
    ts_set_error("bad arguments to search");
    return TS_ERR_INVALID;
  }
  if (h->ntotal == 0) return err_empty();
  if (h->nremoved > 0 && !co_pass_width(h, k, flags)) {
    // removed rows: the filtered search whose only mask is the tombstone bitmap; a search that
    // joins the coalesced passes takes their tombstone form instead (co_submit, co_launch_pass)
    std::vector<int32_t> moq((size_t)nq, -1);
    return ts_index_search_filtered(h, queries, nq, q_dtype, k, nullptr, 0, 0, moq.data(), out_scores, out_ids, flags,
                                    stream);
  }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int qp = queries_per_pass(h);
  if ((flags & TS_FLAG_PIPELINE) && !(flags & TS_FLAG_ASYNC)) {
    ts_set_error("TS_FLAG_PIPELINE needs TS_FLAG_ASYNC");
    return TS_ERR_INVALID;
  }
  if (flags & TS_FLAG_ASYNC) {
    if (flags & TS_FLAG_HOST_PTR) { ts_set_error("TS_FLAG_ASYNC needs device pointers"); return TS_ERR_INVALID; }
    TS_CHECK(admit_async(h, nq, qp, s));
  }
  const size_t qrow = (size_t)h->L.dim * dtype_size(q_dtype);
  if (const int width = co_pass_width(h, k, flags)) {
    std::lock_guard<std::mutex> lk(h->co_mu);
    // the queue holds one stream's batches: moving it to `s` flushes it and orders `s` behind the old stream's passes
    if (h->co_stream != s) TS_CHECK(co_flush_locked(h, s));
    // and passes of one width: a search that asks for another one flushes the pending groups first
    // and one setting of the pass prologue: stationary queues without removed rows, unless the search declines it
    const bool prologue = width == h->co_gstat && h->nremoved == 0 && !(flags & TS_FLAG_NO_PASS_PROLOGUE);
    if (h->co_ngroup > 0 && (h->co_width != width || h->co_prologue != prologue)) TS_CHECK(co_flush_locked(h, s));
    h->co_stream = s;
    h->co_width = width;
    h->co_prologue = prologue;
    h->co_stat_forced = (flags & TS_FLAG_STATIONARY_PASSES) != 0;
    for (int q0 = 0; q0 < nq; q0 += qp) {
      const int c = std::min(qp, nq - q0);
      TS_CHECK(co_submit(h, (const char*)queries + (size_t)q0 * qrow, c, q_dtype, k, out_scores + (size_t)q0 * k,
                         out_ids + (size_t)q0 * k, s));
    }
    std::lock_guard<std::mutex> lk2(h->mu);
    ++h->next_ticket;
    return TS_OK;
  }
  TS_CHECK(co_flush(h, s));   // a search that cannot join the queue runs after the held ones
  CallBuffers b(h);
  TS_CHECK(b.in((flags & TS_FLAG_HOST_PTR) != 0, queries, (size_t)nq * qrow, nullptr, 0, out_scores, out_ids,
                (size_t)nq * k, s));
  for (int q0 = 0; q0 < nq; q0 += qp) {
    const int c = std::min(qp, nq - q0);
    TS_CHECK(search_pass(h, (const char*)b.dq + (size_t)q0 * qrow, c, q_dtype, k, b.ds + (size_t)q0 * k,
                         b.di + (size_t)q0 * k, flags, s));
  }
  if (flags & TS_FLAG_ASYNC) {
    std::lock_guard<std::mutex> lk(h->mu);
    ++h->next_ticket;
  }
  return b.out(out_scores, out_ids, (size_t)nq * k, s);
}

// Filtered search (include/tristage.h): ts_index_search restricted, per query, to the rows of one of
// n_masks bitmaps.  A pass whose queries have no mask is an ordinary ts_index_search pass.
// pdims > 0: ts_index_search_prefix, the same call ranked on the first pdims dimensions (queries of pdims elements)
static int search_filtered_impl(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t k,
                                const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks,
                                const int32_t* mask_of_query, float* out_scores, int64_t* out_ids,
                                uint32_t flags, void* stream, int pdims, const float* bias = nullptr,
                                const float* bias_tail = nullptr) {
  // the checks that need no handle come first (and none of them touches the GPU)
  if (nq < 0 || k <= 0 || !dtype_ok(q_dtype) || (nq > 0 && (!queries || !out_scores || !out_ids))) {
    ts_set_error("bad arguments to search_filtered");
    return TS_ERR_INVALID;
  }
  TS_CHECK(check_mask_args("search_filtered", nq, allow_bits, allow_words, n_masks, mask_of_query));
  if (nq > 0 && !mask_of_query) { ts_set_error("search_filtered: mask_of_query is null"); return TS_ERR_INVALID; }
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  const int64_t N = h->ntotal;
  TS_CHECK(check_mask_words("search_filtered", n_masks, allow_words, N));
  if ((flags & TS_FLAG_PIPELINE) && !(flags & TS_FLAG_ASYNC)) {
    ts_set_error("TS_FLAG_PIPELINE needs TS_FLAG_ASYNC");
    return TS_ERR_INVALID;
  }
  if ((flags & TS_FLAG_ASYNC) && (flags & TS_FLAG_HOST_PTR)) {
    ts_set_error("TS_FLAG_ASYNC needs device pointers");
    return TS_ERR_INVALID;
  }
  if (nq == 0) return TS_OK;
  if (N == 0) return err_empty();
  {
    std::lock_guard<std::mutex> lk(h->mu);
    ++h->fseq;
    for (int i = 0; i < 4; ++i) h->finfo[i] = 0;
  }
  bool any = false;
  for (int32_t q = 0; q < nq && !any; ++q) any = mask_of_query[q] >= 0;
  if (!any && h->nremoved == 0 && !pdims && !bias)
    return ts_index_search(h, queries, nq, q_dtype, k, out_scores, out_ids, flags, stream);
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));   // a filtered search never joins a coalesced pass
  const int qp = queries_per_pass(h);
  if (flags & TS_FLAG_ASYNC) TS_CHECK(admit_async(h, nq, qp, s));
  const size_t qrow = (size_t)(pdims ? pdims : h->L.dim) * dtype_size(q_dtype);
  CallBuffers b(h);
  TS_CHECK(b.in((flags & TS_FLAG_HOST_PTR) != 0, queries, (size_t)nq * qrow, allow_bits,
                (size_t)n_masks * (size_t)allow_words * 4, out_scores, out_ids, (size_t)nq * k, s));
  LiveMasks eff(h);
  TS_CHECK(eff.apply(nq, b.bits, allow_words, n_masks, mask_of_query, s));
  for (int q0 = 0; q0 < nq; q0 += qp) {
    const int c = std::min(qp, nq - q0);
    MaskCtx mc{};
    mc.bits = b.bits;
    mc.words = allow_words;
    mc.bias = bias;
    mc.bias_tail = bias_tail;
    // (a boosted pass always takes the masked path)
    const bool masked = build_mask_pass(mask_of_query + q0, c, mc.mp) || bias != nullptr;
    // A boosted pass none of whose queries has a mask still takes the masked scan, whose unmasked queries read word 0
    // of "mask 0" and OR all ones into it (WalkLive): the pointer has to be readable on the device, whatever the caller
    // left in allow_bits (with n_masks == 0 it is not staged and may be a host address or anything else).  The padded
    // tail of the bias is.
    if (bias && mc.mp.nd == 0) mc.bits = reinterpret_cast<const uint32_t*>(bias_tail);
    TS_CHECK(search_pass(h, (const char*)b.dq + (size_t)q0 * qrow, c, q_dtype, k, b.ds + (size_t)q0 * k,
                         b.di + (size_t)q0 * k, flags, s, masked ? &mc : nullptr, pdims / 16));
  }
  TS_CHECK(eff.done(s));
  if (flags & TS_FLAG_ASYNC) {
    std::lock_guard<std::mutex> lk(h->mu);
    ++h->next_ticket;
  }
  return b.out(out_scores, out_ids, (size_t)nq * k, s);
}

extern "C" int ts_index_search_filtered(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t k,
                                        const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks,
                                        const int32_t* mask_of_query, float* out_scores, int64_t* out_ids,
                                        uint32_t flags, void* stream) {
  return search_filtered_impl(h, queries, nq, q_dtype, k, allow_bits, allow_words, n_masks, mask_of_query, out_scores,
                              out_ids, flags, stream, 0);
}

// ---- funnel search (include/tristage.h "funnel search")
namespace {
constexpr int kFunnelMaxK = 16384;                   // the select kernels hold 16384 keys in LDS
constexpr size_t kRescoreScratchCap = 384u << 20;    // candidate tiles, scores and ids of one chunk of queries
}  // namespace

static int funnel_storage_ok(const ts_index* h, const char* what) {
  if (h->L.dtype == TS_F16 || h->L.dtype == TS_BF16) return TS_OK;
  if (h->L.dtype == TS_MXFP4_E2M1) { ts_set_error("%s is not supported on a 4-bit MX (mxfp4) index", what); return TS_ERR_UNSUPPORTED; }
  ts_set_error("%s takes f16 / bf16 storage only", what);
  return TS_ERR_UNSUPPORTED;
}

extern "C" int ts_index_search_prefix(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t dims,
                                      int32_t k, const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks,
                                      const int32_t* mask_of_query, float* out_scores, int64_t* out_ids,
                                      uint32_t flags, void* stream) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  if (flags & ~(uint32_t)(TS_FLAG_HOST_PTR | TS_FLAG_NO_FILTER)) {
    ts_set_error("search_prefix: flags 0x%x (only TS_FLAG_HOST_PTR and TS_FLAG_NO_FILTER are accepted)", flags);
    return TS_ERR_INVALID;
  }
  if (nq < 0 || k < 1 || k > kFunnelMaxK) {
    ts_set_error("search_prefix: nq = %d, k = %d (k must be in 1 .. %d)", nq, k, kFunnelMaxK);
    return TS_ERR_INVALID;
  }
  TS_CHECK(funnel_storage_ok(h, "search_prefix"));
  if (dims < 128 || dims % 128 != 0 || dims >= h->L.dim) {
    ts_set_error("search_prefix: dims = %d must be a multiple of 128 in [128, %d)", dims, h->L.dim);
    return TS_ERR_INVALID;
  }
  std::vector<int32_t> none;
  if (!mask_of_query && nq > 0) {
    none.assign((size_t)nq, -1);
    mask_of_query = none.data();
  }
  return search_filtered_impl(h, queries, nq, q_dtype, k, allow_bits, allow_words, n_masks, mask_of_query, out_scores,
                              out_ids, flags, stream, dims);
}

// ---- boosted search (include/tristage.h "boosted search")
// The filtered search on score + bias[row]: every pass takes the masked path (live-block list, thresholds on boosted
// sample scores, the biased masked scan of ts_scan_bias.hip) or the dense path with the bias added to each chunk.
extern "C" int ts_index_search_biased(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t k,
                                      const float* bias, int64_t bias_rows, const uint32_t* allow_bits,
                                      int64_t allow_words, int32_t n_masks, const int32_t* mask_of_query,
                                      float* out_scores, int64_t* out_ids, uint32_t flags, void* stream) {
  // the checks that need no handle come first; none of the checks touches the GPU
  if (flags & ~(uint32_t)(TS_FLAG_HOST_PTR | TS_FLAG_NO_FILTER)) {
    ts_set_error("search_biased: flags 0x%x (only TS_FLAG_HOST_PTR and TS_FLAG_NO_FILTER are accepted)", flags);
    return TS_ERR_INVALID;
  }
  if (nq < 0 || k < 1 || k > kFunnelMaxK || !dtype_ok(q_dtype)) {
    ts_set_error("search_biased: nq = %d, k = %d (k must be in 1 .. %d), query dtype %d", nq, k, kFunnelMaxK, q_dtype);
    return TS_ERR_INVALID;
  }
  if (!bias || (nq > 0 && (!queries || !out_scores || !out_ids))) {
    ts_set_error("search_biased: null queries, bias or outputs");
    return TS_ERR_INVALID;
  }
  TS_CHECK(check_mask_args("search_biased", nq, allow_bits, allow_words, n_masks, mask_of_query));
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  TS_CHECK(funnel_storage_ok(h, "search_biased"));
  const int64_t N = h->ntotal;
  if (bias_rows < N) {
    ts_set_error("search_biased: bias_rows = %lld < ntotal = %lld", (long long)bias_rows, (long long)N);
    return TS_ERR_INVALID;
  }
  TS_CHECK(check_mask_words("search_biased", n_masks, allow_words, N));
  const bool host = (flags & TS_FLAG_HOST_PTR) != 0;
  if (host) {
    for (int64_t r = 0; r < N; ++r) {
      if (!std::isfinite(bias[r])) {
        ts_set_error("search_biased: bias[%lld] is not finite", (long long)r);
        return TS_ERR_INVALID;
      }
    }
  } else if (reinterpret_cast<uintptr_t>(bias) % 16 != 0) {
    ts_set_error("search_biased: a device bias must be 16-byte aligned");
    return TS_ERR_INVALID;
  }
  std::lock_guard<std::mutex> blk(h->bias_mu);
  {
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < 4; ++i) h->binfo[i] = 0;
  }
  if (nq == 0) return TS_OK;
  if (N == 0) return err_empty();
  std::vector<int32_t> none;
  if (!mask_of_query) {
    none.assign((size_t)nq, -1);
    mask_of_query = none.data();
  }
  const float* dbias = bias;
  float* tail = nullptr;
  {
    // bias_stage: [0, 32) the padded entries of the last, partial row block; from float 32 on the staged copy of a
    // host array.  Written in stream order; the call returns with the stream drained, so the next call may reuse it.
    TsDeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    TS_CHECK(co_flush(h, s));   // held coalesced passes first, then the call's own work
    const int64_t full = N / TS_ROWS_PER_BLOCK * TS_ROWS_PER_BLOCK;
    TS_CHECK(ts_buf_ensure(h->bias_stage, (size_t)(TS_ROWS_PER_BLOCK + (host ? N : 0)) * 4));
    tail = (float*)h->bias_stage.p;
    if (host) {
      TS_HIP(hipMemcpyAsync(tail + TS_ROWS_PER_BLOCK, bias, (size_t)N * 4, hipMemcpyHostToDevice, s));
      dbias = tail + TS_ROWS_PER_BLOCK;
    }
    TS_HIP(hipMemsetAsync(tail, 0, TS_ROWS_PER_BLOCK * 4, s));
    if (N > full) TS_HIP(hipMemcpyAsync(tail, dbias + full, (size_t)(N - full) * 4, hipMemcpyDeviceToDevice, s));
  }
  return search_filtered_impl(h, queries, nq, q_dtype, k, allow_bits, allow_words, n_masks, mask_of_query, out_scores,
                              out_ids, flags, stream, 0, dbias, tail);
}

extern "C" int ts_index_last_bias_info(const ts_index* h, int64_t info[4]) {
  if (!h || !info) { ts_set_error("bad arguments"); return TS_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(const_cast<ts_index*>(h)->mu);
  for (int i = 0; i < 4; ++i) info[i] = h->binfo[i];
  return TS_OK;
}

// Exact scores of given candidates: gather (ts_mmr.hip) -> one wave per 32-candidate tile against the pass's query
// image (ts_rescore.hip) -> the select, which orders by (score desc, id asc) and drops the entries marked invalid.
extern "C" int ts_index_rescore(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, const int64_t* cand_ids,
                                int32_t ncand, int32_t k, float* out_scores, int64_t* out_ids, void* stream) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  if (nq < 0 || !dtype_ok(q_dtype) || ncand < 1 || ncand > kFunnelMaxK || k < 1 || k > ncand) {
    ts_set_error("rescore: nq = %d, ncand = %d (1 .. %d), k = %d (1 .. ncand)", nq, ncand, kFunnelMaxK, k);
    return TS_ERR_INVALID;
  }
  if (nq > 0 && (!queries || !cand_ids || !out_scores || !out_ids)) { ts_set_error("rescore: null pointer"); return TS_ERR_INVALID; }
  TS_CHECK(funnel_storage_ok(h, "rescore"));
  if (nq == 0) return TS_OK;
  if (h->ntotal == 0) return err_empty();
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));
  TsMmrSource src;
  src.corpus = h->corpus;
  src.L = h->L;
  src.ntotal = h->ntotal;
  src.id_offset = h->id_offset;
  src.live = h->nremoved > 0 ? (const uint32_t*)h->live.p : nullptr;
  src.ivf = false;
  src.id2slot = nullptr;
  src.blk_valid = nullptr;
  const int C = ncand, cbp = (C + 31) / 32;
  const size_t tile_b = (size_t)cbp * h->L.kg * 1024, v_b = (size_t)cbp * 32 * 4, s_b = (size_t)C * 4, i_b = (size_t)C * 8;
  const size_t per_q = tile_b + v_b + i_b + ((s_b + 15) & ~(size_t)15);
  const int qp = queries_per_pass(h);   // (one query image)
  const int qc = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(nq, qp), kRescoreScratchCap / per_q));
  const size_t qrow = (size_t)h->L.dim * dtype_size(q_dtype);
  std::lock_guard<std::mutex> rlk(h->rescore_mu);   // one scratch per handle; the call ends with the stream drained
  TS_CHECK(ts_buf_ensure(h->rescore_scratch, per_q * qc));
  char* base = (char*)h->rescore_scratch.p;
  uint4* tile = (uint4*)base;
  int64_t* ids = (int64_t*)(base + tile_b * qc);
  int32_t* valid = (int32_t*)(base + (tile_b + i_b) * qc);
  float* sc = (float*)(base + (tile_b + i_b + v_b) * qc);
  auto pass = [&](int q0) -> int {
    const int c = std::min(qp, nq - q0);
    const int qh = c > 32 ? 2 : 1;
    SetLease set(h);
    ts_index::WSet* W = set.W;
    TS_CHECK(set.wait_previous(s));
    TS_CHECK(ts_launch_qprep(h->L, (const char*)queries + (size_t)q0 * qrow, q_dtype, c, qh, (uint4*)W->qimg.p, nullptr,
                             nullptr, s));
    for (int c0 = 0; c0 < c; c0 += qc) {
      const int n = std::min(qc, c - c0);
      const int64_t* cid = cand_ids + (size_t)(q0 + c0) * C;
      TS_CHECK(ts_launch_gather_tiles(src, cid, C, cbp, n, tile, valid, s));
      TsRescoreParams rp{};
      rp.tile = tile; rp.valid = valid; rp.ids = cid;
      rp.qimg = (const uint4*)W->qimg.p;
      rp.kg = h->L.kg; rp.qh = qh; rp.C = C; rp.cbp = cbp; rp.col0 = c0;
      rp.scores = sc; rp.ids_out = ids;
      TS_CHECK(ts_launch_rescore(h->L, rp, n, s));
      SelParams p{};
      p.mode = SEL_MERGE64;   // the tiebreak is the real id; an entry whose id is -1 has no rank
      p.scores = sc;
      p.ids64 = ids;
      p.stride = C;
      p.n = (uint32_t)C;
      p.k = k;
      p.out_scores = out_scores + (size_t)(q0 + c0) * k;
      p.out_ids64 = out_ids + (size_t)(q0 + c0) * k;
      p.out_stride = k;
      TS_CHECK(ts_launch_select(p, n, s));
    }
    return set.done(s);
  };
  int st = TS_OK;
  for (int q0 = 0; q0 < nq && st == TS_OK; q0 += qp) st = pass(q0);
  if (st != TS_OK) { (void)hipStreamSynchronize(s); return st; }
  TS_HIP(hipStreamSynchronize(s));
  return TS_OK;
}

extern "C" int ts_index_last_filter_info(const ts_index* h, int64_t info[4]) {
  if (!h || !info) { ts_set_error("bad arguments"); return TS_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(const_cast<ts_index*>(h)->mu);
  for (int i = 0; i < 4; ++i) info[i] = h->finfo[i];
  return TS_OK;
}

// ---- range search (include/tristage.h "range search")
namespace {
constexpr int64_t kRangeDefaultMax = 1ll << 26;   // entries (12 bytes each) a call may return by default
struct RangeStats { int64_t passes = 0, filter_passes = 0, dense_redo = 0; };
}  // namespace

// The result buffers hold `need` entries, of which the first `have` are kept.
static int range_reserve(ts_index* h, int64_t need, int64_t have, int64_t limit, hipStream_t s) {
  if (need <= h->rng_cap) return TS_OK;
  int64_t cap = std::max<int64_t>(need, std::min<int64_t>(limit, 2 * h->rng_cap));
  cap = std::max<int64_t>(cap, 1 << 16);
  TsDevBuf ns, ni;
  int st = ts_buf_ensure(ns, (size_t)cap * 4);
  if (st == TS_OK) st = ts_buf_ensure(ni, (size_t)cap * 8);
  if (st == TS_OK && have > 0 &&
      (hipMemcpyAsync(ns.p, h->rng_s.p, (size_t)have * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
       hipMemcpyAsync(ni.p, h->rng_i.p, (size_t)have * 8, hipMemcpyDeviceToDevice, s) != hipSuccess)) {
    ts_set_error("range search: copying the result so far failed");
    st = TS_ERR_HIP;
  }
  // (the old buffers are freed below: everything that reads or writes them has to be over)
  if (st == TS_OK && hipStreamSynchronize(s) != hipSuccess) { ts_set_error("hipStreamSynchronize failed"); st = TS_ERR_HIP; }
  if (st != TS_OK) { ts_buf_release(ns); ts_buf_release(ni); return st; }
  ts_buf_release(h->rng_s);
  ts_buf_release(h->rng_i);
  h->rng_s = ns;
  h->rng_i = ni;
  h->rng_cap = cap;
  return TS_OK;
}

// One chunk of the dense path: the dense scan of rows [row0, row0 + rows) into W.dense, the allowed ids into W.mids.
static int range_dense_chunk(ts_index* h, ts_index::WSet& W, int nq, int qh, int64_t row0, int64_t rows,
                             int64_t chunk_rows, const MaskCtx* mc, hipStream_t s) {
  TS_CHECK(dense_chunk_scan(h, W, nq, qh, 0, row0, rows, chunk_rows, s));
  if (mc)
    TS_CHECK(ts_launch_mask_ids(mc->bits, mc->words, mc->mp, nq, row0, (uint32_t)rows, chunk_rows, (int32_t*)W.mids.p, s));
  return TS_OK;
}

// One pass of <= 64 queries (device pointers).  rad: the pass's radii (HOST).  *total: entries of the call so far; the
// pass appends its own behind them and writes lims[1 .. nq] (lims[0] is the pass's first offset, already set).
static int range_pass(ts_index* h, const void* dq, int nq, int q_dtype, const float* rad, const MaskCtx* mc,
                      uint32_t flags, int64_t limit, int64_t* total, int64_t* lims, RangeStats* stats, hipStream_t s) {
  const int64_t N = h->ntotal;
  const int64_t nblk = (N + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  const int qh = nq > 32 ? 2 : 1;
  SetLease set(h);
  ts_index::WSet& W = *set.W;
  TS_CHECK(set.wait_previous(s));
  // the query image of search_pass_on; the scan's counts start from zero
  TS_CHECK(ts_launch_qprep(h->L, dq, q_dtype, nq, qh, (uint4*)W.qimg.p, W.cand_cnt(), W.status(), s));
  // (fp32 storage with a mask or tombstones: the dense path, as its filtered top-k search)
  const bool filter = !(flags & TS_FLAG_NO_FILTER) && N >= kMinFilterRows && !(mc && h->L.dtype == TS_F32);
  stats->passes += 1;
  uint32_t cnt[TS_MAX_Q] = {0};
  float tau[TS_MAX_Q];
  for (int j = 0; j < TS_MAX_Q; ++j) tau[j] = j < nq ? rad[j] : 3.402823466e38f;
  bool dense = !filter;
  if (filter) {
    stats->filter_passes += 1;
    TS_HIP(hipMemcpyAsync(W.tau(), tau, sizeof(tau), hipMemcpyHostToDevice, s));
    TS_CHECK(ts_buf_ensure(W.cand_score, (size_t)TS_MAX_Q * kCandCap * 4));
    TS_CHECK(ts_buf_ensure(W.cand_id, (size_t)TS_MAX_Q * kCandCap * 4));
    ScanParams sp = scan_base(h, W, nq);
    scan_filter(sp, W, nblk);
    if (mc) {
      TS_CHECK(launch_live_blocks(h, W, *mc, s));
      TS_CHECK(ts_launch_scan_masked(h->L, qh, masked_scan_params(sp, W, *mc), filter_scan_cus(h), s));
    } else {
      TS_CHECK(ts_launch_scan(h->L, SCAN_FILTER, qh, sp, filter_scan_cus(h), s));
    }
    // the counts are exact, also past the cap: every survivor's atomic runs, only its store is guarded
    TS_HIP(hipMemcpyAsync(cnt, W.cand_cnt(), (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    TS_HIP(hipMemsetAsync(W.cand_cnt(), 0, 256, s));   // (the one-launch search expects the set's counts at zero)
    TS_HIP(hipStreamSynchronize(s));
    uint32_t maxc = 0;
    for (int j = 0; j < nq; ++j) maxc = std::max(maxc, cnt[j]);
    if (maxc > kCandCap) {   // the whole pass is redone densely
      dense = true;
      stats->dense_redo += 1;
    } else {
      int64_t off[TS_MAX_Q + 1];
      off[0] = *total;
      for (int j = 0; j < TS_MAX_Q; ++j) off[j + 1] = off[j] + (j < nq ? (int64_t)cnt[j] : 0);
      for (int j = 0; j < nq; ++j) lims[j + 1] = off[j + 1];
      if (off[nq] > limit) {
        ts_set_error("range search: %lld results so far exceed the limit of %lld", (long long)off[nq], (long long)limit);
        return TS_ERR_UNSUPPORTED;
      }
      TS_CHECK(range_reserve(h, off[nq], *total, limit, s));
      TsRangeSortParams rp{};
      rp.cand_score = (const float*)W.cand_score.p;
      rp.cand_id = (const int32_t*)W.cand_id.p;
      rp.cand_cap = kCandCap;
      for (int j = 0; j < TS_MAX_Q; ++j) rp.cnt[j] = cnt[j];
      for (int j = 0; j <= TS_MAX_Q; ++j) rp.off[j] = off[j];
      rp.out_scores = (float*)h->rng_s.p;
      rp.out_ids = (int64_t*)h->rng_i.p;
      rp.capacity = h->rng_cap;
      rp.id_offset = h->id_offset;
      TS_CHECK(ts_launch_range_sort(rp, nq, maxc, s));
      *total = off[nq];
    }
  }
  if (dense) {
    const auto [chunk_rows, nch] = dense_chunks(N);
    const int64_t chunk_tiles = (chunk_rows + TS_RANGE_TILE - 1) / TS_RANGE_TILE;
    const int64_t ntiles = nch * chunk_tiles;
    TS_CHECK(ts_buf_ensure(W.dense, (size_t)nq * chunk_rows * 4));
    if (mc) TS_CHECK(ts_buf_ensure(W.mids, (size_t)nq * chunk_rows * 4));
    TS_CHECK(ts_buf_ensure(h->rng_tiles, 256 + (size_t)nq * ntiles * 4));
    uint32_t* dtotal = (uint32_t*)h->rng_tiles.p;
    TsRangeDenseParams dp{};
    dp.dense = (const float*)W.dense.p;
    dp.mids = mc ? (const int32_t*)W.mids.p : nullptr;
    dp.ld = chunk_rows;
    dp.chunk_tiles = (uint32_t)chunk_tiles;
    dp.ntiles = ntiles;
    dp.tilecnt = dtotal + 64;
    for (int j = 0; j < TS_MAX_Q; ++j) dp.radius[j] = tau[j];
    // ---- count phase: every chunk's tile counts (each tile of the pass is written), then the prefix per query
    for (int64_t c = 0; c < nch; ++c) {
      const int64_t row0 = c * chunk_rows;
      const int64_t rows = std::min(chunk_rows, N - row0);
      TS_CHECK(range_dense_chunk(h, W, nq, qh, row0, rows, chunk_rows, mc, s));
      dp.row0 = row0;
      dp.rows = (uint32_t)rows;
      dp.tile0 = c * chunk_tiles;
      TS_CHECK(ts_launch_range_count(dp, nq, s));
    }
    TS_CHECK(ts_launch_range_prefix(dp.tilecnt, ntiles, nq, dtotal, s));
    uint32_t dcnt[TS_MAX_Q] = {0};
    TS_HIP(hipMemcpyAsync(dcnt, dtotal, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    TS_HIP(hipStreamSynchronize(s));
    if (filter) {   // both paths counted the same predicate over the same scores
      for (int j = 0; j < nq; ++j) {
        if (dcnt[j] != cnt[j]) {
          ts_set_error("range search: query %d has %u results on the dense path and %u on the filter scan", j, dcnt[j], cnt[j]);
          return TS_ERR_HIP;
        }
      }
    }
    dp.off[0] = *total;
    for (int j = 0; j < TS_MAX_Q; ++j) dp.off[j + 1] = dp.off[j] + (j < nq ? (int64_t)dcnt[j] : 0);
    for (int j = 0; j < nq; ++j) lims[j + 1] = dp.off[j + 1];
    if (dp.off[nq] > limit) {
      ts_set_error("range search: %lld results so far exceed the limit of %lld", (long long)dp.off[nq], (long long)limit);
      return TS_ERR_UNSUPPORTED;
    }
    TS_CHECK(range_reserve(h, dp.off[nq], *total, limit, s));
    dp.out_scores = (float*)h->rng_s.p;
    dp.out_ids = (int64_t*)h->rng_i.p;
    dp.capacity = h->rng_cap;
    dp.id_offset = h->id_offset;
    // ---- fill phase (one chunk: its scores are still in W.dense)
    for (int64_t c = 0; c < nch; ++c) {
      const int64_t row0 = c * chunk_rows;
      const int64_t rows = std::min(chunk_rows, N - row0);
      if (nch > 1) TS_CHECK(range_dense_chunk(h, W, nq, qh, row0, rows, chunk_rows, mc, s));
      dp.row0 = row0;
      dp.rows = (uint32_t)rows;
      dp.tile0 = c * chunk_tiles;
      TS_CHECK(ts_launch_range_fill(dp, nq, s));
    }
    *total = dp.off[nq];
  }
  return set.done(s);
}

extern "C" int ts_index_range_search(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, const float* radius,
                                     const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks,
                                     const int32_t* mask_of_query, int64_t max_total, int64_t* lims, uint32_t flags,
                                     void* stream) {
  // the checks that need no handle come first (and none of them touches the GPU)
  if (!lims) { ts_set_error("range_search: lims is null"); return TS_ERR_INVALID; }
  if (nq < 0 || !dtype_ok(q_dtype) || (nq > 0 && (!queries || !radius))) {
    ts_set_error("bad arguments to range_search");
    return TS_ERR_INVALID;
  }
  if (flags & ~(uint32_t)(TS_FLAG_HOST_PTR | TS_FLAG_NO_FILTER)) {
    ts_set_error("range_search takes TS_FLAG_HOST_PTR and TS_FLAG_NO_FILTER only (it is synchronous)");
    return TS_ERR_INVALID;
  }
  for (int32_t q = 0; q < nq; ++q) {
    if (radius[q] != radius[q]) { ts_set_error("range_search: radius[%d] is NaN", q); return TS_ERR_INVALID; }
  }
  TS_CHECK(check_mask_args("range_search", nq, allow_bits, allow_words, n_masks, mask_of_query));
  lims[0] = 0;
  if (nq == 0) {
    if (h) {
      std::lock_guard<std::mutex> rlk(h->range_mu);
      h->rng_total = 0;
      h->rng_valid = true;
    }
    return TS_OK;
  }
  for (int32_t q = 0; q < nq; ++q) lims[q + 1] = 0;
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  if (h->L.dtype == TS_FP8_E4M3) {
    ts_set_error("range_search is not supported on an e4m3 (fp8) index");
    return TS_ERR_UNSUPPORTED;
  }
  if (h->L.dtype == TS_MXFP4_E2M1) {
    ts_set_error("range_search is not supported on a 4-bit MX (mxfp4) index");
    return TS_ERR_UNSUPPORTED;
  }
  const int64_t N = h->ntotal;
  if (!mask_of_query) n_masks = 0;   // unfiltered
  TS_CHECK(check_mask_words("range_search", n_masks, allow_words, N));
  if (N == 0) return err_empty();
  const int64_t limit = max_total <= 0 ? kRangeDefaultMax : max_total;
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));   // a range search never joins a coalesced pass
  std::lock_guard<std::mutex> rlk(h->range_mu);
  h->rng_valid = false;
  h->rng_total = 0;
  const int qp = queries_per_pass(h);
  const size_t qrow = (size_t)h->L.dim * dtype_size(q_dtype);
  CallBuffers b(h);
  TS_CHECK(b.in((flags & TS_FLAG_HOST_PTR) != 0, queries, (size_t)nq * qrow, allow_bits,
                (size_t)n_masks * (size_t)allow_words * 4, nullptr, nullptr, 0, s));
  const std::vector<int32_t> none((size_t)nq, -1);
  if (!mask_of_query) mask_of_query = none.data();
  LiveMasks eff(h);
  TS_CHECK(eff.apply(nq, b.bits, allow_words, n_masks, mask_of_query, s));
  RangeStats stats;
  int64_t total = 0;
  int st = TS_OK;
  for (int q0 = 0; q0 < nq && st == TS_OK; q0 += qp) {
    const int c = std::min(qp, nq - q0);
    MaskCtx mc{};
    mc.bits = b.bits;
    mc.words = allow_words;
    const bool masked = build_mask_pass(mask_of_query + q0, c, mc.mp);
    lims[q0] = total;
    st = range_pass(h, (const char*)b.dq + (size_t)q0 * qrow, c, q_dtype, radius + q0, masked ? &mc : nullptr, flags,
                    limit, &total, lims + q0, &stats, s);
  }
  if (st != TS_OK) {
    // lims hold the counts so far: the passes that ran (a pass whose counts are known has written them), flat behind
    for (int q = 1; q <= nq; ++q)
      if (lims[q] < lims[q - 1]) lims[q] = lims[q - 1];
    (void)hipStreamSynchronize(s);
    eff.done_after_failure(s);
    set_info(h, 32, stats.passes, stats.filter_passes, stats.dense_redo);
    return st;
  }
  TS_CHECK(eff.done(s));
  TS_HIP(hipStreamSynchronize(s));
  h->rng_total = total;
  h->rng_valid = true;
  set_info(h, 32 | (stats.dense_redo ? 2 : (stats.filter_passes ? 1 : 0)), stats.passes, stats.filter_passes, stats.dense_redo);
  return TS_OK;
}

extern "C" int ts_index_range_fetch(ts_index* h, float* out_scores, int64_t* out_ids, int64_t capacity, uint32_t flags,
                                    void* stream) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  if (capacity < 0 || (flags & ~(uint32_t)TS_FLAG_HOST_PTR)) { ts_set_error("bad arguments to range_fetch"); return TS_ERR_INVALID; }
  std::lock_guard<std::mutex> rlk(h->range_mu);
  if (!h->rng_valid) {
    ts_set_error("range_fetch: no range search result is stored (none was run, it failed, or the index has changed since)");
    return TS_ERR_INVALID;
  }
  const int64_t n = h->rng_total;
  if (capacity < n) {
    ts_set_error("range_fetch: capacity %lld is less than the %lld stored results", (long long)capacity, (long long)n);
    return TS_ERR_INVALID;
  }
  if (n == 0) return TS_OK;
  if (!out_scores || !out_ids) { ts_set_error("range_fetch: null output"); return TS_ERR_INVALID; }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const hipMemcpyKind kind = (flags & TS_FLAG_HOST_PTR) ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  TS_HIP(hipMemcpyAsync(out_scores, h->rng_s.p, (size_t)n * 4, kind, s));
  TS_HIP(hipMemcpyAsync(out_ids, h->rng_i.p, (size_t)n * 8, kind, s));
  TS_HIP(hipStreamSynchronize(s));
  return TS_OK;
}

// ---- removal (include/tristage.h "removal")
// `s` waits for every search enqueued so far on this handle, on any stream: each workspace set records ev_sel behind
// the last search that used it (the five-launch, one-launch, dense and coalesced paths alike)
static int wait_for_searches(ts_index* h, hipStream_t s) {
  std::lock_guard<std::mutex> lk(h->mu);
  for (ts_index::WSet& w : h->ws)
    if (w.used && hipEventQuery(w.ev_sel) != hipSuccess) TS_HIP(hipStreamWaitEvent(s, w.ev_sel, 0));
  return TS_OK;
}

namespace {
constexpr size_t kCompactStageBytes = 256u << 20;   // compaction's staging buffer: chunks of whole row blocks
}  // namespace

extern "C" int ts_index_remove(ts_index* h, const int64_t* ids, int64_t n, int64_t* n_removed, void* stream) {
  if (!h || !n_removed || n < 0 || (n > 0 && !ids)) { ts_set_error("bad arguments to remove"); return TS_ERR_INVALID; }
  *n_removed = 0;
  if (n == 0 || h->ntotal == 0) return TS_OK;
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));   // held passes search the index as it was when they were submitted
  h->rng_valid = false;
  std::lock_guard<std::mutex> elk(h->eff_mu);
  // searches submitted earlier (on any stream) have read the bitmap before it changes: eff_ev follows the last
  // call's passes, and that call's stream waited for the one before it
  if (h->eff_used) TS_HIP(hipStreamWaitEvent(s, h->eff_ev, 0));
  TS_CHECK(wait_for_searches(h, s));
  if (h->nremoved == 0) {   // the first removal: the bitmap starts all-live
    TS_CHECK(live_reserve(h, h->ntotal, s));
    TS_HIP(hipMemsetAsync(h->live.p, 0, (size_t)h->live_cap_words * 4, s));
    TS_CHECK(ts_launch_live_set((uint32_t*)h->live.p, 0, h->ntotal, s));
  }
  const int64_t chunk = std::min<int64_t>(n, 1 << 22);
  TS_CHECK(ts_buf_ensure(h->rids, (size_t)chunk * 8 + 256));
  unsigned long long* cnt = (unsigned long long*)((char*)h->rids.p + (size_t)chunk * 8);
  TS_HIP(hipMemsetAsync(cnt, 0, 8, s));
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    const int64_t c = std::min(chunk, n - i0);
    TS_HIP(hipMemcpyAsync(h->rids.p, ids + i0, (size_t)c * 8, hipMemcpyHostToDevice, s));
    TS_CHECK(ts_launch_live_clear((uint32_t*)h->live.p, (const int64_t*)h->rids.p, c, h->id_offset, h->ntotal, cnt,
                                  s));
  }
  unsigned long long cleared = 0;
  TS_HIP(hipMemcpyAsync(&cleared, cnt, 8, hipMemcpyDeviceToHost, s));
  TS_HIP(hipStreamSynchronize(s));
  h->nremoved += (int64_t)cleared;
  *n_removed = (int64_t)cleared;
  return TS_OK;
}

// ---- update in place (include/tristage.h "update")
namespace {
constexpr size_t kUpdateStageBytes = 64u << 20;   // the tiled staging of one chunk (whole row blocks)
}  // namespace
// -DTS_UPDATE_TRACE: host-clock time of each phase of ts_index_update, summed over the chunks, on stderr
#ifdef TS_UPDATE_TRACE
#include <chrono>
struct UpdTrace {
  const char* name[8] = {"check ids", "ordering waits", "live check", "relayout launch", "group blocks", "table uploads",
                         "kernel launches", "synchronise"};
  double us[8] = {0};
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void mark(int phase) {
    const auto now = std::chrono::steady_clock::now();
    us[phase] += std::chrono::duration<double, std::micro>(now - t).count();
    t = now;
  }
  ~UpdTrace() {
    for (int i = 0; i < 8; ++i) fprintf(stderr, "ts_index_update %-16s %9.1f us\n", name[i], us[i]);
  }
};
#define UPD_MARK(p) upd_trace.mark(p)
#else
#define UPD_MARK(p) ((void)0)
#endif

extern "C" int ts_index_update(ts_index* h, const int64_t* ids, int64_t n, const void* rows, int32_t rows_dtype,
                               uint32_t flags, void* stream) {
  if (!h || n < 0 || (n > 0 && (!ids || !rows)) || !dtype_ok(rows_dtype)) {
    ts_set_error("bad arguments to update");
    return TS_ERR_INVALID;
  }
  if (n == 0) return TS_OK;
#ifdef TS_UPDATE_TRACE
  UpdTrace upd_trace;
#endif
  std::vector<int64_t> r((size_t)n);
  std::vector<uint64_t> keys;   // row << 32 | position, ordered by row
  TS_CHECK(ts_update_check_ids(ids, n, h->id_offset, h->ntotal, r.data(), &keys));
  UPD_MARK(0);
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));   // held passes search the rows as they were when they were submitted
  h->rng_valid = false;
  std::lock_guard<std::mutex> elk(h->eff_mu);
  // as ts_index_remove: searches submitted earlier, on any path and any stream, have read the rows before they change
  if (h->eff_used) TS_HIP(hipStreamWaitEvent(s, h->eff_ev, 0));
  TS_CHECK(wait_for_searches(h, s));
  UPD_MARK(1);
  if (h->nremoved > 0) {   // a removed row cannot be updated: counted before anything is written
    const int64_t chunk = std::min<int64_t>(n, 1 << 22);
    TS_CHECK(ts_buf_ensure(h->rids, (size_t)chunk * 8 + 256));
    unsigned long long* cnt = (unsigned long long*)((char*)h->rids.p + (size_t)chunk * 8);
    unsigned long long dead[2] = {0ull, ~0ull};
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
      const int64_t c = std::min(chunk, n - i0);
      unsigned long long init[2] = {0ull, ~0ull};
      TS_HIP(hipMemcpyAsync(cnt, init, 16, hipMemcpyHostToDevice, s));
      TS_HIP(hipMemcpyAsync(h->rids.p, r.data() + i0, (size_t)c * 8, hipMemcpyHostToDevice, s));
      TS_CHECK(ts_launch_update_live_check((const uint32_t*)h->live.p, (const int64_t*)h->rids.p, c, cnt, s));
      TS_HIP(hipMemcpyAsync(dead, cnt, 16, hipMemcpyDeviceToHost, s));
      TS_HIP(hipStreamSynchronize(s));
      if (dead[0] != 0ull) {
        ts_set_error("update: id %lld was removed", (long long)ids[i0 + (int64_t)dead[1]]);
        return TS_ERR_INVALID;
      }
    }
  }
  UPD_MARK(2);
  const bool norm = (flags & TS_FLAG_NORMALIZE) != 0;
  const bool host = (flags & TS_FLAG_HOST_PTR) != 0;
  const size_t row_bytes = (size_t)h->L.dim * dtype_size(rows_dtype);
  const size_t bb = ts_block_bytes(h->L);
  bool run = true;   // the ids are one ascending run of consecutive rows (the bulk re-embed of a range)
  for (int64_t i = 1; i < n && run; ++i) run = r[(size_t)i] == r[(size_t)i - 1] + 1;
  // Chunks of the call's rows, in the order given.  A run is written by the relayout of ts_index_add itself, at its
  // rows (it writes the units of the rows it is given and of no other).  Otherwise the relayout writes chunk row j to
  // row j of a staging tile and the two kernels of ts_update.hip move the tile's rows to their places.
  int64_t chunk = run ? n : std::max<int64_t>(1, (int64_t)(kUpdateStageBytes / bb)) * TS_ROWS_PER_BLOCK;
  if (host) chunk = std::min(chunk, std::max<int64_t>(TS_ROWS_PER_BLOCK, (int64_t)((64u << 20) / row_bytes) / TS_ROWS_PER_BLOCK * TS_ROWS_PER_BLOCK));
  chunk = std::min(chunk, (n + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK * TS_ROWS_PER_BLOCK);
  const size_t tile_bytes = run ? 0 : (size_t)(chunk / TS_ROWS_PER_BLOCK) * bb;
  if (!run) TS_CHECK(ts_buf_ensure(h->upd_tile, tile_bytes));
  if (host) TS_CHECK(ts_buf_ensure(h->stage, (size_t)chunk * row_bytes));
  if (norm) TS_CHECK(ts_buf_ensure(h->den, (size_t)chunk * 4));
  TsUpdateTables tab;
  std::vector<uint64_t> chunk_keys;
  if (!run && keys.empty()) ts_update_sort_rows(r.data(), n, &keys);   // (ascending ids that are not one run)
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    const int64_t c = std::min(chunk, n - i0);
    const void* src_rows = (const char*)rows + (size_t)i0 * row_bytes;
    if (host) {
      TS_HIP(hipMemcpyAsync(h->stage.p, src_rows, (size_t)c * row_bytes, hipMemcpyHostToDevice, s));
      src_rows = h->stage.p;
    }
    if (run) {
      TS_CHECK(ts_launch_relayout(h->L, src_rows, rows_dtype, c, r[(size_t)i0], h->corpus, norm, (float*)h->den.p, s));
      TS_HIP(hipStreamSynchronize(s));   // (the staging of host rows and the norms are reused by the next chunk)
      continue;
    }
    TS_CHECK(ts_launch_relayout(h->L, src_rows, rows_dtype, c, 0, (uint4*)h->upd_tile.p, norm, (float*)h->den.p, s));
    UPD_MARK(3);
    const uint64_t* ck = keys.data();
    if (c != n) {   // the chunk's keys in the order the id check found, positions counted from the chunk's first row
      chunk_keys.resize((size_t)n + 1);
      size_t m = 0;
      for (const uint64_t k : keys) {   // (without a branch: which chunk a key belongs to is not predictable)
        chunk_keys[m] = k - (uint64_t)i0;
        m += (size_t)((uint64_t)((int64_t)(uint32_t)k - i0) < (uint64_t)c);
      }
      ck = chunk_keys.data();
    }
    ts_update_group_blocks(ck, c, &tab);
    UPD_MARK(4);
    // device tables, back to back: full blk, full src, part blk, part first, part item
    const std::vector<int32_t>* parts[5] = {&tab.full_blk, &tab.full_src, &tab.part_blk, &tab.part_first, &tab.part_item};
    size_t off[6] = {0};
    for (int i = 0; i < 5; ++i) off[i + 1] = off[i] + ((parts[i]->size() + 63) & ~(size_t)63);
    TS_CHECK(ts_buf_ensure(h->upd_tab, off[5] * 4));
    int32_t* dtab = (int32_t*)h->upd_tab.p;
    for (int i = 0; i < 5; ++i)
      if (!parts[i]->empty())
        TS_HIP(hipMemcpyAsync(dtab + off[i], parts[i]->data(), parts[i]->size() * 4, hipMemcpyHostToDevice, s));
    UPD_MARK(5);
    TS_CHECK(ts_launch_update_blocks(h->L, (const uint4*)h->upd_tile.p, h->corpus, dtab + off[0], dtab + off[1],
                                     (int64_t)tab.full_blk.size(), s));
    TS_CHECK(ts_launch_update_rows(h->L, (const uint4*)h->upd_tile.p, h->corpus, dtab + off[2], dtab + off[3],
                                   dtab + off[4], (int64_t)tab.part_blk.size(), s));
    UPD_MARK(6);
    TS_HIP(hipStreamSynchronize(s));   // the staging tile and the tables are reused by the next chunk
    UPD_MARK(7);
  }
  // (the staging tile, at most kUpdateStageBytes, and the tables stay allocated: giving a 64 MiB tile back and taking it
  // again cost a 100 000-id call 0.2 of its 2 ms)
  return TS_OK;
}

extern "C" int64_t ts_index_live_count(const ts_index* h) { return h ? h->ntotal - h->nremoved : -1; }

extern "C" int ts_index_live_words(ts_index* h, uint32_t* out, void* stream) {
  if (!h || (!out && h->ntotal > 0)) { ts_set_error("bad arguments to live_words"); return TS_ERR_INVALID; }
  const int64_t words = (h->ntotal + 31) / 32;
  if (words == 0) return TS_OK;
  if (h->nremoved == 0) {
    for (int64_t w = 0; w < words; ++w) {
      const int64_t rows = h->ntotal - w * 32;
      out[w] = rows >= 32 ? ~0u : ((1u << rows) - 1u);
    }
    return TS_OK;
  }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_HIP(hipMemcpyAsync(out, h->live.p, (size_t)words * 4, hipMemcpyDeviceToHost, s));
  TS_HIP(hipStreamSynchronize(s));
  return TS_OK;
}

extern "C" int ts_index_compact(ts_index* h, int64_t* old2new, void* stream) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  const int64_t N = h->ntotal;
  if (h->nremoved == 0) {
    if (old2new)
      for (int64_t r = 0; r < N; ++r) old2new[r] = r;
    return TS_OK;
  }
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));
  h->rng_valid = false;
  std::lock_guard<std::mutex> elk(h->eff_mu);
  if (h->eff_used) TS_HIP(hipStreamWaitEvent(s, h->eff_ev, 0));   // earlier searches have read the old corpus
  TS_CHECK(wait_for_searches(h, s));
  const size_t sb = ts_compact_scratch_bytes(N);
  if (sb == 0) { ts_set_error("bad compaction size"); return TS_ERR_INVALID; }
  TS_CHECK(ts_buf_ensure(h->compact_scratch, sb + (old2new ? (size_t)N * 8 : 0)));
  const size_t stage = std::max(kCompactStageBytes - kCompactStageBytes % ts_block_bytes(h->L), ts_block_bytes(h->L));
  TS_CHECK(ts_buf_ensure(h->compact_stage, stage));
  int64_t* o2n = old2new ? (int64_t*)((char*)h->compact_scratch.p + sb) : nullptr;
  int64_t nlive = 0;
  const int st = ts_compact_corpus(h->L, h->corpus, (const uint32_t*)h->live.p, N, h->compact_scratch.p, sb,
                                   (uint4*)h->compact_stage.p, stage, o2n, &nlive, s);
  if (st == TS_ERR_INVALID) ts_set_error("compaction scratch too small");
  TS_CHECK(st);
  if (old2new) TS_HIP(hipMemcpyAsync(old2new, o2n, (size_t)N * 8, hipMemcpyDeviceToHost, s));
  TS_HIP(hipStreamSynchronize(s));
  // the staging buffer is the size of a few hundred row blocks: given back, as the scratch is
  ts_buf_release(h->compact_stage);
  ts_buf_release(h->compact_scratch);
  h->ntotal = nlive;
  h->nremoved = 0;
  return TS_OK;
}

// All inner products (no selection): the dense scan writes straight into the caller's matrix.
extern "C" int ts_index_scores(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, float* out,
                               int64_t ld, void* stream) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  if (nq == 0) return TS_OK;
  const int64_t N = h->ntotal;
  const int64_t nblk = (N + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  if (!queries || !out || nq < 0 || !dtype_ok(q_dtype) || ld < nblk * TS_ROWS_PER_BLOCK || (ld & 3) ||
      (reinterpret_cast<uintptr_t>(out) & 15)) {
    ts_set_error("bad arguments to scores (ld must be a multiple of 4 and >= ntotal rounded up to 32, out 16-byte aligned)");
    return TS_ERR_INVALID;
  }
  if (N == 0) return err_empty();
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  TS_CHECK(co_flush(h, s));
  const int qp = queries_per_pass(h);
  const size_t qrow = (size_t)h->L.dim * dtype_size(q_dtype);
  for (int q0 = 0; q0 < nq; q0 += qp) {
    const int c = std::min(qp, nq - q0);
    const int qh = c > 32 ? 2 : 1;
    SetLease set(h);
    TS_CHECK(set.wait_previous(s));
    TS_CHECK(ts_launch_qprep(h->L, (const char*)queries + (size_t)q0 * qrow, q_dtype, c, qh, (uint4*)set.W->qimg.p,
                             nullptr, nullptr, s));
    ScanParams sp = scan_base(h, *set.W, c);
    scan_window(sp, 0, nblk, 1, out + (size_t)q0 * ld, ld);
    TS_CHECK(ts_launch_scan(h->L, SCAN_DENSE, qh, sp, h->num_cus, s));
    TS_CHECK(set.done(s));
  }
  TS_HIP(hipStreamSynchronize(s));
  return TS_OK;
}

// 1 = a search with this k goes through the threshold filter (its result has to be VERIFIED: a synchronous call does
// it, an asynchronous one leaves it to ts_index_finish), 0 = it takes the dense path, which is exact by construction —
// an asynchronous search is then final as soon as the stream reaches it.  Mirrors search_pass_on.
extern "C" int ts_index_filter_path(const ts_index* h, int32_t k) {
  if (!h || k <= 0) { ts_set_error("bad arguments to filter_path"); return TS_ERR_INVALID; }
  const int64_t N = h->ntotal;
  return (k <= kMaxFilterK && N >= kMinFilterRows && N >= 32 * (int64_t)k) ? 1 : 0;
}

extern "C" int64_t ts_index_last_ticket(const ts_index* h) {
  if (!h) return -1;
  std::lock_guard<std::mutex> lk(const_cast<ts_index*>(h)->mu);
  return h->next_ticket - 1;
}

extern "C" int ts_index_finish(ts_index* h, void* stream, int64_t* failed_tickets, int32_t max_failed,
                               int32_t* n_failed) {
  if (!h || !n_failed || max_failed < 0 || (max_failed > 0 && !failed_tickets)) {
    ts_set_error("bad arguments to finish");
    return TS_ERR_INVALID;
  }
  TsDeviceGuard g(h->device);
  {
    std::lock_guard<std::mutex> clk(h->co_mu);
    TS_CHECK(co_flush_locked(h, (hipStream_t)stream));   // the sync below then covers every held pass
  }
  TS_HIP(hipStreamSynchronize((hipStream_t)stream));
  std::lock_guard<std::mutex> lk(h->mu);
  int nf = 0;
  uint32_t maxc = 0;
  for (int i = 0; i < h->npending; ++i) {
    ts_index::Pending& pe = h->pending[i];
    const uint32_t* rep = h->host_status + (size_t)pe.slot * TS_SLOT_WORDS;
    for (int q = 0; q < pe.nq; ++q) maxc = std::max(maxc, rep[q]);
    if (rep[64] != 0) {
      if (pe.set >= 0 && pe.set < TS_NSETS) h->ws[pe.set].hist_dirty = true;
      if (nf == 0 || failed_tickets[nf - 1] != pe.ticket) {
        if (nf < max_failed) failed_tickets[nf] = pe.ticket;
        ++nf;
      }
    }
    if (pe.e0 && pe.e1) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pe.e0, pe.e1) == hipSuccess) { h->phase_ms[3] += ms; h->phase_cnt[3] += 1; }
      (void)hipEventDestroy(pe.e0);
      (void)hipEventDestroy(pe.e1);
    }
    h->info[0] = 1 | (pe.set >= 0 ? 16 : 0); h->info[2] = pe.S; h->info[3] = pe.m;
    if (pe.fseq >= 0 && pe.fseq == h->fseq) h->finfo[0] += rep[65];
    h->slot_busy[pe.slot] = false;
  }
  if (h->npending) h->info[1] = maxc;
  h->npending = 0;
  *n_failed = nf;
  if (nf > max_failed) { ts_set_error("%d searches need a redo but only %d tickets fit", nf, max_failed); return TS_ERR_INVALID; }
  return TS_OK;
}

extern "C" int ts_index_set_profiling(ts_index* h, int32_t on) {
  if (!h) { ts_set_error("null handle"); return TS_ERR_INVALID; }
  TsDeviceGuard g(h->device);
  if (on && !h->ev[0]) {
    for (hipEvent_t& e : h->ev) TS_HIP(hipEventCreate(&e));
  }
  h->profiling = on != 0;
  h->prof_every = on > 1 ? on : 1;   // on = N: time every N-th search
  h->prof_seq.store(0);
  return TS_OK;
}

extern "C" int ts_index_get_timings(ts_index* h, double ms[8], int64_t counts[8], int32_t reset) {
  if (!h || !ms || !counts) { ts_set_error("bad arguments"); return TS_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(h->mu);
  for (int i = 0; i < TS_NPHASE; ++i) {
    ms[i] = h->phase_ms[i];
    counts[i] = h->phase_cnt[i];
    if (reset) { h->phase_ms[i] = 0.0; h->phase_cnt[i] = 0; }
  }
  return TS_OK;
}

// ------------------------------------------------------------------ read-bandwidth probe
// What a kernel that ONLY reads the index's tiled corpus reaches on this box, with the scan's own access pattern
// (persistent workgroups of 8 waves on 7/8 of the CUs, wave w takes row blocks w, w + W, ...; a block is kg
// contiguous 1 KiB units read 8 at a time with non-temporal 16-byte loads) and nothing else: no LDS, no MFMA, no
// epilogue.  bench.py reports it next to the 8 TB/s specification as the measured ceiling.
typedef uint32_t probe_u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(512) void read_probe_kernel(const probe_u32x4* corpus, int64_t nblk, int kg,
                                                         uint32_t* sink) {
  const int lane = threadIdx.x & 63;
  const int64_t W = (int64_t)gridDim.x * (blockDim.x >> 6);
  probe_u32x4 acc = {0u, 0u, 0u, 0u};
  // two groups of 8 loads alternate, so 8-16 KiB per wave are always in flight (the scan keeps 8 KiB in its ring and a
  // few waits apart; a probe that waited for each group before requesting the next read SLOWER than the scan).  No
  // branch around a load: the group index is clamped instead (a wave re-reads at most its last two groups).
  const int64_t b0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int gpb = kg / 8;                                       // groups of 8 units per row block
  const int64_t myblocks = b0 < nblk ? (nblk - b0 + W - 1) / W : 0;
  const int64_t ng = myblocks * gpb;
  if (ng == 0) return;
  auto group = [&](int64_t t) -> const probe_u32x4* {
    t = t < ng ? t : ng - 1;
    return corpus + ((size_t)(b0 + (t / gpb) * W) * kg + (size_t)(t % gpb) * 8) * 64 + lane;
  };
  probe_u32x4 va[8], vb[8];
  {
    const probe_u32x4* q = group(0);
#pragma unroll
    for (int i = 0; i < 8; ++i) va[i] = __builtin_nontemporal_load(q + (size_t)i * 64);
  }
  for (int64_t t = 0; t < ng; t += 2) {
    const probe_u32x4* qb = group(t + 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) vb[i] = __builtin_nontemporal_load(qb + (size_t)i * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc ^= va[i];
    const probe_u32x4* qa = group(t + 2);
#pragma unroll
    for (int i = 0; i < 8; ++i) va[i] = __builtin_nontemporal_load(qa + (size_t)i * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc ^= vb[i];
  }
  if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x9e3779b9u) sink[0] = 1u;   // keeps the loads alive; practically never true
}

extern "C" int ts_index_read_probe(ts_index* h, int32_t reps, double* ms_avg, double* ms_best, int64_t* bytes,
                                   void* stream) {
  if (!h || reps <= 0 || reps > 1000 || !ms_avg || !ms_best || !bytes) {
    ts_set_error("bad arguments to read_probe");
    return TS_ERR_INVALID;
  }
  if (h->ntotal == 0) return err_empty();
  TsDeviceGuard g(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nblk = (h->ntotal + TS_ROWS_PER_BLOCK - 1) / TS_ROWS_PER_BLOCK;
  const int grid = std::max(1, filter_scan_cus(h));
  ts_index::WSet* W = acquire_set(h);          // its 4 KiB scratch page: word 1023 is nobody's
  uint32_t* sink = (uint32_t*)W->small.p + 1023;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int st = TS_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) st = TS_ERR_HIP;
  double sum = 0.0, best = 1e30;
  for (int r = 0; r <= reps && st == TS_OK; ++r) {     // pass 0 is a warm-up
    if (hipEventRecord(e0, s) != hipSuccess) { st = TS_ERR_HIP; break; }
    hipLaunchKernelGGL(read_probe_kernel, dim3(grid), dim3(512), 0, s, (const probe_u32x4*)h->corpus, nblk, h->L.kg, sink);
    float ms = 0.f;
    if (hipGetLastError() != hipSuccess || hipEventRecord(e1, s) != hipSuccess ||
        hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { st = TS_ERR_HIP; break; }
    if (r) { sum += ms; best = std::min(best, (double)ms); }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  release_set(h, W);
  if (st != TS_OK) { ts_set_error("HIP call failed in ts_index_read_probe"); return st; }
  *ms_avg = sum / reps;
  *ms_best = best;
  *bytes = nblk * (int64_t)ts_block_bytes(h->L);
  return TS_OK;
}

// ------------------------------------------------------------------ diagnostics
// The per-device one-time table (ts_common.h TsDeviceOnce) exercised WITHOUT a GPU: n_threads host
// threads race through n_devices device numbers; every device's action must run exactly once, a
// failing action must be retried, and an out-of-range device must run the action every time.
extern "C" int ts_selftest_device_once(int32_t n_threads, int32_t n_devices) {
  if (n_threads <= 0 || n_threads > 256 || n_devices <= 0 || n_devices > TS_MAX_DEVICES) {
    ts_set_error("bad arguments to selftest");
    return TS_ERR_INVALID;
  }
  TsDeviceOnce once;
  std::atomic<int> runs[TS_MAX_DEVICES];
  std::atomic<int> fails[TS_MAX_DEVICES];
  for (int i = 0; i < TS_MAX_DEVICES; ++i) { runs[i] = 0; fails[i] = 0; }
  std::atomic<int> bad{0}, untracked{0};
  auto worker = [&](int t) {
    for (int rep = 0; rep < 200; ++rep) {
      const int dev = (t + rep) % n_devices;
      int st;
      do {
        st = ts_once_per_device(once, dev, [&]() -> int {
          // the first attempt on every odd device fails: it must not be recorded as done
          if ((dev & 1) && fails[dev].fetch_add(1) == 0) return TS_ERR_HIP;
          runs[dev].fetch_add(1);
          return TS_OK;
        });
      } while (st != TS_OK);
      if (!(once.done.load() & (1ull << dev))) bad.fetch_add(1);
    }
    (void)ts_once_per_device(once, TS_MAX_DEVICES + t, [&]() -> int { untracked.fetch_add(1); return TS_OK; });
    (void)ts_once_per_device(once, -1, [&]() -> int { untracked.fetch_add(1); return TS_OK; });
  };
  std::vector<std::thread> th;
  for (int t = 0; t < n_threads; ++t) th.emplace_back(worker, t);
  for (std::thread& x : th) x.join();
  for (int d = 0; d < n_devices; ++d)
    if (runs[d].load() != 1) { ts_set_error("device %d: action ran %d times", d, runs[d].load()); return TS_ERR_INVALID; }
  for (int d = n_devices; d < TS_MAX_DEVICES; ++d)
    if (runs[d].load() != 0 || (once.done.load() & (1ull << d))) { ts_set_error("device %d touched", d); return TS_ERR_INVALID; }
  if (bad.load() || untracked.load() != 2 * n_threads) {
    ts_set_error("bit missing after success (%d) or untracked runs %d != %d", bad.load(), untracked.load(), 2 * n_threads);
    return TS_ERR_INVALID;
  }
  return TS_OK;
}

// ------------------------------------------------------------------ merge
static int merge_once(const float* scores, const int64_t* ids, int32_t nlists, int32_t nq, int32_t k,
                      int64_t score_list_stride, int64_t id_list_stride, float* out_scores,
                      int64_t* out_ids, void* stream) {
  SelParams p{};
  p.mode = SEL_MERGE64;
  p.scores = scores;
  p.ids64 = ids;
  p.stride = k;                       // query q of list 0 starts at q*k
  p.seg_len = (uint32_t)k;
  p.seg_stride = score_list_stride;   // next list (scores)
  p.seg_stride_ids = id_list_stride;  // next list (ids)
  p.n = (uint32_t)(nlists * k);
  p.k = k;
  p.out_scores = out_scores;
  p.out_ids64 = out_ids;
  p.out_stride = k;
  return ts_launch_select(p, nq, (hipStream_t)stream);
}

static int merge_impl(const float* scores, const int64_t* ids, int32_t nlists, int32_t nq, int32_t k,
                      int64_t score_list_stride, int64_t id_list_stride, float* out_scores,
                      int64_t* out_ids, int32_t device, void* stream) {
  if (!scores || !ids || !out_scores || !out_ids || nlists <= 0 || nq < 0 || k <= 0) {
    ts_set_error("bad arguments to merge");
    return TS_ERR_INVALID;
  }
  if (nq == 0) return TS_OK;
  if (k > TS_SEL_LDS_KEYS / 2) {
    ts_set_error("merge: k = %d exceeds %d", k, TS_SEL_LDS_KEYS / 2);
    return TS_ERR_UNSUPPORTED;
  }
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  if ((int64_t)nlists * k <= TS_SEL_LDS_KEYS)
    return merge_once(scores, ids, nlists, nq, k, score_list_stride, id_list_stride, out_scores, out_ids, stream);
  // More entries per query than one workgroup selects among in LDS (e.g. 16 ranks x k = 2048): merge the lists
  // in groups that fit, then merge the groups' results — the order (score desc, id asc) is total, so merging is
  // associative and the result is the same.  Rare, so the intermediate lists are allocated on the spot.
  const int per = TS_SEL_LDS_KEYS / k;                    // lists per group (>= 2)
  const int ngroups = (nlists + per - 1) / per;
  float* ts = nullptr;
  int64_t* ti = nullptr;
  const size_t cells = (size_t)ngroups * nq * k;
  if (hipMalloc((void**)&ts, cells * 4) != hipSuccess || hipMalloc((void**)&ti, cells * 8) != hipSuccess) {
    if (ts) (void)hipFree(ts);
    ts_set_error("merge: cannot allocate %zu bytes of intermediate lists", cells * 12);
    return TS_ERR_OOM;
  }
  int st = TS_OK;
  for (int gi = 0; gi < ngroups && st == TS_OK; ++gi) {
    const int l0 = gi * per, nl = std::min(per, nlists - l0);
    st = merge_once(scores + (size_t)l0 * score_list_stride, ids + (size_t)l0 * id_list_stride, nl, nq, k,
                    score_list_stride, id_list_stride, ts + (size_t)gi * nq * k, ti + (size_t)gi * nq * k, stream);
  }
  if (st == TS_OK)
    st = merge_impl(ts, ti, ngroups, nq, k, (int64_t)nq * k, (int64_t)nq * k, out_scores, out_ids, device, stream);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && st == TS_OK) {
    ts_set_error("merge: stream synchronisation failed");
    st = TS_ERR_HIP;
  }
  (void)hipFree(ts);
  (void)hipFree(ti);
  return st;
}

extern "C" int ts_merge_topk(const float* scores, const int64_t* ids, int32_t nlists,
                             int32_t nq, int32_t k, float* out_scores, int64_t* out_ids,
                             int32_t device, void* stream) {
  return merge_impl(scores, ids, nlists, nq, k, (int64_t)nq * k, (int64_t)nq * k, out_scores, out_ids,
                    device, stream);
}

extern "C" int ts_merge_topk_strided(const float* scores, const int64_t* ids, int32_t nlists,
                                     int32_t nq, int32_t k, int64_t score_list_stride,
                                     int64_t id_list_stride, float* out_scores, int64_t* out_ids,
                                     int32_t device, void* stream) {
  return merge_impl(scores, ids, nlists, nq, k, score_list_stride, id_list_stride, out_scores, out_ids,
                    device, stream);
}

// ------------------------------------------------------------------ maxsim
extern "C" int ts_maxsim(const void* q, int32_t Lq, const void* docs, const int32_t* doc_off,
                         int32_t n_docs, int32_t H, int32_t dtype, int32_t mode, float* out,
                         int32_t device, void* stream) {
  if (n_docs == 0) return TS_OK;
  if (!q || !docs || !doc_off || !out || Lq < 0 || n_docs < 0 || H <= 0 || !dtype_ok(dtype) ||
      (mode != 0 && mode != 1)) {
    ts_set_error("bad arguments to maxsim");
    return TS_ERR_INVALID;
  }
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  const int st = ts_launch_maxsim16(q, Lq, docs, doc_off, nullptr, nullptr, n_docs, H, dtype, mode, out,
                                    device, (hipStream_t)stream);
  if (st != TS_ERR_UNSUPPORTED) return st;
  return ts_launch_maxsim(q, Lq, docs, doc_off, nullptr, nullptr, n_docs, H, dtype, mode, out,
                          (hipStream_t)stream);
}

extern "C" int ts_maxsim_indexed(const void* q, int32_t Lq, const void* store, const int64_t* starts,
                                 const int32_t* lens, int32_t n_docs, int32_t H, int32_t dtype,
                                 int32_t mode, float* out, int32_t device, void* stream) {
  if (n_docs == 0) return TS_OK;
  if (!q || !store || !starts || !lens || !out || Lq < 0 || n_docs < 0 || H <= 0 || !dtype_ok(dtype) ||
      (mode != 0 && mode != 1)) {
    ts_set_error("bad arguments to maxsim_indexed");
    return TS_ERR_INVALID;
  }
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  const int st = ts_launch_maxsim16(q, Lq, store, nullptr, starts, lens, n_docs, H, dtype, mode, out,
                                    device, (hipStream_t)stream);
  if (st != TS_ERR_UNSUPPORTED) return st;
  return ts_launch_maxsim(q, Lq, store, nullptr, starts, lens, n_docs, H, dtype, mode, out,
                          (hipStream_t)stream);
}

extern "C" int ts_maxsim_indexed_batch(const void* q, const int32_t* q_off, int32_t nq, const void* store,
                                       const int64_t* starts, const int32_t* lens, const int32_t* cand_off,
                                       int32_t H, int32_t dtype, int32_t mode, float* out, int32_t device,
                                       void* stream) {
  if (nq == 0) return TS_OK;
  if (!q || !q_off || !store || !starts || !lens || !cand_off || !out || nq < 0 || H <= 0 ||
      !dtype_ok(dtype) || (mode != 0 && mode != 1)) {
    ts_set_error("bad arguments to maxsim_indexed_batch");
    return TS_ERR_INVALID;
  }
  for (int j = 0; j < nq; ++j)
    if (q_off[j + 1] < q_off[j] || cand_off[j + 1] < cand_off[j]) {
      ts_set_error("maxsim_indexed_batch: offsets must be non-decreasing");
      return TS_ERR_INVALID;
    }
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  const int st = ts_launch_maxsim16_batch(q, q_off, nq, store, starts, lens, cand_off, H, dtype, mode, out,
                                          device, (hipStream_t)stream);
  if (st != TS_ERR_UNSUPPORTED) return st;
  // shapes the one-launch form does not take: query by query
  const size_t esize = (dtype == TS_F32) ? 4 : 2;
  for (int j = 0; j < nq; ++j) {
    const int nc = cand_off[j + 1] - cand_off[j];
    if (nc == 0) continue;
    TS_CHECK(ts_maxsim_indexed((const char*)q + (size_t)q_off[j] * H * esize, q_off[j + 1] - q_off[j], store,
                               starts + cand_off[j], lens + cand_off[j], nc, H, dtype, mode,
                               out + cand_off[j], device, stream));
  }
  return TS_OK;
}

// ---- e4m3 token store (include/tristage.h "stage-2 MaxSim over an e4m3 token store")
static bool fp8_query_dtype_ok(int dt) { return dt == TS_F16 || dt == TS_BF16; }

extern "C" int ts_maxsim_indexed_fp8(const void* q, int32_t q_dtype, int32_t Lq, const void* store,
                                     const int64_t* starts, const int32_t* lens, int32_t n_docs, int32_t H,
                                     int32_t mode, float* out, int32_t device, void* stream) {
  if (!q || !store || !starts || !lens || !out || Lq <= 0 || n_docs < 0 || H <= 0 || !fp8_query_dtype_ok(q_dtype) ||
      (mode != 0 && mode != 1)) {
    ts_set_error("bad arguments to maxsim_indexed_fp8");
    return TS_ERR_INVALID;
  }
  if (H % 16 != 0) {
    ts_set_error("maxsim_indexed_fp8: H = %d is not a multiple of 16", H);
    return TS_ERR_UNSUPPORTED;
  }
  if (n_docs == 0) return TS_OK;
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  const int st = ts_launch_maxsim16(q, Lq, store, nullptr, starts, lens, n_docs, H, TS_FP8_E4M3, mode, out,
                                    device, (hipStream_t)stream, q_dtype);
  if (st == TS_ERR_UNSUPPORTED)   // (no general kernel behind this one)
    ts_set_error("maxsim_indexed_fp8: H = %d, Lq = %d is not a shape the streaming kernel takes", H, Lq);
  return st;
}

extern "C" int ts_maxsim_indexed_batch_fp8(const void* q, int32_t q_dtype, const int32_t* q_off, int32_t nq,
                                           const void* store, const int64_t* starts, const int32_t* lens,
                                           const int32_t* cand_off, int32_t H, int32_t mode, float* out,
                                           int32_t device, void* stream) {
  if (!q || !q_off || !store || !starts || !lens || !cand_off || !out || nq < 0 || H <= 0 ||
      !fp8_query_dtype_ok(q_dtype) || (mode != 0 && mode != 1)) {
    ts_set_error("bad arguments to maxsim_indexed_batch_fp8");
    return TS_ERR_INVALID;
  }
  for (int j = 0; j < nq; ++j)
    if (q_off[j + 1] < q_off[j] || cand_off[j + 1] < cand_off[j]) {
      ts_set_error("maxsim_indexed_batch_fp8: offsets must be non-decreasing");
      return TS_ERR_INVALID;
    }
  if (H % 16 != 0) {
    ts_set_error("maxsim_indexed_batch_fp8: H = %d is not a multiple of 16", H);
    return TS_ERR_UNSUPPORTED;
  }
  if (nq == 0) return TS_OK;
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  const int st = ts_launch_maxsim16_batch(q, q_off, nq, store, starts, lens, cand_off, H, TS_FP8_E4M3, mode, out,
                                          device, (hipStream_t)stream, q_dtype);
  if (st != TS_ERR_UNSUPPORTED) return st;
  // shapes the one-launch form does not take (a query of > 4096 candidates): query by query
  for (int j = 0; j < nq; ++j) {
    const int nc = cand_off[j + 1] - cand_off[j];
    if (nc == 0) continue;
    TS_CHECK(ts_maxsim_indexed_fp8((const char*)q + (size_t)q_off[j] * H * 2, q_dtype, q_off[j + 1] - q_off[j],
                                   store, starts + cand_off[j], lens + cand_off[j], nc, H, mode, out + cand_off[j],
                                   device, stream));
  }
  return TS_OK;
}

extern "C" int ts_quantize_rows_fp8(const void* x, int32_t x_dtype, int64_t rows, int32_t H, void* out,
                                    int32_t device, void* stream) {
  if (!x || !out || rows < 0 || H <= 0 || !dtype_ok(x_dtype)) {
    ts_set_error("bad arguments to quantize_rows_fp8");
    return TS_ERR_INVALID;
  }
  if (H % 16 != 0 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15)) {
    ts_set_error("quantize_rows_fp8: needs H %% 16 == 0 (H = %d) and 16-byte aligned rows", H);
    return TS_ERR_UNSUPPORTED;
  }
  if (rows == 0) return TS_OK;
  TsDeviceGuard g(device);
  if (!g.ok) { ts_set_error("hipSetDevice(%d) failed", device); return TS_ERR_HIP; }
  return ts_launch_quantize_rows_fp8(x, x_dtype, rows, H, out, (hipStream_t)stream);
}
