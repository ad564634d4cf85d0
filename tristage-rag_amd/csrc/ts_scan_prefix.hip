// Prefix scans (ts_index_search_prefix): the ring scan of ts_scan_dev.h over the first p.kg k groups
// of every row block.  A row block is p.kg_row KiB long and its k groups lie in ascending order, so the first
// dims = 16 p.kg dimensions of its 32 rows are its first p.kg KiB: the walks below are the strided and the live-list
// walk with the row blocks p.kg_row groups apart, and everything else is scan_kernel as it stands, with the query image
// of a p.kg-group layout.  p.kg is a multiple of TS_RING (dims % 128 == 0); at p.kg == TS_RING the main loop of
// scan_kernel is empty and the tail, which refills the ring from the next row block, is the whole block.
#include "ts_scan_dev.h"

namespace {

struct WalkStridedPrefix : WalkStrided {
  typedef PrefixScanParams Params;
  static __device__ __forceinline__ int row_groups(const Params& p) { return p.kg_row; }
};

struct WalkLivePrefix : WalkLive {
  typedef PrefixMaskedScanParams Params;
  static __device__ __forceinline__ int row_groups(const Params& p) { return p.kg_row; }
};

int prefix_check(const TsLayout& L, int qh, int kg, int kg_row) {
  if (L.dtype != TS_F16 && L.dtype != TS_BF16) {
    ts_set_error("the prefix scan takes f16 / bf16 storage only");
    return TS_ERR_UNSUPPORTED;
  }
  if (kg < TS_RING || kg % TS_RING != 0 || kg > kg_row || kg_row != L.kg || (qh != 1 && qh != 2)) {
    ts_set_error("prefix scan: %d of %d k groups, %d query halves", kg, kg_row, qh);
    return TS_ERR_INVALID;
  }
  if ((size_t)kg * qh * 1024 + sizeof(StageLds) > TS_LDS_BYTES) {
    ts_set_error("prefix of %d dimensions too large for the LDS-resident query image", kg * 16);
    return TS_ERR_UNSUPPORTED;
  }
  return TS_OK;
}

}  // namespace

int ts_launch_scan_prefix(const TsLayout& L, int mode, int qh, const PrefixScanParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  TS_CHECK(prefix_check(L, qh, p.kg, p.kg_row));
  return L.dtype == TS_F16 ? launch_scan<Op16<TS_F16>, WalkStridedPrefix>(mode, qh, p.kg, p, num_cus, stream)
                           : launch_scan<Op16<TS_BF16>, WalkStridedPrefix>(mode, qh, p.kg, p, num_cus, stream);
}

int ts_launch_scan_prefix_masked(const TsLayout& L, int qh, const PrefixMaskedScanParams& p, int num_cus,
                                 hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  TS_CHECK(prefix_check(L, qh, p.kg, p.kg_row));
  return L.dtype == TS_F16 ? launch_scan<Op16<TS_F16>, WalkLivePrefix>(SCAN_FILTER, qh, p.kg, p, num_cus, stream)
                           : launch_scan<Op16<TS_BF16>, WalkLivePrefix>(SCAN_FILTER, qh, p.kg, p, num_cus, stream);
}
