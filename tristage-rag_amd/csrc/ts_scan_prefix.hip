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

template <int DT, int QH, int MODE>
int launch_prefix_t(const PrefixScanParams& p, int num_cus, hipStream_t stream) {
  const size_t lds = (size_t)p.kg * QH * 1024 + (MODE == SCAN_FILTER ? sizeof(StageLds) : 0);
  // as launch_scan_t (ts_scan.hip): the short dense scans take a second workgroup per CU when LDS allows
  const int wg_per_cu = (MODE == SCAN_DENSE && 2 * lds <= 160 * 1024) ? 2 : 1;
  return launch_scan_ring<QH, MODE, Op16<DT>, WalkStridedPrefix>(p, lds, ts_scan_grid(p.nwork, (int64_t)num_cus * wg_per_cu),
                                                                 stream);
}

template <int DT>
int launch_prefix_dt(int mode, int qh, const PrefixScanParams& p, int num_cus, hipStream_t s) {
  if (qh == 1) {
    return mode == SCAN_DENSE ? launch_prefix_t<DT, 1, SCAN_DENSE>(p, num_cus, s)
                              : launch_prefix_t<DT, 1, SCAN_FILTER>(p, num_cus, s);
  }
  return mode == SCAN_DENSE ? launch_prefix_t<DT, 2, SCAN_DENSE>(p, num_cus, s)
                            : launch_prefix_t<DT, 2, SCAN_FILTER>(p, num_cus, s);
}

// p.nwork: every row block (the live count is only known on the device; waves past it leave at once)
template <int DT, int QH>
int launch_prefix_masked_t(const PrefixMaskedScanParams& p, int num_cus, hipStream_t stream) {
  return launch_scan_ring<QH, SCAN_FILTER, Op16<DT>, WalkLivePrefix>(p, (size_t)p.kg * QH * 1024 + sizeof(StageLds),
                                                                    ts_scan_grid(p.nwork, num_cus), stream);
}

int prefix_check(const TsLayout& L, int qh, int kg, int kg_row) {
  if (L.dtype != TS_F16 && L.dtype != TS_BF16) {
    ts_set_error("the prefix scan takes f16 / bf16 storage only");
    return TS_ERR_UNSUPPORTED;
  }
  if (kg < TS_RING || kg % TS_RING != 0 || kg > kg_row || kg_row != L.kg || (qh != 1 && qh != 2)) {
    ts_set_error("prefix scan: %d of %d k groups, %d query halves", kg, kg_row, qh);
    return TS_ERR_INVALID;
  }
  if ((size_t)kg * qh * 1024 + sizeof(StageLds) > 160 * 1024) {
    ts_set_error("prefix of %d dimensions too large for the LDS-resident query image", kg * 16);
    return TS_ERR_UNSUPPORTED;
  }
  return TS_OK;
}

}  // namespace

int ts_launch_scan_prefix(const TsLayout& L, int mode, int qh, const PrefixScanParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  TS_CHECK(prefix_check(L, qh, p.kg, p.kg_row));
  return L.dtype == TS_F16 ? launch_prefix_dt<TS_F16>(mode, qh, p, num_cus, stream)
                           : launch_prefix_dt<TS_BF16>(mode, qh, p, num_cus, stream);
}

int ts_launch_scan_prefix_masked(const TsLayout& L, int qh, const PrefixMaskedScanParams& p, int num_cus,
                                 hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  TS_CHECK(prefix_check(L, qh, p.kg, p.kg_row));
  if (L.dtype == TS_F16)
    return qh == 1 ? launch_prefix_masked_t<TS_F16, 1>(p, num_cus, stream) : launch_prefix_masked_t<TS_F16, 2>(p, num_cus, stream);
  return qh == 1 ? launch_prefix_masked_t<TS_BF16, 1>(p, num_cus, stream) : launch_prefix_masked_t<TS_BF16, 2>(p, num_cus, stream);
}
