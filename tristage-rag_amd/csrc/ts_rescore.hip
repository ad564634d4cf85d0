// Exact full-dimension scores of given candidates (ts_index_rescore).
//
// The candidates' rows have been gathered into per-query 32-candidate tiles in fragment order (mmr_gather_kernel,
// ts_mmr.hip), so a tile is the A operand of the scan's MFMA and the pass's query image its B operand.  One wave per
// tile accumulates the kg k groups in ascending order, exactly as scan_kernel does for a row block, and keeps the
// column of its own query: a column of a 32x32 MFMA depends on that column of B only, so the numbers are the scan's,
// bit for bit.  The 31 other columns are computed and dropped; the kernel is bound by its two 1 KiB loads per group,
// both from L2 (the tile was just written, the image is shared by every wave).
#include "ts_scan_dev.h"

namespace {

constexpr int kRescoreRing = 4;   // k groups a wave keeps in flight (divides TS_RING)
static_assert(TS_RING % kRescoreRing == 0, "kg is a multiple of TS_RING");

// grid (ceil(cbp / 4), nq), 4 waves: wave w of workgroup x owns tile 4 x + w of query blockIdx.y
template <int DT>
__global__ __launch_bounds__(256) void rescore_kernel(TsRescoreParams p) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= p.cbp) return;   // wave-uniform
  const int64_t q = blockIdx.y;
  const int col = p.col0 + (int)q;
  const u32x4* pa = reinterpret_cast<const u32x4*>(p.tile) + (q * p.cbp + b) * p.kg * 64 + lane;
  // unit (g * qh + hq) * 64 + l of the image holds, for query 32 hq + (l & 31), the k's of group g
  const u32x4* pb = reinterpret_cast<const u32x4*>(p.qimg) + (col >> 5) * 64 + lane;
  const int64_t bstep = (int64_t)p.qh * 64;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  u32x4 ra[kRescoreRing], rb[kRescoreRing];
#pragma unroll
  for (int i = 0; i < kRescoreRing; ++i) {
    ra[i] = pa[(int64_t)i * 64];
    rb[i] = pb[(int64_t)i * bstep];
  }
  for (int g0 = 0; g0 < p.kg; g0 += kRescoreRing) {
#pragma unroll
    for (int i = 0; i < kRescoreRing; ++i) {
      mma_group<DT>(acc, ra[i], rb[i]);   // k group g0 + i: ascending order
      const int gn = g0 + kRescoreRing + i;
      if (gn < p.kg) {
        ra[i] = pa[(int64_t)gn * 64];
        rb[i] = pb[(int64_t)gn * bstep];
      }
    }
  }
  if ((lane & 31) != (col & 31)) return;
  const int32_t* valid = p.valid + (q * p.cbp + b) * 32;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, lane);
    const int c = b * 32 + row;
    if (c < p.C) {
      const bool ok = valid[row] != 0;
      p.scores[q * p.C + c] = ok ? acc[r] : -3.402823466e38f;
      p.ids_out[q * p.C + c] = ok ? p.ids[q * p.C + c] : -1;
    }
  }
}

}  // namespace

int ts_launch_rescore(const TsLayout& L, const TsRescoreParams& p, int nq, hipStream_t stream) {
  if (nq <= 0 || p.cbp <= 0) return TS_OK;
  if (p.kg != L.kg || p.kg % kRescoreRing != 0 || (p.qh != 1 && p.qh != 2) || p.col0 < 0 || p.col0 + nq > 32 * p.qh ||
      p.C < 1 || p.C > 32 * p.cbp) {
    ts_set_error("rescore: bad launch parameters");
    return TS_ERR_INVALID;
  }
  const dim3 grid((unsigned)((p.cbp + 3) / 4), (unsigned)nq);
  if (L.dtype == TS_F16) hipLaunchKernelGGL(rescore_kernel<TS_F16>, grid, dim3(256), 0, stream, p);
  else if (L.dtype == TS_BF16) hipLaunchKernelGGL(rescore_kernel<TS_BF16>, grid, dim3(256), 0, stream, p);
  else { ts_set_error("rescore takes f16 / bf16 storage only"); return TS_ERR_UNSUPPORTED; }
  TS_HIP(hipGetLastError());
  return TS_OK;
}
