// e4m3-storage scan (TS_FP8_E4M3 flat index, gfx950): one byte per corpus element, scored in place.
//
// Format: element x of an index with scale exponent s is the byte e4m3fn_rne(x * 2^s) (fp8_quantize below: round to
// nearest even on the f32 bits, e4m3 subnormals kept, |x * 2^s| > 448 and Inf saturate to +-448, NaN -> 0x7F).  One
// fixed power of two per index and no per-row scale: stage-1 scores are compared across rows.
//
// Layout (ts_common.h): a 16-byte unit of lane h*32 + r in k group g holds k = 32g + 16m + 8h + j (m = 0/1, j = 0..7),
// so bytes 0-7 / 8-15, converted in registers with v_cvt_scalef32_pk_bf16_fp8 (every e4m3 value is exact in bf16), are
// the A fragments of k steps 2g / 2g + 1 of v_mfma_f32_32x32x16_bf16.  The query image is the bf16 image of a bf16
// layout of the same padded dimension (unit ((2g + m) * QH + hq) * 64 + l), holding the queries rounded to bf16 and
// multiplied by 2^-s (exact), so that the accumulators hold final scores and everything behind them (sample,
// thresholds, candidate lists, selects, masks) is what it is for the 16-bit scans.  A score equals, bit for bit, the
// score of a bf16 index that holds the decoded rows: the same operands up to the power of two, the same k order.
//
// The scans are scan_kernel (ts_scan_dev.h) with OpFp8 below, over WalkStrided or, for filtered searches, WalkLive:
// a ring slot feeds two MFMAs per query half, and the image is twice an Op16 image.
#include "ts_scan_dev.h"

__device__ __forceinline__ uint32_t fp8_pair_bf16(uint32_t w, bool hi) {
  return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true))
            : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
}

// the eight bytes (w0, w1) -> the bf16 A fragment of one k step
__device__ __forceinline__ u32x4 fp8_frag(uint32_t w0, uint32_t w1) {
  u32x4 o;
  o[0] = fp8_pair_bf16(w0, false);
  o[1] = fp8_pair_bf16(w0, true);
  o[2] = fp8_pair_bf16(w1, false);
  o[3] = fp8_pair_bf16(w1, true);
  return o;
}

// one ring slot (k group g) against the image: k steps 2g and 2g + 1 of every query half
template <int QH>
__device__ __forceinline__ void fp8_slot(f32x16 (&acc)[QH], const u32x4& a, const u32x4* ql, int g) {
  const u32x4 a0 = fp8_frag(a[0], a[1]);
#pragma unroll
  for (int hq = 0; hq < QH; ++hq) {
    const u32x4 b = ql[(size_t)((2 * g) * QH + hq) * 64];
    mma_group<TS_BF16>(acc[hq], a0, b);
  }
  const u32x4 a1 = fp8_frag(a[2], a[3]);
#pragma unroll
  for (int hq = 0; hq < QH; ++hq) {
    const u32x4 b = ql[(size_t)((2 * g + 1) * QH + hq) * 64];
    mma_group<TS_BF16>(acc[hq], a1, b);
  }
}

struct OpFp8 {
  typedef StageLds Stage;
  template <int QH> static __device__ __forceinline__ int image_kib(int kg) { return 2 * kg * QH; }
  template <int QH>
  static __device__ __forceinline__ void step(f32x16 (&acc)[QH], const u32x4 (&ring)[TS_RING], int i, const u32x4* ql, int g) {
    fp8_slot<QH>(acc, ring[i], ql, g);
  }
};

size_t ts_scan_fp8_lds_bytes(const TsLayout& L, int qh) {
  return (size_t)2 * L.kg * qh * 1024 + sizeof(StageLds);
}

int ts_launch_scan_fp8(const TsLayout& L, int mode, int qh, const ScanParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (L.dtype != TS_FP8_E4M3 || p.kg != L.kg || (qh != 1 && qh != 2) || ts_scan_fp8_lds_bytes(L, qh) > TS_LDS_BYTES) {
    ts_set_error("e4m3 scan: dimension %d does not fit the LDS-resident query image for %d queries", L.dim, 32 * qh);
    return TS_ERR_UNSUPPORTED;
  }
  return launch_scan<OpFp8, WalkStrided>(mode, qh, 2 * L.kg, p, num_cus, stream);
}

int ts_launch_scan_masked_fp8(const TsLayout& L, int qh, const MaskedScanParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (L.dtype != TS_FP8_E4M3 || p.kg != L.kg || (qh != 1 && qh != 2) || ts_scan_fp8_lds_bytes(L, qh) > TS_LDS_BYTES) {
    ts_set_error("e4m3 masked scan: dimension %d does not fit the LDS-resident query image for %d queries", L.dim,
                 32 * qh);
    return TS_ERR_UNSUPPORTED;
  }
  return launch_scan<OpFp8, WalkLive>(SCAN_FILTER, qh, 2 * L.kg, p, num_cus, stream);
}

// ------------------------------------------------------------------ query image
// thread per 16-byte unit: unit (G * qh + hq) * 64 + l = query 32 hq + (l & 31), k = 16 G + 8 (l >> 5) + 0..7 (the
// bf16 image), each value bf16_rne(q) * 2^-s (exact: a power of two times a bf16 value, far above the subnormals)
template <typename TIN>
__global__ void qprep_fp8_kernel(const TIN* q, int nq, int dim, int ng, int qh, float inv_scale, uint4* qimg,
                                 uint32_t* cand_cnt, uint32_t* status) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < TS_MAX_Q && cand_cnt) cand_cnt[t] = 0;
  if (t == 0 && status) status[0] = 0;
  if (t >= ng * qh * 64) return;
  const int lane = t & 63;
  const int hq = (t >> 6) % qh;
  const int G = (t >> 6) / qh;
  const int qi = hq * 32 + (lane & 31), h = lane >> 5;
  const TIN* src = q + (int64_t)qi * dim;
  uint32_t b[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = 16 * G + 8 * h + e;
    const float x = (qi < nq && k < dim) ? ElemIO<TIN>::ld(src + k) : 0.f;
    const float r = __builtin_bit_cast(float, (uint32_t)f32_to_storage16(x, TS_BF16) << 16) * inv_scale;
    b[e] = __builtin_bit_cast(uint32_t, r) >> 16;
  }
  u32x4 out;
#pragma unroll
  for (int d = 0; d < 4; ++d) out[d] = b[2 * d] | (b[2 * d + 1] << 16);
  reinterpret_cast<u32x4*>(qimg)[t] = out;
}

static float fp8_pow2(int e) { return __builtin_bit_cast(float, (uint32_t)(127 + e) << 23); }

int ts_launch_qprep_fp8(const TsLayout& L, const void* q, int q_dtype, int nq, int qh, uint4* qimg, uint32_t* cand_cnt,
                        uint32_t* status, hipStream_t stream) {
  const int ng = 2 * L.kg;
  const int units = ng * qh * 64;
  const int blocks = (units + 255) / 256;
  const float inv = fp8_pow2(-L.fp8_scale_log2);
  return ts_typed_queries(q, q_dtype, [&](auto* qt) -> int {
    typedef typename TsPointee<decltype(qt)>::type TIN;
    hipLaunchKernelGGL(qprep_fp8_kernel<TIN>, dim3(blocks), dim3(256), 0, stream, qt, nq, L.dim, ng, qh, inv, qimg,
                       cand_cnt, status);
    TS_HIP(hipGetLastError());
    return TS_OK;
  });
}

// ------------------------------------------------------------------ layout
// e4m3fn_rne(y) on the bits of y (index.py quantize_rows_e4m3_fixed_reference is the definition)
__device__ __forceinline__ uint32_t fp8_quantize(float y) {
  const uint32_t u = __builtin_bit_cast(uint32_t, y);
  const uint32_t sign = (u >> 24) & 0x80u;
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return 0x7Fu;                 // NaN
  const uint32_t e = a >> 23;
  if (e >= 121u) {                                    // |y| >= 2^-6: an e4m3 normal; 20 mantissa bits dropped
    const uint32_t r = (a + 0x7FFFFu + ((a >> 20) & 1u)) >> 20;
    const uint32_t b = r - 960u;                      // exponent bias 127 -> 7
    return sign | (b > 0x7Eu ? 0x7Eu : b);            // above 448 (Inf too): +-448
  }
  if (e < 117u) return sign;                          // |y| < 2^-10: below half of the subnormal step 2^-9
  // subnormal: round(|y| * 2^9) to nearest even, 0 .. 8 (8 is the byte of 2^-6)
  const uint32_t m = (a & 0x7fffffu) | 0x800000u;
  const uint32_t sh = 141u - e;                       // 21 .. 24
  uint32_t qv = m >> sh;
  const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
  qv += (rem > half || (rem == half && (qv & 1u))) ? 1u : 0u;
  return sign | qv;
}

__device__ __forceinline__ float fp8_decode(uint32_t b) {
  const uint32_t sign = (b & 0x80u) << 24, e = (b >> 3) & 15u, m = b & 7u;
  if ((b & 0x7Fu) == 0x7Fu) return __builtin_bit_cast(float, sign | 0x7fc00000u);
  if (e == 0u) return __builtin_bit_cast(float, sign | __builtin_bit_cast(uint32_t, (float)m * 0.001953125f));
  return __builtin_bit_cast(float, sign | ((e + 120u) << 23) | (m << 20));
}

// One wave per (row block, k group): 64 lanes write one contiguous 1 KiB unit row (relayout_kernel's walk).  With
// `den` the quantiser takes the f32 quotient v / den, as the other storage types do.
template <typename TIN>
__global__ void relayout_fp8_kernel(const TIN* rows, int64_t n, int dim, int64_t row0, int64_t blk_first,
                                    int64_t nunits_wave, uint4* tiled, int kg, float scale, const float* den, int vec) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= nunits_wave) return;
  const int64_t b = blk_first + wv / kg;
  const int g = (int)(wv % kg);
  const int r = lane & 31, h = lane >> 5;
  const int64_t row = b * TS_ROWS_PER_BLOCK + r;
  if (row < row0 || row >= row0 + n) return;
  const TIN* src = rows + (row - row0) * dim;
  const float d = den ? den[row - row0] : 1.0f;
  u32x4 out;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int k0 = 32 * g + 16 * m + 8 * h;
    float v[8];
    if (vec && k0 < dim) {   // (dim % 8 == 0: the eight values are inside the row)
      ld8<TIN>(src + k0, v);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (k0 + e < dim) ? ElemIO<TIN>::ld(src + k0 + e) : 0.f;
    }
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x = v[e];
      if (den) x = x / d;
      w[e >> 2] |= fp8_quantize(x * scale) << (8 * (e & 3));
    }
    out[2 * m] = w[0];
    out[2 * m + 1] = w[1];
  }
  reinterpret_cast<u32x4*>(tiled)[(size_t)(b * kg + g) * 64 + lane] = out;
}

int ts_launch_relayout_fp8(const TsLayout& L, const void* rows, int in_dtype, int64_t n, int64_t row0, uint4* tiled,
                           bool normalize, float* den_scratch, hipStream_t stream) {
  if (n <= 0) return TS_OK;
  if (normalize) TS_CHECK(ts_launch_row_den(rows, in_dtype, n, L.dim, den_scratch, stream));
  return ts_typed_rows(rows, in_dtype, [&](auto* r) -> int {
    typedef typename TsPointee<decltype(r)>::type TIN;
    TsRelayoutGeom g;
    TS_CHECK(ts_relayout_geom(L.dim, L.kg, r, sizeof(TIN), row0, n, g));
    hipLaunchKernelGGL(relayout_fp8_kernel<TIN>, dim3(g.blocks), dim3(256), 0, stream, r, n, L.dim, row0, g.blk_first,
                       g.nwave, tiled, L.kg, fp8_pow2(L.fp8_scale_log2),
                       normalize ? den_scratch : (const float*)nullptr, g.vec);
    TS_HIP(hipGetLastError());
    return TS_OK;
  });
}

// thread per (row, 16-byte unit): the decoded values e4m3 * 2^-s (exact in f32)
__global__ void reconstruct_fp8_kernel(const uint4* tiled, int64_t row0, int64_t n, int dim, int kg, float inv_scale,
                                       float* out) {
  const int upr = kg * 2;  // units per row
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * upr) return;
  const int64_t row = row0 + t / upr;
  const int u = (int)(t % upr);
  const int g = u >> 1, h = u & 1;
  const int64_t b = row / TS_ROWS_PER_BLOCK;
  const int lane = h * 32 + (int)(row % TS_ROWS_PER_BLOCK);
  const u32x4 v = reinterpret_cast<const u32x4*>(tiled)[(size_t)(b * kg + g) * 64 + lane];
  float* dst = out + (row - row0) * dim;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int k = 32 * g + 16 * (e >> 3) + 8 * h + (e & 7);
    const uint32_t byte = (v[e >> 2] >> (8 * (e & 3))) & 0xFFu;
    if (k < dim) dst[k] = fp8_decode(byte) * inv_scale;
  }
}

int ts_launch_reconstruct_fp8(const TsLayout& L, const uint4* tiled, int64_t row0, int64_t n, float* out,
                              hipStream_t stream) {
  if (n <= 0) return TS_OK;
  unsigned blocks;
  TS_CHECK(ts_reconstruct_blocks(n, L.kg, blocks));
  hipLaunchKernelGGL(reconstruct_fp8_kernel, dim3(blocks), dim3(256), 0, stream, tiled, row0, n, L.dim, L.kg,
                     fp8_pow2(-L.fp8_scale_log2), out);
  TS_HIP(hipGetLastError());
  return TS_OK;
}
