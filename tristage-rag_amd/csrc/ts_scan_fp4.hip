// 4-bit MX storage scan (TS_MXFP4_E2M1 flat index, gfx950): OCP e2m1 elements with one E8M0 scale per 32 elements,
// scored in place.
//
// Format (index.py quantize_rows_mxfp4_reference is the definition): a row is zero-padded to a multiple of 64; scale
// block (g, h) holds the 32 dimensions k = 64g + 16m + 8h + j (m = 0..3, j = 0..7), the dimensions lane h*32 + r feeds
// to k steps 4g .. 4g+3 of v_mfma_f32_32x32x16_bf16.  Its exponent e is floor(log2 amax) - 2, plus one when
// amax > 6 * 2^e, clamped to -100 .. 100 (0 for a zero block), stored as e + 127; an element is its sign bit and the
// index of the value of {0, 0.5, 1, 1.5, 2, 3, 4, 6} nearest to |x| / 2^e, ties to the even index.
//
// Layout (ts_common.h): a row block is NS scale units and then NG = dpad / 64 code units of 1 KiB, dpad a multiple of
// 256 (d = 768: 1 + 12 KiB).  Nibble j of dword m of lane l's 16 bytes in code unit g is element k above; byte g % 16
// of lane l's 16 bytes in scale unit g / 16 is the scale byte of block (g, l >> 5).  Update, compaction and the
// gathers move lane l's 16 bytes of all KG = NS + NG units, so a row's scale bytes travel with its codes.
//
// The scans are scan_kernel (ts_scan_dev.h) with OpFp4 over walks whose row blocks are KG units apart; the ring
// (TS_RING = 4 here: 12 code units are three turns) streams the code units only.  A lane's scale bytes of the next
// row block are requested beside the mask words, just before the tail's ring loads, by two unpredicated 16-byte loads
// (scale_fetch), so they never drain the ring.  Dword m of a slot becomes the A fragment of k step 4g + m by four
// v_cvt_scalef32_pk_bf16_fp4 with the lane's 2^e, and meets the plain bf16 query image (unit ((4g + m) * QH + hq) * 64
// + l).  A score equals, bit for bit, that of a bf16 index holding the decoded rows: the same operands, the same k
// order; the zero k steps of the wider padding add nothing.
// TS_RING is this unit's alone: ts_make_layout pads by it, so the layout builder is compiled out here and every layout
// is one the caller built with the library's TS_RING.  No host helper below depends on TS_RING.
#define TS_RING 4
#define TS_NO_LAYOUT_BUILDER
#include "ts_scan_dev.h"

static_assert(TS_RING == 4, "OpFp4: one dword of scale bytes per ring turn");

// dword w (8 nibbles) -> the bf16 A fragment of one k step, each value times scale (a power of two)
__device__ __forceinline__ u32x4 fp4_frag(uint32_t w, float scale) {
  u32x4 o;
  o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
  o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
  o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
  o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
  return o;
}

struct OpFp4 {
  typedef StageLds Stage;
  static constexpr bool kScaled = true;
  template <int QH> static __device__ __forceinline__ int image_kib(int kg) { return 4 * kg * QH; }
  // blk_ptr: the lane's 16 bytes of the row block's first code unit; the NS = ceil(kg / 16) scale units lie just before
  // it.  sc[0] is the first scale unit, sc[1] the last (the same one when NS == 1).
  static __device__ __forceinline__ void scale_fetch(const u32x4* blk_ptr, int kg, u32x4 (&sc)[2]) {
    const int ns = (kg + 15) >> 4;
    sc[0] = stream_load(blk_ptr - (size_t)ns * 64);
    sc[1] = stream_load(blk_ptr - 64);
  }
  // the scale bytes of code units g0 .. g0 + 3 (g0 a multiple of 4, below 32): explicit selects, no indexed registers
  static __device__ __forceinline__ uint32_t scale_word(const u32x4 (&sc)[2], int g0) {
    const int j = g0 >> 2;
    uint32_t w = sc[0][0];
    w = (j == 1) ? sc[0][1] : w;
    w = (j == 2) ? sc[0][2] : w;
    w = (j == 3) ? sc[0][3] : w;
    w = (j == 4) ? sc[1][0] : w;
    w = (j == 5) ? sc[1][1] : w;
    w = (j == 6) ? sc[1][2] : w;
    w = (j == 7) ? sc[1][3] : w;
    return w;
  }
  // ring slot i (code unit g) against the image: k steps 4g .. 4g + 3 of every query half
  template <int QH>
  static __device__ __forceinline__ void step_scaled(f32x16 (&acc)[QH], const u32x4 (&ring)[TS_RING], int i,
                                                     const u32x4* ql, int g, uint32_t sw) {
    const float scale = __builtin_bit_cast(float, ((sw >> (8 * i)) & 0xFFu) << 23);   // 2^e: the byte is e + 127
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const u32x4 a = fp4_frag(ring[i][m], scale);
#pragma unroll
      for (int hq = 0; hq < QH; ++hq) {
        const u32x4 b = ql[(size_t)((4 * g + m) * QH + hq) * 64];
        mma_group<TS_BF16>(acc[hq], a, b);
      }
    }
  }
};

// p.kg code units are scanned of row blocks that lie p.kg + NS units apart
struct WalkStridedFp4 : WalkStrided {
  static __device__ __forceinline__ int row_groups(const Params& p) { return p.kg + ((p.kg + 15) >> 4); }
};
struct WalkLiveFp4 : WalkLive {
  static __device__ __forceinline__ int row_groups(const Params& p) { return p.kg + ((p.kg + 15) >> 4); }
};

size_t ts_scan_fp4_lds_bytes(const TsLayout& L, int qh) {
  return (size_t)L.qkg * qh * 1024 + sizeof(StageLds);
}

static bool fp4_scan_ok(const TsLayout& L, int kg, int qh) {
  return L.dtype == TS_MXFP4_E2M1 && kg == L.kg && (qh == 1 || qh == 2) && ts_fp4_code_groups(L) % TS_RING == 0 &&
         ts_fp4_code_groups(L) <= 32 && ts_scan_fp4_lds_bytes(L, qh) <= TS_LDS_BYTES;
}

// the kernel's view of the corpus: p.corpus at the first code unit of row block 0, p.kg the code units of a row block
template <class P>
static P fp4_params(const TsLayout& L, const P& p) {
  P q = p;
  q.corpus = p.corpus + (size_t)ts_fp4_scale_units(L) * 64;
  q.kg = ts_fp4_code_groups(L);
  return q;
}

int ts_launch_scan_fp4(const TsLayout& L, int mode, int qh, const ScanParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (!fp4_scan_ok(L, p.kg, qh)) {
    ts_set_error("mxfp4 scan: dimension %d does not fit the LDS-resident query image for %d queries", L.dim, 32 * qh);
    return TS_ERR_UNSUPPORTED;
  }
  return launch_scan<OpFp4, WalkStridedFp4>(mode, qh, L.qkg, fp4_params(L, p), num_cus, stream);
}

int ts_launch_scan_masked_fp4(const TsLayout& L, int qh, const MaskedScanParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (!fp4_scan_ok(L, p.kg, qh)) {
    ts_set_error("mxfp4 masked scan: dimension %d does not fit the LDS-resident query image for %d queries", L.dim,
                 32 * qh);
    return TS_ERR_UNSUPPORTED;
  }
  return launch_scan<OpFp4, WalkLiveFp4>(SCAN_FILTER, qh, L.qkg, fp4_params(L, p), num_cus, stream);
}

// ------------------------------------------------------------------ query image
// the bf16 image of the padded dimension: the e4m3 index's qprep kernel with scale 2^0 (ts_scan_fp8.hip)
int ts_launch_qprep_fp4(const TsLayout& L, const void* q, int q_dtype, int nq, int qh, uint4* qimg, uint32_t* cand_cnt,
                        uint32_t* status, hipStream_t stream) {
  TsLayout Q = L;
  Q.kg = L.qkg / 2;   // (ts_launch_qprep_fp8 writes 2 * kg units per 32 queries)
  Q.fp8_scale_log2 = 0;
  return ts_launch_qprep_fp8(Q, q, q_dtype, nq, qh, qimg, cand_cnt, status, stream);
}

// ------------------------------------------------------------------ layout
// NaN counts as 0, +-Inf as +-FLT_MAX
__device__ __forceinline__ float fp4_clean(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x), a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return 0.f;
  if (a == 0x7f800000u) return __builtin_bit_cast(float, (u & 0x80000000u) | 0x7f7fffffu);
  return x;
}

// the block exponent of amax (finite, >= 0), from its f32 bits
__device__ __forceinline__ int fp4_block_exp(float amax) {
  const uint32_t a = __builtin_bit_cast(uint32_t, amax);
  if (a == 0u) return 0;
  // floor(log2 amax) - 2; amax > 6 * 2^e = 1.5 * 2^floor(log2 amax) adds one.  (An f32 subnormal gives -129 here
  // instead of its true value: both clamp to -100.)
  int e = (int)(a >> 23) - 127 - 2 + ((a & 0x7fffffu) > 0x400000u ? 1 : 0);
  return e < -100 ? -100 : (e > 100 ? 100 : e);
}

// the 3-bit index of the grid value nearest to y >= 0, ties to the even index, values above 6 -> 7 (the index of 6)
__device__ __forceinline__ uint32_t fp4_index(float y) {
  return (uint32_t)(y > 0.25f) + (uint32_t)(y >= 0.75f) + (uint32_t)(y > 1.25f) + (uint32_t)(y >= 1.75f) +
         (uint32_t)(y > 2.5f) + (uint32_t)(y >= 3.5f) + (uint32_t)(y > 5.0f);
}

// sign * grid[index] * 2^e, from integer operations (exact in f32 and bf16)
__device__ __forceinline__ float fp4_decode(uint32_t code, int e) {
  const uint32_t sign = (code & 8u) << 28, idx = code & 7u;
  if (idx == 0u) return __builtin_bit_cast(float, sign);
  // 0.5 = 1.0 * 2^-1; index 2 + 2t + m is (1 + m / 2) * 2^t
  const int ex = idx == 1u ? -1 : (int)(idx >> 1) - 1;
  const uint32_t man = idx == 1u ? 0u : (idx & 1u);
  return __builtin_bit_cast(float, sign | ((uint32_t)(127 + e + ex) << 23) | (man << 22));
}

__device__ __forceinline__ float fp4_pow2(int e) { return __builtin_bit_cast(float, (uint32_t)(127 + e) << 23); }

// One wave per (row block, code unit): a lane holds exactly one scale block, so amax needs no cross-lane step.  64
// lanes write one contiguous 1 KiB code unit and each its scale byte.  With `den` the quantiser takes the f32 quotient
// v / den, as the other storage types do.
template <typename TIN>
__global__ void relayout_fp4_kernel(const TIN* rows, int64_t n, int dim, int64_t row0, int64_t blk_first,
                                    int64_t nunits_wave, uint4* tiled, int ng, int ns, const float* den, int vec) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= nunits_wave) return;
  const int64_t b = blk_first + wv / ng;
  const int g = (int)(wv % ng);
  const int r = lane & 31, h = lane >> 5;
  const int64_t row = b * TS_ROWS_PER_BLOCK + r;
  if (row < row0 || row >= row0 + n) return;
  const TIN* src = rows + (row - row0) * dim;
  const float d = den ? den[row - row0] : 1.0f;
  float x[32];
  float amax = 0.f;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int k0 = 64 * g + 16 * m + 8 * h;
    float v[8];
    if (vec && k0 < dim) {   // (dim % 8 == 0: the eight values are inside the row)
      ld8<TIN>(src + k0, v);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (k0 + e < dim) ? ElemIO<TIN>::ld(src + k0 + e) : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = v[e];
      if (den) t = t / d;
      t = fp4_clean(t);
      x[8 * m + e] = t;
      amax = fmaxf(amax, fabsf(t));
    }
  }
  const int be = fp4_block_exp(amax);
  const float inv = fp4_pow2(-be);
  u32x4 out;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    uint32_t w = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = x[8 * m + e];
      const uint32_t code = ((__builtin_bit_cast(uint32_t, t) >> 28) & 8u) | fp4_index(fabsf(t) * inv);
      w |= code << (4 * e);
    }
    out[m] = w;
  }
  const size_t blk_unit = (size_t)b * (ng + ns);
  reinterpret_cast<u32x4*>(tiled)[(blk_unit + ns + g) * 64 + lane] = out;
  reinterpret_cast<uint8_t*>(tiled)[((blk_unit + (g >> 4)) * 64 + lane) * 16 + (g & 15)] = (uint8_t)(be + 127);
}

int ts_launch_relayout_fp4(const TsLayout& L, const void* rows, int in_dtype, int64_t n, int64_t row0, uint4* tiled,
                           bool normalize, float* den_scratch, hipStream_t stream) {
  if (n <= 0) return TS_OK;
  if (normalize) TS_CHECK(ts_launch_row_den(rows, in_dtype, n, L.dim, den_scratch, stream));
  const int ng = ts_fp4_code_groups(L), ns = ts_fp4_scale_units(L);
  return ts_typed_rows(rows, in_dtype, [&](auto* r) -> int {
    typedef typename TsPointee<decltype(r)>::type TIN;
    TsRelayoutGeom g;
    TS_CHECK(ts_relayout_geom(L.dim, ng, r, sizeof(TIN), row0, n, g));
    hipLaunchKernelGGL(relayout_fp4_kernel<TIN>, dim3(g.blocks), dim3(256), 0, stream, r, n, L.dim, row0, g.blk_first,
                       g.nwave, tiled, ng, ns, normalize ? den_scratch : (const float*)nullptr, g.vec);
    TS_HIP(hipGetLastError());
    return TS_OK;
  });
}

// thread per (row, code unit, lane half): the 32 decoded values of one scale block, by integer operations
__global__ void reconstruct_fp4_kernel(const uint4* tiled, int64_t row0, int64_t n, int dim, int ng, int ns,
                                       float* out) {
  const int upr = ng * 2;  // scale blocks per row
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * upr) return;
  const int64_t row = row0 + t / upr;
  const int u = (int)(t % upr);
  const int g = u >> 1, h = u & 1;
  const int64_t b = row / TS_ROWS_PER_BLOCK;
  const int lane = h * 32 + (int)(row % TS_ROWS_PER_BLOCK);
  const size_t blk_unit = (size_t)b * (ng + ns);
  const u32x4 v = reinterpret_cast<const u32x4*>(tiled)[(blk_unit + ns + g) * 64 + lane];
  const int e = (int)reinterpret_cast<const uint8_t*>(tiled)[((blk_unit + (g >> 4)) * 64 + lane) * 16 + (g & 15)] - 127;
  float* dst = out + (row - row0) * dim;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const int k = 64 * g + 16 * (i >> 3) + 8 * h + (i & 7);
    const uint32_t code = (v[i >> 3] >> (4 * (i & 7))) & 0xFu;
    if (k < dim) dst[k] = fp4_decode(code, e);
  }
}

int ts_launch_reconstruct_fp4(const TsLayout& L, const uint4* tiled, int64_t row0, int64_t n, float* out,
                              hipStream_t stream) {
  if (n <= 0) return TS_OK;
  const int ng = ts_fp4_code_groups(L), ns = ts_fp4_scale_units(L);
  unsigned blocks;
  TS_CHECK(ts_reconstruct_blocks(n, ng, blocks));
  hipLaunchKernelGGL(reconstruct_fp4_kernel, dim3(blocks), dim3(256), 0, stream, tiled, row0, n, L.dim, ng, ns, out);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// ------------------------------------------------------------------ update
// upd_rows_kernel (ts_update.hip) for a row block that is not a multiple of eight units: one wave per (entry, unit),
// scale units included.  Entry e holds the items first[e] .. first[e + 1) (fewer than 32), item = staging row * 32 +
// row of the block.
__global__ __launch_bounds__(256) void upd_rows_fp4_kernel(const uint4* stage, uint4* corpus, const int32_t* blk,
                                                           const int32_t* first, const int32_t* item, int64_t nwave,
                                                           int kg) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= nwave) return;
  const int64_t e = wv / kg;
  const int g = (int)(wv % kg);
  const int f0 = first[e], cnt = first[e + 1] - f0;
  const int mine = lane < cnt ? item[f0 + lane] : -1;
  int64_t j = -1;
  for (int t = 0; t < cnt; ++t) {
    const int it = __shfl(mine, t, 64);
    if ((it & 31) == (lane & 31)) j = it >> 5;
  }
  if (j < 0) return;
  corpus[((int64_t)blk[e] * kg + g) * 64 + lane] = stage[((j >> 5) * kg + g) * 64 + (lane & 32) + (j & 31)];
}

int ts_launch_update_rows_fp4(const TsLayout& L, const uint4* stage, uint4* corpus, const int32_t* blk,
                              const int32_t* first, const int32_t* item, int64_t n_entries, hipStream_t stream) {
  if (n_entries <= 0) return TS_OK;
  const int64_t nwave = n_entries * L.kg;
  const int64_t blocks = (nwave + 3) / 4;
  if (blocks > 0x7fffffffLL) { ts_set_error("update: too many rows in one chunk"); return TS_ERR_INVALID; }
  hipLaunchKernelGGL(upd_rows_fp4_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, stage, corpus, blk, first,
                     item, nwave, L.kg);
  TS_HIP(hipGetLastError());
  return TS_OK;
}
