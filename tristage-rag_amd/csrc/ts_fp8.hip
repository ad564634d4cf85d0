// The e4m3 token store's one stored format (include/tristage.h): a row x of H elements becomes the
// H bytes e4m3_rne(x * 2^k), k the largest integer with max|x_i| * 2^k <= 448 (so that max|x_i| * 2^k is in
// (224, 448]).  Stage 2 scores cosines, which no positive per-row factor changes, so k is not kept.  A zero row
// stores zeros (k = 0); a row holding a NaN or an Inf stores 0x7F (NaN) in every byte.
//
// One wave per row: absmax over the row, k from the exponent bits of the absmax, then a second pass over the row
// (from L2) that scales, rounds and writes 16 bytes per lane.  The rounding is integer arithmetic on the f32 bits
// (round to nearest even, e4m3 subnormals kept) so that it is bit for bit the torch CPU cast
// `(x * 2^k).to(torch.float8_e4m3fn)` the package's reference quantiser uses.
#include "ts_common.h"

namespace {
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kQThreads = 256;   // 4 rows per workgroup

// 16 elements of a row, as f32 (exact for every input type)
template <int XT>
__device__ __forceinline__ void q8_load16(const unsigned char* p, float (&v)[16]) {
  if constexpr (XT == TS_F32) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(p + 16 * j);
      v[4 * j + 0] = __uint_as_float(w.x); v[4 * j + 1] = __uint_as_float(w.y);
      v[4 * j + 2] = __uint_as_float(w.z); v[4 * j + 3] = __uint_as_float(w.w);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(p + 16 * j);
      const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t lo = ws[i] & 0xFFFFu, hi = ws[i] >> 16;
        if constexpr (XT == TS_BF16) {
          v[8 * j + 2 * i] = __uint_as_float(lo << 16);
          v[8 * j + 2 * i + 1] = __uint_as_float(hi << 16);
        } else {
          v[8 * j + 2 * i] = (float)__builtin_bit_cast(_Float16, (uint16_t)lo);
          v[8 * j + 2 * i + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)hi);
        }
      }
    }
  }
}

// e4m3fn bits of a finite f32 with |v| <= 448, round to nearest even
__device__ __forceinline__ uint32_t q8_encode(float v) {
  const uint32_t u = __float_as_uint(v);
  const uint32_t s = (u >> 24) & 0x80u, a = u & 0x7FFFFFFFu;
  uint32_t r;
  if (a >= 0x3C800000u) {   // |v| >= 2^-6: a normal e4m3 value; keep 3 mantissa bits, rebias 127 -> 7
    r = ((a + 0x7FFFFu + ((a >> 20) & 1u)) >> 20) - (120u << 3);
  } else {                  // subnormal range: multiples of 2^-9 (8 * 2^-9 = 2^-6 encodes as 0x08, the first normal)
    r = (uint32_t)__builtin_rintf(__uint_as_float(a) * 512.0f);
  }
  return s | r;
}

template <int XT>
__global__ __launch_bounds__(kQThreads) void quantize_rows_fp8_kernel(const unsigned char* x, int64_t rows, int H,
                                                                      unsigned char* out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kQThreads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;   // (uniform per wave)
  constexpr int esize = XT == TS_F32 ? 4 : 2;
  const unsigned char* xr = x + row * (int64_t)H * esize;
  unsigned char* orow = out + row * (int64_t)H;

  // |x| as f32 bits: for non-NaN values their unsigned order is the order of |x|, and every NaN / Inf is >= 0x7F800000
  uint32_t mx = 0;
  for (int c = 16 * lane; c < H; c += 16 * 64) {
    float v[16];
    q8_load16<XT>(xr + (size_t)c * esize, v);
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = max(mx, __float_as_uint(v[i]) & 0x7FFFFFFFu);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));

  if (mx >= 0x7F800000u) {   // NaN or Inf in the row: NaN everywhere, no finite garbage
    const u32x4 nan4 = {0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu};
    for (int c = 16 * lane; c < H; c += 16 * 64) *reinterpret_cast<u32x4*>(orow + c) = nan4;
    return;
  }
  // max|x| = 2^e * (1 + f / 2^23); 448 = 2^8 * 1.75, so k = 8 - e while the mantissa is <= 1.75 (f <= 0x600000),
  // else 7 - e.  A zero row keeps k = 0.
  int k = 0;
  if (mx != 0) {
    int e = (int)(mx >> 23);
    uint32_t f = mx & 0x7FFFFFu;
    if (e == 0) {   // f32 subnormal (a bf16 or f32 input): normalise the mantissa
      const int sh = __clz((int)f) - 8;
      f = (f << sh) & 0x7FFFFFu;
      e = 1 - sh;
    }
    k = (f <= 0x600000u ? 8 : 7) - (e - 127);
  }
  for (int c = 16 * lane; c < H; c += 16 * 64) {
    float v[16];
    q8_load16<XT>(xr + (size_t)c * esize, v);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i >> 2] |= q8_encode(__builtin_ldexpf(v[i], k)) << (8 * (i & 3));   // (exact)
    *reinterpret_cast<u32x4*>(orow + c) = u32x4{w[0], w[1], w[2], w[3]};
  }
}
}  // namespace

int ts_launch_quantize_rows_fp8(const void* x, int x_dtype, int64_t rows, int H, void* out, hipStream_t stream) {
  const int64_t blocks = (rows + kQThreads / 64 - 1) / (kQThreads / 64);
  if (blocks > 0x7FFFFFFF) return TS_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks), block(kQThreads);
  const unsigned char* xp = (const unsigned char*)x;
  unsigned char* op = (unsigned char*)out;
  if (x_dtype == TS_F32) hipLaunchKernelGGL(quantize_rows_fp8_kernel<TS_F32>, grid, block, 0, stream, xp, rows, H, op);
  else if (x_dtype == TS_F16) hipLaunchKernelGGL(quantize_rows_fp8_kernel<TS_F16>, grid, block, 0, stream, xp, rows, H, op);
  else hipLaunchKernelGGL(quantize_rows_fp8_kernel<TS_BF16>, grid, block, 0, stream, xp, rows, H, op);
  TS_HIP(hipGetLastError());
  return TS_OK;
}
