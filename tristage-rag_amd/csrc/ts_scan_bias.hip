// Boosted search (ts_index_search_biased): every row's score plus a per-row f32 prior, ranked inside
// the stage-1 scan.  boosted(q, r) = score(q, r) + bias[r], one f32 addition of the score every other search produces.
//
//   scan_kernel<QH, SCAN_FILTER, Op16<DT>, WalkLiveBias>   the masked ring scan whose walk also carries the 32 biases
//                                                          of its row block and whose epilogue tests score + bias
//   tau_biased_kernel                                      tau_masked_kernel (ts_select.hip) on sample score + bias
//   bias_ids_kernel                                        the dense path: adds the bias to a chunk of dense scores
//                                                          and writes the ids of mask_ids_kernel
//
// The bias reaches the registers through vector loads, not scalar ones: a lane holds rows acc_row(r, lane), r < 16,
// of its block, which are four runs of four rows, so four 16-byte loads at bias + 32 blk + 8 r4 + 4 (lane >> 5) give
// it exactly its 16 values (every lane of a half wave reads the same 16 bytes: one request).  They are issued for the
// NEXT block beside the allow words, just before the tail refills the ring from that block, unpredicated; vmcnt
// retires in order, so the first ring wait of the next block covers them and no wait is added anywhere.  Scalar loads
// would share lgkmcnt with the LDS reads of the query image: with one outstanding, every LDS wait of the block's
// first steps becomes lgkmcnt(0), and the bias (4 bytes per row, 40 MB at 10 M rows) comes from HBM, not from a
// cache as the live-block list does.
//
// The caller's array has ntotal entries and ntotal need not be a multiple of 32: the last, partial row block reads
// bias_tail, a 32-float copy of its entries padded with zeros (ts_index.hip), chosen by a wave-uniform select of the
// address.  Every device write below is a plain vector store or a vector atomic.
#include "ts_scan_dev.h"

namespace {

struct WalkLiveBias : WalkLive {
  typedef BiasScanParams Params;
  static constexpr bool kBiased = true;

  static __device__ __forceinline__ const f32x4* bias_of(const Params& p, int64_t blk, int lane) {
    const float* bp = (blk == p.tail_blk) ? p.bias_tail : p.bias + blk * TS_ROWS_PER_BLOCK;
    return reinterpret_cast<const f32x4*>(bp + 4 * (lane >> 5));
  }
  static __device__ __forceinline__ float bias_max(const f32x4 (&b)[4]) {
    const float m0 = fmaxf(fmaxf(b[0][0], b[0][1]), fmaxf(b[0][2], b[0][3]));
    const float m1 = fmaxf(fmaxf(b[1][0], b[1][1]), fmaxf(b[1][2], b[1][3]));
    const float m2 = fmaxf(fmaxf(b[2][0], b[2][1]), fmaxf(b[2][2], b[2][3]));
    const float m3 = fmaxf(fmaxf(b[3][0], b[3][1]), fmaxf(b[3][2], b[3][3]));
    return fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
  }
  // rows 8 r4 + 4 (lane >> 5) + 0..3 of the block are accumulator registers 4 r4 + 0..3 (acc_row)
  static __device__ __forceinline__ void bias_fetch(const Params& p, int64_t blk, int lane, f32x4 (&b)[4]) {
    const f32x4* src = bias_of(p, blk, lane);
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) b[r4] = src[2 * r4];
  }
  static __device__ __forceinline__ void bias_init(const Params& p, int64_t blk, int lane, f32x4 (&bcur)[4], float& bmax) {
    bias_fetch(p, blk, lane, bcur);
    bmax = bias_max(bcur);
  }
  static __device__ __forceinline__ void bias_advance(const f32x4 (&bnxt)[4], f32x4 (&bcur)[4], float& bmax) {
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) bcur[r4] = bnxt[r4];
    bmax = bias_max(bcur);
  }

  // epilogue_filter<QH, SL, true> on boosted scores.  The common path stays one ballot: the f32 addition is monotone
  // in both arguments, so fl(max score + max bias) is at least every fl(score + bias) of the lane and the test never
  // loses a survivor (fmaxf drops a NaN bias; a NaN boosted score fails the >= of the rare path, so such a row is
  // never staged).  Only the rare path forms the 16 boosted scores; it stages those, not the raw ones.
  template <int QH, class SL>
  static __device__ __forceinline__ void epilogue(const Params& p, SL* st, const f32x16 (&acc)[QH], const float (&tau)[QH],
                                                  int64_t blk, int lane, const uint32_t (&mw)[QH], const f32x4 (&bcur)[4],
                                                  float bmax) {
    bool hit = false;
#pragma unroll
    for (int hq = 0; hq < QH; ++hq) hit |= (acc_max(acc[hq]) + bmax >= tau[hq]);
    if (__builtin_amdgcn_ballot_w64(hit) == 0ull) return;  // the common case
    const int64_t row_base = blk * TS_ROWS_PER_BLOCK;
#pragma unroll
    for (int hq = 0; hq < QH; ++hq) {
      const int q = hq * 32 + (lane & 31);
      float bs[16];
      uint32_t mask = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        bs[r] = acc[hq][r] + bcur[r >> 2][r & 3];
        const bool ok = (bs[r] >= tau[hq]) && (row_base + acc_row(r, lane) < p.ntotal) &&
                        ((mw[hq] >> acc_row(r, lane)) & 1u);
        mask |= ok ? (1u << r) : 0u;
      }
      if (mask) {
        uint32_t slot = atomicAdd(&st->cnt, (uint32_t)__builtin_popcount(mask));  // LDS
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (mask & (1u << r)) {
            const int32_t id = (int32_t)(row_base + acc_row(r, lane));
            if (slot < SL::kCap) {
              st->score[slot] = bs[r];
              st->id[slot] = id;
              st->q[slot] = (uint8_t)q;
            } else {
              // staging area full (heavily clustered hits): append directly
              const uint32_t g = atomicAdd(&p.cand_cnt[q], 1u);
              if (g < p.cand_cap) {
                p.cand_score[(size_t)q * p.cand_cap + g] = bs[r];
                p.cand_id[(size_t)q * p.cand_cap + g] = id;
              }
            }
            ++slot;
          }
        }
      }
    }
  }
};

#define BIAS_SEL_THREADS 1024
#define BIAS_NEG_MAX (-3.402823466e38f)

// the order-preserving keys of the select kernels (ts_select.hip)
__device__ __forceinline__ uint32_t bias_f2key(float f) {
  if (f != f) return 0u;  // NaN ranks last
  f = f + 0.0f;           // -0 -> +0 so equal scores have equal keys
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bias_key2f(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __builtin_bit_cast(float, u);
}

}  // namespace

// Thresholds of a boosted pass: tau_masked_kernel (ts_select.hip) with sample entry i keyed by s[i] + bias[row], the
// same f32 addition the scan and the dense path make.  S_q, N_q, m_q and need[q] are as there; the sample itself is
// the unbiased strided dense sample, read once.  A copy, with the key helpers it needs, and not a body shared through a
// header: built from a shared __device__ template, tau_masked_kernel no longer disassembles to the instructions it
// has (tools/kernel_disasm_diff.sh), and the kernels of the existing searches are to stay as they are.  A fix to one
// of the two belongs in both.
__global__ __launch_bounds__(BIAS_SEL_THREADS) void tau_biased_kernel(const float* sample, int64_t S, int64_t sstride,
                                                                      int64_t ntotal, const uint32_t* bits,
                                                                      int64_t words, const float* bias, TsMaskDev* md,
                                                                      int nq, int k, uint32_t over, uint32_t min_rank,
                                                                      float* tau, uint32_t* report) {
  constexpr int KEEP = 4;
  __shared__ __attribute__((aligned(16))) uint32_t keys[KEEP * BIAS_SEL_THREADS];
  __shared__ uint32_t cnt;
  const int q = blockIdx.x;
  const int tid = threadIdx.x;
  if (q == 0 && tid == 0 && report) report[0] = md->nlive;
  if (q >= nq) {
    if (tid == 0) { tau[q] = 3.402823466e38f; md->need[q] = 0u; }
    return;
  }
  const int32_t qm = md->qmask[q];
  const uint32_t* mrow = qm >= 0 ? bits + (int64_t)qm * words : nullptr;
  const float* s = sample + (int64_t)q * S;
  if (tid == 0) cnt = 0;
  __syncthreads();
  uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, mine = 0;
  for (int64_t i = tid; i < S; i += BIAS_SEL_THREADS) {
    const int64_t row = (i >> 5) * sstride * TS_ROWS_PER_BLOCK + (i & 31);
    if (row >= ntotal) continue;
    if (mrow && !((mrow[row >> 5] >> (row & 31)) & 1u)) continue;
    ++mine;
    const uint32_t kk = bias_f2key(s[i] + bias[row]);
    if (kk > a3) {
      if (kk > a0) { a3 = a2; a2 = a1; a1 = a0; a0 = kk; }
      else if (kk > a1) { a3 = a2; a2 = a1; a1 = kk; }
      else if (kk > a2) { a3 = a2; a2 = kk; }
      else a3 = kk;
    }
  }
  if (mine) atomicAdd(&cnt, mine);
  keys[tid] = a0;
  keys[BIAS_SEL_THREADS + tid] = a1;
  keys[2 * BIAS_SEL_THREADS + tid] = a2;
  keys[3 * BIAS_SEL_THREADS + tid] = a3;
  __syncthreads();
  constexpr uint32_t P = KEEP * BIAS_SEL_THREADS;
  for (uint32_t size = 2; size <= P; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t t = tid; t < (P >> 1); t += BIAS_SEL_THREADS) {
        const uint32_t i = 2 * t - (t & (stride - 1));
        const uint32_t j = i + stride;
        const bool desc = (i & size) == 0;
        const uint32_t a = keys[i], b = keys[j];
        if (desc ? (b > a) : (a > b)) { keys[i] = b; keys[j] = a; }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    const uint64_t Nq = qm >= 0 ? (uint64_t)md->popc[md->qd[q]] : (uint64_t)ntotal;
    const uint64_t Sq = cnt;
    uint64_t m = Nq ? ((uint64_t)over * (uint64_t)k * Sq + Nq - 1) / Nq : 0;
    if (m < min_rank) m = min_rank;
    float t = BIAS_NEG_MAX;
    if (Sq >= m) {
      uint32_t idx = (uint32_t)(m - 1);
      if (idx >= P) idx = P - 1;
      const uint32_t kx = keys[idx];
      t = (kx == 0u) ? BIAS_NEG_MAX : bias_key2f(kx);
    }
    tau[q] = t;
    md->need[q] = (uint32_t)((uint64_t)k < Nq ? (uint64_t)k : Nq);
  }
}

int ts_launch_tau_biased(const float* sample, int64_t S, int64_t sstride, int64_t ntotal, const uint32_t* bits,
                         int64_t words, const float* bias, TsMaskDev* md, int nq, int k, uint32_t over,
                         uint32_t min_rank, float* tau, uint32_t* report, hipStream_t stream) {
  hipLaunchKernelGGL(tau_biased_kernel, dim3(TS_MAX_Q), dim3(BIAS_SEL_THREADS), 0, stream, sample, S, sstride, ntotal,
                     bits, words, bias, md, nq, k, over, min_rank, tau, report);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// The dense path of a boosted search, one chunk: dense[q][i] += bias[row0 + i] and ids[q][i] = row0 + i where the row
// is allowed for query q (mask_ids_kernel) and its boosted score is a number, else -1; SEL_PAIRS32 over the two then
// ranks exactly the eligible rows.  Rows at or beyond ntotal are outside `rows`.
__global__ void bias_ids_kernel(const uint32_t* bits, int64_t words, TsMaskPass mp, const float* bias, int64_t row0,
                                uint32_t rows, int64_t ld, float* dense, int32_t* ids) {
  const int q = blockIdx.y;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const int32_t qm = mp.qmask[q];
  const int64_t row = row0 + i;
  const float b = dense[(int64_t)q * ld + i] + bias[row];
  const bool ok = (qm < 0 || ((bits[(int64_t)qm * words + (row >> 5)] >> (row & 31)) & 1u)) && b == b;
  dense[(int64_t)q * ld + i] = b;
  ids[(int64_t)q * ld + i] = ok ? (int32_t)row : -1;
}

int ts_launch_bias_ids(const uint32_t* bits, int64_t words, const TsMaskPass& mp, const float* bias, int nq,
                       int64_t row0, uint32_t rows, int64_t ld, float* dense, int32_t* ids, hipStream_t stream) {
  if (nq <= 0 || rows == 0) return TS_OK;
  hipLaunchKernelGGL(bias_ids_kernel, dim3((rows + 255) / 256, nq), dim3(256), 0, stream, bits, words, mp, bias, row0,
                     rows, ld, dense, ids);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

int ts_launch_scan_biased(const TsLayout& L, int qh, const BiasScanParams& p, int num_cus, hipStream_t stream) {
  if (p.nwork <= 0) return TS_OK;
  if (L.dtype != TS_F16 && L.dtype != TS_BF16) {
    ts_set_error("the biased scan takes f16 / bf16 storage only");
    return TS_ERR_UNSUPPORTED;
  }
  if ((qh != 1 && qh != 2) || !p.bias || !p.bias_tail) {
    ts_set_error("biased scan: %d query halves, bias %p, tail %p", qh, (const void*)p.bias, (const void*)p.bias_tail);
    return TS_ERR_INVALID;
  }
  if (ts_scan_lds_bytes(L, qh) > TS_LDS_BYTES) {
    ts_set_error("dimension %d too large for the LDS-resident query image", L.dim);
    return TS_ERR_UNSUPPORTED;
  }
  return L.dtype == TS_F16 ? launch_scan<Op16<TS_F16>, WalkLiveBias>(SCAN_FILTER, qh, L.kg, p, num_cus, stream)
                           : launch_scan<Op16<TS_BF16>, WalkLiveBias>(SCAN_FILTER, qh, L.kg, p, num_cus, stream);
}
