// Removal of rows (ts_index_remove / ts_index_compact): the tombstone bitmap of a flat index and
// the on-device compaction of its tiled corpus.
//
// The bitmap has the layout of the filtered-search masks: bit r % 32 of word r / 32 set = row r live, so word b
// is row block b (TS_ROWS_PER_BLOCK = 32 rows), and a search of an index with removed rows is a filtered search
// whose masks are ANDed with it (ts_launch_and_live).  Bits at or beyond ntotal are kept clear.  Every device
// write below is a plain vector store or a vector atomic.
#include "ts_common.h"

// ---------------------------------------------------------------- bitmap
// sets the bits of rows [row0, row1); one thread per word, so no two threads touch the same word
__global__ void live_set_kernel(uint32_t* live, int64_t row0, int64_t row1) {
  const int64_t w = row0 / 32 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t lo = std::max<int64_t>(row0, w * 32), hi = std::min<int64_t>(row1, w * 32 + 32);
  if (lo >= hi) return;
  const int n = (int)(hi - lo), s = (int)(lo - w * 32);
  const uint32_t bits = (n >= 32 ? ~0u : ((1u << n) - 1u)) << s;
  live[w] = (s == 0 && n == 32) ? bits : (live[w] | bits);
}

int ts_launch_live_set(uint32_t* live, int64_t row0, int64_t row1, hipStream_t stream) {
  if (row1 <= row0) return TS_OK;
  const int64_t nw = (row1 + 31) / 32 - row0 / 32;
  hipLaunchKernelGGL(live_set_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, stream, live, row0, row1);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// clears the bits of the listed ids (after the id offset); an id outside [0, ntotal) or already clear is not
// counted, and of two equal ids in one call only the one whose atomic clears the bit is
__global__ void live_clear_kernel(uint32_t* live, const int64_t* ids, int64_t n, int64_t id_offset, int64_t ntotal,
                                  unsigned long long* cleared) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t hit = 0;
  if (i < n) {
    const int64_t r = ids[i] - id_offset;
    if (r >= 0 && r < ntotal) {
      const uint32_t bit = 1u << (r & 31);
      hit = (atomicAnd(&live[r >> 5], ~bit) & bit) ? 1u : 0u;
    }
  }
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit != 0);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(cleared, (unsigned long long)__builtin_popcountll(bal));
}

int ts_launch_live_clear(uint32_t* live, const int64_t* ids, int64_t n, int64_t id_offset, int64_t ntotal,
                         unsigned long long* cleared, hipStream_t stream) {
  if (n <= 0) return TS_OK;
  hipLaunchKernelGGL(live_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, live, ids, n,
                     id_offset, ntotal, cleared);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// out[m][w] = bits[m][w] & live[w] for m < n_masks, out[n_masks][w] = live[w]: the masks a filtered pass of an index
// with removed rows reads (a query without a mask gets the last one)
__global__ void and_live_kernel(const uint32_t* bits, int64_t bit_words, int n_masks, const uint32_t* live,
                                int64_t words, uint32_t* out) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int m = blockIdx.y;
  if (w >= words) return;
  const uint32_t lw = live[w];
  out[(int64_t)m * words + w] = m < n_masks ? (bits[(int64_t)m * bit_words + w] & lw) : lw;
}

int ts_launch_and_live(const uint32_t* bits, int64_t bit_words, int n_masks, const uint32_t* live, int64_t words,
                       uint32_t* out, hipStream_t stream) {
  if (words <= 0) return TS_OK;
  hipLaunchKernelGGL(and_live_kernel, dim3((unsigned)((words + 255) / 256), (unsigned)(n_masks + 1)), dim3(256), 0,
                     stream, bits, bit_words, n_masks, live, words, out);
  TS_HIP(hipGetLastError());
  return TS_OK;
}

// ---------------------------------------------------------------- compaction
// Prefix count over the live words (three launches, no library scan): cnt[w] = live rows of word w and per tile of
// kTile words its sum, then an exclusive scan of the tile sums in one workgroup, then per tile the exclusive scan of
// its words plus the tile's prefix -> pre[w], the new position of word w's first live row.  first[0] = the lowest
// removed row (rows below it keep their slots).
constexpr int kTile = 256;

// exclusive prefix of v over the workgroup (blockDim.x a multiple of 64, at most 1024); *total = the sum
__device__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) lds[wid] = x;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (int i = 0; i < nw; ++i) {
    if (i < wid) base += lds[i];
    tot += lds[i];
  }
  *total = tot;
  return base + x - v;
}

__global__ __launch_bounds__(kTile) void word_count_kernel(const uint32_t* live, int64_t words, int64_t ntotal,
                                                           uint32_t* cnt, uint32_t* tile_sum,
                                                           unsigned long long* first) {
  __shared__ uint32_t lds[kTile / 64];
  const int64_t w = (int64_t)blockIdx.x * kTile + threadIdx.x;
  uint32_t c = 0;
  if (w < words) {
    const int64_t rows = ntotal - w * 32;
    const uint32_t valid = rows >= 32 ? ~0u : ((1u << rows) - 1u);
    const uint32_t lw = live[w] & valid;
    c = (uint32_t)__builtin_popcount(lw);
    cnt[w] = c;
    const uint32_t holes = ~lw & valid;
    if (holes) atomicMin(first, (unsigned long long)(w * 32 + __builtin_ctz(holes)));
  }
  uint32_t tot = 0;
  (void)block_exclusive_scan(c, lds, &tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// one workgroup of 1024 threads: tile_sum[] -> its exclusive prefix, in place
__global__ __launch_bounds__(1024) void tile_scan_kernel(uint32_t* tile_sum, int64_t tiles) {
  __shared__ uint32_t lds[16];
  const int64_t per = (tiles + 1023) / 1024;
  const int64_t t0 = std::min<int64_t>(tiles, threadIdx.x * per), t1 = std::min<int64_t>(tiles, t0 + per);
  uint32_t sum = 0;
  for (int64_t t = t0; t < t1; ++t) sum += tile_sum[t];
  uint32_t tot = 0;
  uint32_t run = block_exclusive_scan(sum, lds, &tot);
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t v = tile_sum[t];
    tile_sum[t] = run;
    run += v;
  }
}

__global__ __launch_bounds__(kTile) void word_scan_kernel(const uint32_t* cnt, const uint32_t* tile_pre, int64_t words,
                                                          uint32_t* pre) {
  __shared__ uint32_t lds[kTile / 64];
  const int64_t w = (int64_t)blockIdx.x * kTile + threadIdx.x;
  const uint32_t c = w < words ? cnt[w] : 0u;
  uint32_t tot = 0;
  const uint32_t x = block_exclusive_scan(c, lds, &tot);
  if (w < words) pre[w] = tile_pre[blockIdx.x] + x;
}

__global__ void compact_map_kernel(const uint32_t* live, const uint32_t* pre, int64_t ntotal, int32_t* new2old,
                                   int64_t* old2new) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= ntotal) return;
  const uint32_t lw = live[r >> 5];
  const uint32_t bit = 1u << (r & 31);
  int64_t j = -1;
  if (lw & bit) {
    j = (int64_t)pre[r >> 5] + __builtin_popcount(lw & (bit - 1u));
    new2old[j] = (int32_t)r;
  }
  if (old2new) old2new[r] = j;
}

// Staging image of the new row blocks [b0, b0 + nb): unit u of the tiled layout (ts_common.h) takes the same unit of
// the row's old slot, or zero for the padding rows at or beyond nlive.  Written in the tiled order, so that the
// image goes back into the corpus as one contiguous copy.
__global__ void compact_gather_kernel(const uint4* corpus, int kg, const int32_t* new2old, int64_t nlive, int64_t b0,
                                      int64_t nunits, uint4* stage) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= nunits) return;
  const int l = (int)(u & 63);
  const int64_t bg = u >> 6;             // (b - b0) * kg + g
  const int64_t b = b0 + bg / kg;
  const int64_t g = bg % kg;
  const int64_t j = b * 32 + (l & 31);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (j < nlive) {
    const int64_t r = new2old[j];
    v = corpus[(((r >> 5) * kg + g) << 6) + (l & 32) + (r & 31)];
  }
  stage[u] = v;
}

static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t ts_compact_scratch_bytes(int64_t ntotal) {
  const int64_t words = (ntotal + 31) / 32, tiles = (words + kTile - 1) / kTile;
  return 2 * al256((size_t)words * 4) + al256((size_t)tiles * 4) + 256 + al256((size_t)ntotal * 4);
}

int ts_compact_corpus(const TsLayout& L, uint4* corpus, const uint32_t* live, int64_t ntotal, void* scratch,
                      size_t scratch_bytes, uint4* stage, size_t stage_bytes, int64_t* old2new_dev, int64_t* nlive_out,
                      hipStream_t stream) {
  const int64_t words = (ntotal + 31) / 32, tiles = (words + kTile - 1) / kTile;
  // scratch: cnt[words], pre[words], tile sums, first (8 B), new2old[ntotal]
  if (scratch_bytes < ts_compact_scratch_bytes(ntotal)) return TS_ERR_INVALID;   // (the caller sizes it)
  char* sc = (char*)scratch;
  uint32_t* cnt = (uint32_t*)sc;
  uint32_t* pre = (uint32_t*)(sc + al256((size_t)words * 4));
  uint32_t* tile = (uint32_t*)(sc + 2 * al256((size_t)words * 4));
  unsigned long long* first = (unsigned long long*)(sc + 2 * al256((size_t)words * 4) + al256((size_t)tiles * 4));
  int32_t* new2old = (int32_t*)((char*)first + 256);
  TS_HIP(hipMemsetAsync(first, 0xFF, 8, stream));
  hipLaunchKernelGGL(word_count_kernel, dim3((unsigned)tiles), dim3(kTile), 0, stream, live, words, ntotal, cnt, tile,
                     first);
  TS_HIP(hipGetLastError());
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, stream, tile, tiles);
  TS_HIP(hipGetLastError());
  hipLaunchKernelGGL(word_scan_kernel, dim3((unsigned)tiles), dim3(kTile), 0, stream, cnt, tile, words, pre);
  TS_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_map_kernel, dim3((unsigned)((ntotal + 255) / 256)), dim3(256), 0, stream, live, pre,
                     ntotal, new2old, old2new_dev);
  TS_HIP(hipGetLastError());
  uint32_t last[2] = {0, 0};
  unsigned long long first_h = 0;
  TS_HIP(hipMemcpyAsync(&last[0], pre + words - 1, 4, hipMemcpyDeviceToHost, stream));
  TS_HIP(hipMemcpyAsync(&last[1], cnt + words - 1, 4, hipMemcpyDeviceToHost, stream));
  TS_HIP(hipMemcpyAsync(&first_h, first, 8, hipMemcpyDeviceToHost, stream));
  TS_HIP(hipStreamSynchronize(stream));
  const int64_t nlive = (int64_t)last[0] + last[1];
  *nlive_out = nlive;
  const int64_t first_hole = first_h == ~0ull ? ntotal : (int64_t)first_h;
  // Ascending chunks of whole row blocks through `stage`: chunk c gathers the new blocks [b, b + cb) from their old
  // slots, then overwrites them.  A new row position is never above its old one, so no later chunk reads a block
  // that an earlier one has written; within a chunk the staging copy separates the reads from the writes.
  const size_t bb = ts_block_bytes(L);
  const int64_t cb = std::max<int64_t>(1, (int64_t)(stage_bytes / bb));
  const int64_t new_blocks = (nlive + 31) / 32, old_blocks = (ntotal + 31) / 32;
  for (int64_t b = first_hole / 32; b < new_blocks; b += cb) {
    const int64_t nb = std::min(cb, new_blocks - b);
    const int64_t nunits = nb * L.kg * 64;
    hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)((nunits + 255) / 256)), dim3(256), 0, stream, corpus,
                       L.kg, new2old, nlive, b, nunits, stage);
    TS_HIP(hipGetLastError());
    TS_HIP(hipMemcpyAsync((char*)corpus + (size_t)b * bb, stage, (size_t)nb * bb, hipMemcpyDeviceToDevice, stream));
  }
  // the blocks the survivors no longer reach go back to the zeros of never-written storage (grow_corpus)
  if (old_blocks > new_blocks)
    TS_HIP(hipMemsetAsync((char*)corpus + (size_t)new_blocks * bb, 0, (size_t)(old_blocks - new_blocks) * bb, stream));
  return TS_OK;
}
