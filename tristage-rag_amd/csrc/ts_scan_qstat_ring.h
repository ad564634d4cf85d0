// The ring arithmetic of the query-stationary passes (ts_scan_qstat.hip), for the kernels, for the
// host that sizes their LDS, and for tests/qstat_ring.hip, which walks it without a GPU.  Integer arithmetic only.
//
// A workgroup walks `steps` row blocks of NWIN windows (8 KiB each).  Window W of the walk is k window W % NWIN of
// block W / NWIN and lives in slot W % depth.  The prologue requests windows 0 .. depth-1; step s requests windows
// depth + s*NWIN + kw, kw < NWIN, into the slots block s freed: (s*NWIN + kw) % depth.  depth is a constant of NWIN, so
// which block and k window request kw of a step belongs to, relative to the step, is known at compile time.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS_QSTAT_HD __host__ __device__
#else
#define TS_QSTAT_HD
#endif

#define TS_QSTAT_WINDOW 8192u          // bytes
#define TS_QSTAT_DEPTH 15              // windows: 120 KiB of ring, 4734 staging entries
#define TS_QSTAT_MAX_LEAD 8            // depth - 2 * NWIN, the walk's vmcnt

// windows of the ring: 15 for NWIN = 5 and 6
TS_QSTAT_HD constexpr int qstat_depth(int nwin) {
  const int hi = 2 * nwin + TS_QSTAT_MAX_LEAD;
  const int d = TS_QSTAT_DEPTH < hi ? TS_QSTAT_DEPTH : hi;
  return d > 2 * nwin ? d : 2 * nwin;
}

template <int NWIN>
struct QstatRing {
  static constexpr int DEPTH = qstat_depth(NWIN);
  // the counted wait of a step: with at most LEAD requests outstanding, block s + 1's pieces have landed
  static constexpr int LEAD = DEPTH - 2 * NWIN;
  static constexpr uint32_t RING_BYTES = (uint32_t)DEPTH * TS_QSTAT_WINDOW;
  static constexpr uint32_t BLOCK_BYTES = (uint32_t)NWIN * TS_QSTAT_WINDOW;   // of LDS and of the tiled corpus
  static_assert(NWIN >= 1 && LEAD >= 0 && LEAD <= TS_QSTAT_MAX_LEAD, "ring depth");

  // request kw of step s: block s + req_ahead(kw) of the walk, k window req_kwin(kw) of it
  TS_QSTAT_HD static constexpr int req_ahead(int kw) { return (DEPTH + kw) / NWIN; }
  TS_QSTAT_HD static constexpr int req_kwin(int kw) { return (DEPTH + kw) % NWIN; }
  static constexpr int AHEAD0 = DEPTH / NWIN;                    // the block of a step's first request
  static constexpr int AHEAD_MAX = (DEPTH + NWIN - 1) / NWIN;    // the block of its last one
  // requests of a step that go to block s + AHEAD0; the rest go to block s + AHEAD0 + 1
  static constexpr int SPLIT = AHEAD_MAX == AHEAD0 ? NWIN : NWIN - DEPTH % NWIN;

  // steps 0 .. main_steps-1 issue only requests inside the walk (step s is fully live iff s + AHEAD_MAX < steps)
  TS_QSTAT_HD static constexpr int main_steps(int steps) { return steps > AHEAD_MAX ? steps - AHEAD_MAX : 0; }

  // byte offset of a slot `add` bytes on (off < RING_BYTES, add <= RING_BYTES; unsigned wrap picks the smaller)
  TS_QSTAT_HD static constexpr uint32_t slot_add(uint32_t off, uint32_t add) {
    const uint32_t t = off + add, u = t - RING_BYTES;
    return t < u ? t : u;
  }
};

// The request state of one wave's walk, advanced by additions only.  P is a byte address: a pointer in the kernels, an
// offset into the corpus in the host test.
//   slot[kw]  LDS byte offset of window kw of the block the step computes; the step's request kw refills it
//   src0/src1 k window 0 of blocks s + AHEAD0 and s + AHEAD0 + 1 of the walk, the two row blocks a step's requests
//             belong to (request kw takes src0 iff kw < SPLIT); past the walk's end they are not dereferenced
template <int NWIN, class P>
struct QstatRingState {
  using R = QstatRing<NWIN>;
  uint32_t slot[NWIN];
  P src0, src1;
  int64_t step_bytes;

  // `first`: k window 0 of the walk's block 0
  TS_QSTAT_HD void start(P first, int64_t step_bytes_) {
    step_bytes = step_bytes_;
#pragma unroll
    for (int kw = 0; kw < NWIN; ++kw) slot[kw] = (uint32_t)kw * TS_QSTAT_WINDOW;
    src0 = first;
#pragma unroll
    for (int b = 0; b < R::AHEAD0; ++b) src0 = src0 + step_bytes;
    src1 = src0 + step_bytes;
  }
  // the prologue's request W < DEPTH: slot W, k window W % NWIN of block W / NWIN, inside the walk iff that block is
  TS_QSTAT_HD static constexpr bool prologue_live(int W, int steps) { return W / NWIN < steps; }
  TS_QSTAT_HD static P prologue_block(P first, int64_t step_bytes_, int W) {
    P b = first;
#pragma unroll
    for (int i = 0; i < W / NWIN; ++i) b = b + step_bytes_;
    return b;
  }
  // request kw of step s
  TS_QSTAT_HD static constexpr bool req_live(int kw, int s, int steps) { return s + R::req_ahead(kw) < steps; }
  TS_QSTAT_HD P req_block(int kw) const { return R::req_ahead(kw) == R::AHEAD0 ? src0 : src1; }
  // to the next step
  TS_QSTAT_HD void advance() {
    src0 = src0 + step_bytes;
    src1 = src1 + step_bytes;
#pragma unroll
    for (int kw = 0; kw < NWIN; ++kw) slot[kw] = R::slot_add(slot[kw], R::BLOCK_BYTES);
  }
};

// bytes between two consecutive row blocks of a workgroup's walk in the tiled corpus
TS_QSTAT_HD constexpr int64_t qstat_step_bytes(int64_t grid, int64_t blk_stride, int64_t blk_bytes) {
  return grid * blk_stride * blk_bytes;
}
// byte offset of the first row block of workgroup `bid`
TS_QSTAT_HD constexpr int64_t qstat_first_byte(int64_t blk0, int64_t bid, int64_t blk_stride, int64_t blk_bytes) {
  return (blk0 + bid * blk_stride) * blk_bytes;
}
