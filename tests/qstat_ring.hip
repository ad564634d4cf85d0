// Walks the ring of the query-stationary passes (ts_scan_qstat_ring.h: the arithmetic scan_qstat_kernel and
// scan_qstat_sample_kernel use) as a wave does, prologue, main loop and tail, against a model of the LDS slots and of
// the in-order request queue.  Built and run by tests/test_qstat_ring_host.py.  Host arithmetic only: no HIP call, no
// device needed.  Prints one line per (NWIN, grid shape) and "ok"; the first violated property ends it with status 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ts_scan_qstat_ring.h"

#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);    \
      printf(__VA_ARGS__);                                       \
      printf("\n");                                              \
      exit(1);                                                   \
    }                                                            \
  } while (0)

static const int64_t DEAD = -1;   // the address a request past the walk reads

struct Request {
  int64_t src;      // byte offset in the corpus, or DEAD
  uint32_t dst;     // LDS byte offset of the slot
  int64_t window;   // the window of the walk it carries, or -1
};

// one workgroup's walk: `steps` row blocks blk0 + (bid + s * grid) * stride of a corpus of `corpus_bytes`
template <int NWIN>
static long walk(int steps, int64_t bid, int64_t grid, int64_t blk0, int64_t stride, int64_t corpus_bytes) {
  using R = QstatRing<NWIN>;
  using State = QstatRingState<NWIN, int64_t>;
  const int64_t blk_bytes = R::BLOCK_BYTES;
  auto want_src = [&](int64_t W) {   // the model's own address of window W: not the incremental one
    return (blk0 + (bid + (W / NWIN) * grid) * stride) * blk_bytes + (W % NWIN) * (int64_t)TS_QSTAT_WINDOW;
  };
  std::vector<Request> issued;
  int64_t slot_window[R::DEPTH];       // what each slot was last requested for (-1: dead bytes)
  for (int i = 0; i < R::DEPTH; ++i) slot_window[i] = -2;   // never requested
  std::vector<int> times_requested((size_t)steps * NWIN, 0);
  int64_t landed = 0;                  // requests 0 .. landed-1 have been waited for

  // `barrier_step`: the steps whose reads are behind a barrier are 0 .. barrier_step-1
  auto request = [&](uint32_t dst, int64_t src, int64_t W, int barrier_step) {
    CHECK(dst % TS_QSTAT_WINDOW == 0 && dst < R::RING_BYTES, "dst %u", dst);
    const int sl = (int)(dst / TS_QSTAT_WINDOW);
    CHECK(sl == (int)(W % R::DEPTH), "window %lld into slot %d", (long long)W, sl);
    // no slot is requested again before the barrier that follows its last read
    if (slot_window[sl] >= 0 && slot_window[sl] / NWIN < steps)
      CHECK(slot_window[sl] / NWIN < barrier_step, "slot %d of block %lld restaged at barrier %d", sl,
            (long long)(slot_window[sl] / NWIN), barrier_step);
    if (W / NWIN < steps) {
      CHECK(src == want_src(W), "window %lld from %lld, want %lld", (long long)W, (long long)src, (long long)want_src(W));
      CHECK(src >= 0 && src + (int64_t)TS_QSTAT_WINDOW <= corpus_bytes, "window %lld outside the corpus", (long long)W);
      times_requested[(size_t)W] += 1;
      slot_window[sl] = W;
    } else {
      CHECK(src == DEAD, "window %lld past the walk reads %lld", (long long)W, (long long)src);
      slot_window[sl] = -1;
    }
    issued.push_back({src, dst, W / NWIN < steps ? W : -1});
  };

  const int64_t first = qstat_first_byte(blk0, bid, stride, blk_bytes);
  const int64_t step_bytes = qstat_step_bytes(grid, stride, blk_bytes);
  // ---- prologue: windows 0 .. DEPTH-1, then vmcnt(0) and a barrier
  for (int W = 0; W < R::DEPTH; ++W) {
    const bool live = State::prologue_live(W, steps);
    request((uint32_t)W * TS_QSTAT_WINDOW,
            live ? State::prologue_block(first, step_bytes, W) + (W % NWIN) * (int64_t)TS_QSTAT_WINDOW : DEAD, W, 0);
  }
  State st;
  st.start(first, step_bytes);
  landed = (int64_t)issued.size();

  const int nmain = R::main_steps(steps);
  CHECK(nmain >= 0 && nmain <= steps && steps - nmain <= R::AHEAD_MAX, "split %d of %d", nmain, steps);
  for (int s = 0; s < steps; ++s) {
    // the block's reads: its windows are in its slots and were waited for one barrier ago
    for (int kw = 0; kw < NWIN; ++kw) {
      const int64_t W = (int64_t)s * NWIN + kw;
      CHECK(st.slot[kw] == (uint32_t)(W % R::DEPTH) * TS_QSTAT_WINDOW, "step %d window %d reads %u", s, kw, st.slot[kw]);
      CHECK(slot_window[W % R::DEPTH] == W, "step %d: slot holds window %lld", s, (long long)slot_window[W % R::DEPTH]);
      CHECK(W < landed && issued[(size_t)W].window == W, "step %d reads window %lld before it landed", s, (long long)W);
    }
    // the counted wait: at most LEAD outstanding.  Requests retire in order and request n carries window n.
    CHECK((int64_t)issued.size() == R::DEPTH + (int64_t)s * NWIN, "step %d: %zu issued", s, issued.size());
    landed = (int64_t)issued.size() - R::LEAD;
    if (s + 1 < steps) CHECK(((int64_t)s + 2) * NWIN <= landed, "step %d: block %d not landed at its wait", s, s + 1);
    // the barrier; then the step's NWIN requests into the slots block s freed
    const size_t before = issued.size();
    bool all_live = true;
    for (int kw = 0; kw < NWIN; ++kw) all_live = all_live && State::req_live(kw, s, steps);
    CHECK(all_live == (s < nmain), "step %d of %d: main loop %d", s, steps, nmain);
    for (int kw = 0; kw < NWIN; ++kw) {
      CHECK((R::req_ahead(kw) == R::AHEAD0) == (kw < R::SPLIT), "request %d", kw);   // (the main loop's one statement)
      const bool live = s < nmain || State::req_live(kw, s, steps);   // the main loop does not ask
      const int64_t W = R::DEPTH + (int64_t)s * NWIN + kw;
      request(st.slot[kw], live ? st.req_block(kw) + R::req_kwin(kw) * (int64_t)TS_QSTAT_WINDOW : DEAD, W, s + 1);
    }
    CHECK(issued.size() - before == (size_t)NWIN, "step %d issued %zu requests", s, issued.size() - before);
    st.advance();
  }
  for (size_t W = 0; W < times_requested.size(); ++W)
    CHECK(times_requested[W] == 1, "window %zu requested %d times", W, times_requested[W]);
  return (long)issued.size();
}

template <int NWIN>
static void all_walks() {
  using R = QstatRing<NWIN>;
  static_assert(R::DEPTH == 15, "the ring of both widths");
  static_assert(R::LEAD == 15 - 2 * NWIN, "the counted wait");
  // step s is fully live iff (depth + s * NWIN + NWIN - 1) / NWIN < steps: s + 3 < steps at both widths
  for (int steps = 1; steps <= 64; ++steps) {
    int n = 0;
    for (int s = 0; s < steps; ++s) n += (R::DEPTH + s * NWIN + NWIN - 1) / NWIN < steps;
    CHECK(n == R::main_steps(steps) && n == (steps > 3 ? steps - 3 : 0), "main steps of %d: %d", steps, n);
  }
  for (uint32_t off = 0; off < R::RING_BYTES; off += TS_QSTAT_WINDOW)
    for (uint32_t add = 0; add <= R::RING_BYTES; add += TS_QSTAT_WINDOW)
      CHECK(R::slot_add(off, add) == (off + add) % R::RING_BYTES, "slot_add(%u, %u)", off, add);
  // every steps in 1..64 with one workgroup; then grids whose workgroups differ by one step (nwork = grid * s + r):
  // workgroup bid walks ceil((nwork - bid) / grid) blocks.  Plain walks, strided samples, a walk that starts inside.
  const int64_t shapes[][3] = {{1, 0, 1}, {2, 0, 1}, {5, 0, 1}, {256, 0, 1}, {3, 7, 1}, {4, 0, 5}, {256, 3, 129}};
  for (const auto& sh : shapes) {
    const int64_t grid = sh[0], blk0 = sh[1], stride = sh[2];
    long walks = 0, requests = 0;
    for (int s = 1; s <= 64; ++s) {
      const int64_t rs[] = {0, 1, grid / 2, grid - 1};
      for (int64_t r : rs) {
        if (r >= grid) continue;
        const int64_t nwork = grid * (s - 1) + (r == 0 ? grid : r);   // workgroups < r (or all) walk s steps, the rest s - 1
        if (nwork < grid) continue;   // (the launchers keep grid <= nwork)
        const int64_t corpus_bytes = (blk0 + (nwork - 1) * stride + 1) * (int64_t)R::BLOCK_BYTES;
        const int64_t bids[] = {0, r > 0 ? r - 1 : grid - 1, r, grid - 1};
        for (int64_t bid : bids) {
          if (bid < 0 || bid >= grid || bid >= nwork) continue;
          const int steps = (int)((nwork - 1 - bid) / grid) + 1;   // (the kernels' expression)
          CHECK(steps == s || steps == s - 1, "steps %d of %d", steps, s);
          requests += walk<NWIN>(steps, bid, grid, blk0, stride, corpus_bytes);
          ++walks;
        }
      }
    }
    printf("nwin=%d depth=%d lead=%d grid=%lld blk0=%lld stride=%lld walks=%ld requests=%ld\n", NWIN, R::DEPTH, R::LEAD,
           (long long)grid, (long long)blk0, (long long)stride, walks, requests);
  }
}

int main() {
  all_walks<5>();
  all_walks<6>();
  printf("ok\n");
  return 0;
}
