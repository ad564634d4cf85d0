#!/usr/bin/env python3
"""Per-wave phase sums of the last wide coalesced pass (needs a -DTS_TUNING -DWIDE_TRACE build in TRISTAGE_LIB).

    python tools/trace_wide.py [--rows 10000000] [--dim 768] [--batches 3] [--json OUT]

Submits `--batches` asynchronous batches of 64 queries (k = 1000) a few times, so the last scan launch is one wide
pass of 2 x batches groups, and prints, per phase of scan_wide_kernel's window (ts_scan.hip, WIDE_TRACE), the mean
time per window and its share of the walk, over the traced waves; plus the ratio of the s_memtime count to the
100 MHz clock.  The stamps wait for the window's first-slot operand reads in one piece, which the untraced walk does not, so
the traced pass is slightly slower than the untraced one.  Each phase is also given for the first and the second half of
a workgroup's waves: with staggered requests (TS_WIDE_STAGGER) the second half requests inside the slots phase."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tristage_rag_amd import _lib  # noqa: E402
from tristage_rag_amd.index import FlatIPIndex  # noqa: E402

ROW, WAVES, WGS = 10, 8, 256
PHASES = ["gather requests", "first-slot operand reads", "slots: MFMAs, re-reads, refills", "fill pointer + epilogue",
          "vmcnt wait (next window's units)", "barrier"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    idx = FlatIPIndex(args.dim, dtype="f16")
    idx.reserve(args.rows)
    for r0 in range(0, args.rows, 1 << 20):
        n = min(1 << 20, args.rows - r0)
        idx.add(torch.randn((n, args.dim), generator=g, device="cuda", dtype=torch.float16), normalize=True)
    qs = [torch.nn.functional.normalize(torch.randn((64, args.dim), generator=g, device="cuda"), dim=1).half()
          for _ in range(args.batches)]
    idx.wide_passes = True
    for _ in range(4):
        for q in qs:
            idx.search(q, 1000, async_=True)
        assert idx.finish() == []
    torch.cuda.synchronize()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    buf = (ctypes.c_uint32 * (WGS * WAVES * ROW))()
    assert lib.ts_debug_wide_trace(buf) == 0
    t = np.frombuffer(buf, dtype=np.uint32).reshape(WGS * WAVES, ROW).astype(np.float64)
    half = (np.arange(WGS * WAVES) % WAVES >= WAVES // 2)[t[:, 8] > 0]   # the waves that request late when staggered
    t = t[t[:, 8] > 0]
    nwin = t[:, 8]
    walk_us = t[:, 6] / 100.0
    out = {"rows": args.rows, "dim": args.dim, "groups": 2 * args.batches, "waves_traced": int(t.shape[0]),
           "windows_per_wave": [int(nwin.min()), int(nwin.max())],
           "walk_us": {"median": round(float(np.median(walk_us)), 1), "max": round(float(walk_us.max()), 1)},
           "memtime_counts_per_100MHz_tick": round(float((t[:, 7] / t[:, 6]).mean()), 3), "phases": {}}
    print(f"{t.shape[0]} waves traced, {int(nwin.min())}-{int(nwin.max())} windows each; walk median "
          f"{np.median(walk_us):.1f} us, max {walk_us.max():.1f} us; s_memtime counts per 100 MHz tick "
          f"{out['memtime_counts_per_100MHz_tick']}")
    for k, name in enumerate(PHASES):
        per_win_ns = t[:, k] * 10.0 / nwin
        share = t[:, k] / t[:, 6]
        out["phases"][name] = {"ns_per_window_mean": round(float(per_win_ns.mean()), 1),
                               "ns_per_window_p5_p95": [round(float(np.percentile(per_win_ns, 5)), 1),
                                                        round(float(np.percentile(per_win_ns, 95)), 1)],
                               "share_of_walk": round(float(share.mean()), 4),
                               "ns_per_window_mean_waves_0_3_4_7": [round(float(per_win_ns[~half].mean()), 1),
                                                                    round(float(per_win_ns[half].mean()), 1)]}
        print(f"  {k} {name:34s} {per_win_ns.mean():8.1f} ns per window (p5 {np.percentile(per_win_ns, 5):7.1f}, "
              f"p95 {np.percentile(per_win_ns, 95):7.1f})  {100 * share.mean():5.1f} % of the walk; "
              f"waves 0-3 {per_win_ns[~half].mean():7.1f}, 4-7 {per_win_ns[half].mean():7.1f}")
    idx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
