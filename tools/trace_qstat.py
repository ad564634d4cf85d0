#!/usr/bin/env python3
"""Per-wave phase sums of the last query-stationary pass (needs a -DTS_TUNING -DQSTAT_TRACE build in TRISTAGE_LIB).

    python tools/trace_qstat.py [--rows 10000000] [--dim 768] [--batches 4] [--json OUT]

Submits `--batches` asynchronous batches of 64 queries (k = 1000) a few times, so the last scan launch is one
stationary pass of 2 x batches groups, and prints, per phase of scan_qstat_kernel's step (ts_scan_qstat.hip,
QSTAT_TRACE), the mean time per step with its p5 and p95 over the traced waves, for waves 0-3 and 4-7 of a workgroup,
and its share of the walk; plus the in-kernel clock: s_memtime counts per 100 MHz tick of s_memrealtime.  A stamp is a
scalar memory read and waits lgkmcnt(0) itself, so the first-MFMA stamp waits for the step's first four operand reads in
one piece, which the untraced walk does not: the traced pass is slightly slower than the untraced one."""
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
PHASES = ["step start -> first MFMA (offsets, first reads)", "first MFMA -> last MFMA", "survivor test",
          "counted wait (next block's pieces)", "barrier", "requests + ring advance"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batches", type=int, default=4)
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
    idx.stationary_passes = True
    for _ in range(4):
        for q in qs:
            idx.search(q, 1000, async_=True)
        assert idx.finish() == []
    torch.cuda.synchronize()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    buf = (ctypes.c_uint32 * (WGS * WAVES * ROW))()
    assert lib.ts_debug_qstat_trace(buf) == 0
    t = np.frombuffer(buf, dtype=np.uint32).reshape(WGS * WAVES, ROW).astype(np.float64)
    half = (np.arange(WGS * WAVES) % WAVES >= WAVES // 2)[t[:, 8] > 0]
    t = t[t[:, 8] > 0]
    steps = t[:, 8]
    walk_us = t[:, 6] / 100.0
    counts_per_tick = float((t[:, 7] / t[:, 6]).mean())
    out = {"rows": args.rows, "dim": args.dim, "groups": 2 * args.batches, "waves_traced": int(t.shape[0]),
           "steps_per_wave": [int(steps.min()), int(steps.max())],
           "walk_us": {"median": round(float(np.median(walk_us)), 1), "max": round(float(walk_us.max()), 1)},
           "ns_per_step": round(float((t[:, 6] * 10.0 / steps).mean()), 1),
           "memtime_counts_per_100MHz_tick": round(counts_per_tick, 3), "phases": {}}
    print(f"{t.shape[0]} waves traced, {int(steps.min())}-{int(steps.max())} steps each; walk median "
          f"{np.median(walk_us):.1f} us, max {walk_us.max():.1f} us, {out['ns_per_step']} ns per step; s_memtime counts "
          f"per 100 MHz tick {out['memtime_counts_per_100MHz_tick']}")
    for k, name in enumerate(PHASES):
        ns = t[:, k] * 10.0 / steps
        share = t[:, k] / t[:, 6]
        stat = lambda x: [round(float(x.mean()), 1), round(float(np.percentile(x, 5)), 1),   # noqa: E731
                          round(float(np.percentile(x, 95)), 1)]
        out["phases"][name] = {"ns_per_step_mean_p5_p95": stat(ns), "waves_0_3_mean_p5_p95": stat(ns[~half]),
                               "waves_4_7_mean_p5_p95": stat(ns[half]), "share_of_walk": round(float(share.mean()), 4)}
        a, b = stat(ns[~half]), stat(ns[half])
        print(f"  {k} {name:48s} {ns.mean():7.1f} ns per step  {100 * share.mean():5.1f} % of the walk; waves 0-3 "
              f"{a[0]:7.1f} (p5 {a[1]:7.1f}, p95 {a[2]:7.1f}), 4-7 {b[0]:7.1f} (p5 {b[1]:7.1f}, p95 {b[2]:7.1f})")
    idx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
