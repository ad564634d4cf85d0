"""A/B of coalesced passes (TS_FLAG_COALESCE): batches of 64 queries, k = 1000, submitted back to back with
async_=True and completed by one finish(), with `coalesce` on and off on the same index.  Prints one JSON object.

    python tools/coalesce_probe.py [--rows 1250000] [--dim 768] [--steps 20] [--reps 3] [--modes classic]
                                   [--wide auto True False]

Modes per shape: the default path (one-launch at <= 4 M rows, five-launch above), the five-launch path
(classic) and the pipelined path (inputs_ready=True, which never coalesces).  --wide: the FlatIPIndex.wide_passes
settings the coalesced runs take, one run each (wide passes)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_250_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["default", "classic", "pipelined"],
                    choices=["default", "classic", "pipelined"])
    ap.add_argument("--wide", nargs="+", default=["auto"], choices=["auto", "True", "False"])
    args = ap.parse_args()
    import torch
    from tristage_rag_amd.index import FlatIPIndex
    out = {"dim": args.dim, "batch": args.batch, "k": args.k, "steps": args.steps, "results": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for rows in args.rows:
        idx = FlatIPIndex(args.dim, dtype="f16")
        idx.reserve(rows)
        for r0 in range(0, rows, 1 << 20):
            n = min(1 << 20, rows - r0)
            idx.add(torch.randn((n, args.dim), generator=g, device="cuda", dtype=torch.float16), normalize=True)
        qs = [torch.nn.functional.normalize(torch.randn((args.batch, args.dim), generator=g, device="cuda"), dim=1)
              .half() for _ in range(4)]
        torch.cuda.synchronize()
        for mode in args.modes:
            idx.classic_filter = mode == "classic"
            for co, wide in [(False, "auto")] + [(True, w) for w in args.wide]:
                idx.coalesce = co
                idx.wide_passes = {"auto": "auto", "True": True, "False": False}[wide]
                ms = []
                for rep in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(args.steps):
                        idx.search(qs[i % 4], args.k, async_=True, inputs_ready=mode == "pipelined")
                    redone = idx.finish()
                    torch.cuda.synchronize()
                    if rep:   # the first repetition warms up
                        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
                    assert redone == [], redone
                out["results"].append({"rows": rows, "mode": mode, "coalesce": co, "wide_passes": wide,
                                       "ms_per_batch": [round(x, 4) for x in ms],
                                       "qps_best": round(args.batch / (min(ms) * 1e-3), 1)})
                print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
        idx.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
