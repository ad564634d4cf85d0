"""The fp4 (4-bit MX) stage-1 index against the f16 and fp8 indexes in one process: ms per batch at
B = 1, 32 and 64 (k = 1000), synchronous and asynchronous, the three indexes' runs alternating; recall@10 / @100 /
@1000 of fp4 (and fp8) against the f16 ranking, and how much of the f16 top-k lies inside the fp4 top-4k, on the
benchmark's corpus generator.  The f16 and fp8 indexes are the yardstick: their kernels are not touched by fp4 storage.
Writes one JSON document.

  python tools/fp4_index_probe.py --rows 10000000 --dim 768 --out profiles/fp4_index_probe.json

Kernel times and bytes come from two profiler runs of the short form (--trace-only: build the indexes, three B = 64
searches each), whose CSVs a later call merges into the JSON:

  rocprofv3 --kernel-trace --stats --output-format csv -d prof/kt -o kt -- python tools/fp4_index_probe.py --trace-only
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d prof/pmc -o pmc -- python tools/fp4_index_probe.py --trace-only
  python tools/fp4_index_probe.py --merge prof --out profiles/fp4_index_probe.json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.fp8_index_probe import gen_rows, recall   # noqa: E402

DTYPES = ("f16", "fp8", "fp4")


def build(x, d, dtypes=DTYPES):
    from tristage_rag_amd.index import FlatIPIndex
    out = {}
    for dt in dtypes:
        idx = FlatIPIndex(d, dtype=dt)
        idx.classic_filter = True      # all on the five-launch path: the fp8 and fp4 indexes have no other
        idx.coalesce = False
        idx.reserve(x.shape[0])
        idx.add(x)
        out[dt] = idx
    return out


def stored_bytes(n, d):
    """Bytes a pass reads: fp4 row blocks are (dpad / 64 + ceil(dpad / 1024)) KiB with dpad a multiple of 256."""
    blocks = (n + 31) // 32
    dp4 = -(-d // 256) * 256
    return {"f16": blocks * 32 * (-(-d // 128) * 128) * 2, "fp8": blocks * 32 * (-(-d // 256) * 256),
            "fp4": blocks * 1024 * (dp4 // 64 + -(-dp4 // 1024))}


def time_alternating(torch, idxs, q, k, rounds, async_batches=8):
    """Per index the per-batch ms of `rounds` runs, the indexes alternating: synchronous searches one at a time, and
    `async_batches` asynchronous searches finished together."""
    res = {dt: {"sync_ms": [], "async_ms": []} for dt in idxs}
    for idx in idxs.values():          # warm-up: workspaces, LDS attributes
        idx.search(q, k)
    for _ in range(rounds):
        for dt, idx in idxs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            idx.search(q, k)
            torch.cuda.synchronize()
            res[dt]["sync_ms"].append(1e3 * (time.perf_counter() - t0))
        for dt, idx in idxs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(async_batches):
                idx.search(q, k, async_=True)
            idx.finish()
            torch.cuda.synchronize()
            res[dt]["async_ms"].append(1e3 * (time.perf_counter() - t0) / async_batches)
    out = {}
    for dt, r in res.items():
        out[dt] = {key: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for key, v in r.items()}
    # each ratio beside the spread of the fp8 runs it is measured against
    for key in ("sync_ms", "async_ms"):
        f8 = out["fp8"][key]
        out.setdefault("ratios", {})[key] = {
            "fp4_over_fp8": out["fp4"][key]["median"] / f8["median"],
            "fp4_over_f16": out["fp4"][key]["median"] / out["f16"][key]["median"],
            "fp8_spread_max_over_min": f8["max"] / f8["min"]}
    return out


def inside(I_small, I_ref, k, factor=4):
    """Share of the reference top-k that lies inside the first factor * k of I_small."""
    a, b = I_small[:, :factor * k].cpu(), I_ref[:, :k].cpu()
    return float(sum(len(set(x.tolist()) & set(y.tolist())) for x, y in zip(a, b)) / (k * b.shape[0]))


def merge(prof_dir, res):
    """Kernel statistics and FETCH_SIZE of the scan kernels from the two rocprofv3 runs."""
    scans = ("Op16<1>, WalkStrided>", "OpFp8, WalkStrided>", "OpFp4, WalkStridedFp4>")
    kt = {}
    for path in glob.glob(os.path.join(prof_dir, "kt", "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if any(s in row["Name"] for s in scans):
                kt[row["Name"]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                   "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    pmc = {}
    for path in glob.glob(os.path.join(prof_dir, "pmc", "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if row.get("Counter_Name") == "FETCH_SIZE" and any(s in row["Kernel_Name"] for s in scans):
                pmc.setdefault(row["Kernel_Name"], []).append(float(row["Counter_Value"]))
    res["kernel_trace"] = kt
    res["fetch_size_as_reported"] = {name: {"launches": len(v), "max": max(v), "values": v[:12]} for name, v in pmc.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--merge", default=None, help="directory of the two rocprofv3 runs (kt/, pmc/)")
    ap.add_argument("--out", default="profiles/fp4_index_probe.json")
    a = ap.parse_args()
    if a.merge:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        json.dump(merge(a.merge, res), open(a.out, "w"), indent=1)
        return
    import torch
    x = gen_rows(torch, a.rows, a.dim, seed=0)
    q = gen_rows(torch, 64, a.dim, seed=1)
    idxs = build(x, a.dim)
    if a.trace_only:
        for _ in range(3):
            for idx in idxs.values():
                idx.search(q, a.k)
        torch.cuda.synchronize()
        return
    res = {"rows": a.rows, "dim": a.dim, "k": a.k, "rounds": a.rounds, "stored_bytes": stored_bytes(a.rows, a.dim),
           "path": {dt: (idx.search(q, a.k), idx.last_search_info()["path"])[1] for dt, idx in idxs.items()}}
    for b in (1, 32, 64):
        res[f"b{b}"] = time_alternating(torch, idxs, q[:b].contiguous(), a.k, a.rounds)
        print(json.dumps({f"b{b}": {dt: {m: res[f"b{b}"][dt][m]["median"] for m in ("sync_ms", "async_ms")} for dt in idxs},
                          "ratios": res[f"b{b}"]["ratios"]}), flush=True)
    I = {dt: idx.search(q, a.k)[1] for dt, idx in idxs.items()}
    res["recall_vs_f16"] = {dt: {f"at_{kk}": recall(I[dt], I["f16"], kk) for kk in (10, 100, 1000)} for dt in ("fp8", "fp4")}
    # 4 k <= 2048 keeps the filter path: the f16 top-k inside the fp4 top-4k for k = 10, 100, 500
    I4 = idxs["fp4"].search(q, 2000)[1]
    res["f16_top_k_inside_fp4_top_4k"] = {f"k_{kk}": inside(I4, I["f16"], kk) for kk in (10, 100, 500)}
    print(json.dumps({"recall_vs_f16": res["recall_vs_f16"], "inside": res["f16_top_k_inside_fp4_top_4k"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
