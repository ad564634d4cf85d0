"""The fp8 (e4m3) stage-1 index against the f16 index in one process: ms per batch at B = 1 and
B = 64 (k = 1000), synchronous and asynchronous, the two indices' runs alternating; recall@10 / @100 / @1000 of fp8
against f16 on the benchmark's corpus generator and on the clustered mixture of 4.9.  Writes one JSON document.

  python tools/fp8_index_probe.py --rows 10000000 --dim 768 --out profiles/fp8_index_probe.json

Kernel times and bytes come from two profiler runs of the short form (--trace-only: build both indices, three B = 64
searches each), whose CSVs a later call merges into the JSON:

  rocprofv3 --kernel-trace --stats --output-format csv -d prof/kt -o kt -- python tools/fp8_index_probe.py --trace-only
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d prof/pmc -o pmc -- python tools/fp8_index_probe.py --trace-only
  python tools/fp8_index_probe.py --merge prof --out profiles/fp8_index_probe.json
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


def gen_rows(torch, n, d, seed, chunk=1 << 20):
    """bench.py's generator (unit-norm Gaussian rows), f16, in chunks."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((n, d), dtype=torch.float16, device="cuda")
    for r0 in range(0, n, chunk):
        x = torch.randn((min(n, r0 + chunk) - r0, d), generator=g, device="cuda", dtype=torch.float32)
        out[r0:r0 + x.shape[0]] = (x / (x.norm(dim=1, keepdim=True) + 1e-8)).half()
    return out


def recall(I, I0, k):
    I, I0 = I[:, :k].cpu(), I0[:, :k].cpu()
    return float(sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(I, I0)) / (k * I.shape[0]))


def build(torch, x, d):
    from tristage_rag_amd.index import FlatIPIndex
    out = {}
    for dt in ("f16", "fp8"):
        idx = FlatIPIndex(d, dtype=dt)
        idx.classic_filter = True      # both on the five-launch path: the fp8 index has no other
        idx.coalesce = False
        idx.reserve(x.shape[0])
        idx.add(x)
        out[dt] = idx
    return out


def time_alternating(torch, idxs, q, k, rounds, async_batches=8):
    """Per index the per-batch ms of `rounds` runs, f16 and fp8 alternating: synchronous searches one at a time, and
    `async_batches` asynchronous searches finished together."""
    res = {dt: {"sync_ms": [], "async_ms": []} for dt in idxs}
    for dt, idx in idxs.items():       # warm-up: workspaces, LDS attributes
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
    return out


def merge(prof_dir, res):
    """Kernel statistics and FETCH_SIZE of the scan kernels from the two rocprofv3 runs."""
    # the dense / filter scans of the 16-bit and the e4m3 index: scan_kernel<QH, MODE, Op16<DT> | OpFp8, WalkStrided>
    scans = ("Op16<0>, WalkStrided>", "Op16<1>, WalkStrided>", "Op16<2>, WalkStrided>", "OpFp8, WalkStrided>")
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
    ap.add_argument("--centers", type=int, default=2000)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--merge", default=None, help="directory of the two rocprofv3 runs (kt/, pmc/)")
    ap.add_argument("--out", default="profiles/fp8_index_probe.json")
    a = ap.parse_args()
    if a.merge:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        json.dump(merge(a.merge, res), open(a.out, "w"), indent=1)
        return
    import torch
    from tools.ivf_probe import clustered
    x = gen_rows(torch, a.rows, a.dim, seed=0)
    q = gen_rows(torch, 64, a.dim, seed=1)
    idxs = build(torch, x, a.dim)
    if a.trace_only:
        for _ in range(3):
            for idx in idxs.values():
                idx.search(q, a.k)
        torch.cuda.synchronize()
        return
    res = {"rows": a.rows, "dim": a.dim, "k": a.k, "rounds": a.rounds,
           "corpus_bytes": {"f16": a.rows * a.dim * 2, "fp8": a.rows * a.dim},
           "path": {dt: (idx.search(q, a.k), idx.last_search_info()["path"])[1] for dt, idx in idxs.items()},
           "b1": time_alternating(torch, idxs, q[:1].contiguous(), a.k, a.rounds),
           "b64": time_alternating(torch, idxs, q, a.k, a.rounds)}
    print(json.dumps({b: {dt: {m: res[b][dt][m]["median"] for m in ("sync_ms", "async_ms")} for dt in idxs}
                      for b in ("b1", "b64")}), flush=True)
    I16, I8 = idxs["f16"].search(q, a.k)[1], idxs["fp8"].search(q, a.k)[1]
    res["recall_gaussian"] = {f"at_{kk}": recall(I8, I16, kk) for kk in (10, 100, 1000)}
    for idx in idxs.values():
        idx.close()
    del idxs, x
    torch.cuda.empty_cache()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = clustered(a.rows, a.dim, a.centers, gen)
    q = clustered(64, a.dim, a.centers, torch.Generator(device="cuda").manual_seed(1))
    idxs = build(torch, x, a.dim)
    I16, I8 = idxs["f16"].search(q, a.k)[1], idxs["fp8"].search(q, a.k)[1]
    res["recall_mixture"] = {"centers": a.centers, **{f"at_{kk}": recall(I8, I16, kk) for kk in (10, 100, 1000)}}
    print(json.dumps({"recall_gaussian": res["recall_gaussian"], "recall_mixture": res["recall_mixture"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
