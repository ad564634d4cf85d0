"""Funnel search timed on one GPU, synchronous calls in one process: search, search_prefix, rescore
and search_funnel per (dims, k) at the default fetch_k, the filter-scan kernel time of the full and the prefix pass
from HIP events with the bytes each reads, and recall@k of the funnel against search on two SYNTHETIC inputs (random
unit rows, which have no Matryoshka structure, and rows whose per-dimension scale decays as (1 + j)^-1/2).  One JSON
document.

  python tools/funnel_probe.py --rows 10000000 --dim 768 --out profiles/funnel_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gen_rows(torch, n, d, seed, decay=False, chunk=1 << 20):
    """bench.py's generator (unit-norm Gaussian rows), f16, in chunks; decay: dimension j scaled by (1 + j)^-1/2 first."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((n, d), dtype=torch.float16, device="cuda")
    scale = (1.0 + torch.arange(d, device="cuda", dtype=torch.float32)).rsqrt() if decay else None
    for r0 in range(0, n, chunk):
        x = torch.randn((min(n, r0 + chunk) - r0, d), generator=g, device="cuda", dtype=torch.float32)
        if decay:
            x = x * scale
        out[r0:r0 + x.shape[0]] = (x / (x.norm(dim=1, keepdim=True) + 1e-8)).half()
    return out


def timed(torch, fn, rounds):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


def scan_kernel_ms(torch, idx, fn, rounds):
    """Mean HIP-event time of the filter-scan kernel over ``rounds`` calls of ``fn``."""
    idx.set_profiling(True)
    idx.timings(reset=True)
    for _ in range(rounds):
        fn()
    torch.cuda.synchronize()
    ms, cnt = idx.timings(reset=True)["filter_scan"]
    idx.set_profiling(False)
    return ms / max(cnt, 1)


def recall(torch, idx, q, dims_list, ks):
    out = []
    for k in ks:
        want = idx.search(q, k)[1]
        for dims in dims_list:
            got = idx.search_funnel(q, k, dims)[1]
            hit = (got.unsqueeze(2) == want.unsqueeze(1)).any(dim=2).float().sum(dim=1) / k
            out.append({"dims": dims, "k": k, "fetch_k": idx.last_funnel_info()["fetch_k"],
                        "recall_mean": float(hit.mean().item()), "recall_min": float(hit.min().item())})
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--recall-rows", type=int, default=2_000_000, help="rows of the decaying-scale corpus")
    ap.add_argument("--out", default="profiles/funnel_probe.json")
    a = ap.parse_args()
    import torch
    from tristage_rag_amd.index import FlatIPIndex, funnel_default_fetch_k
    doc = {"rows": a.rows, "dim": a.dim, "batch": a.batch, "dtype": "f16", "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "what": "synchronous calls, host wall clock per batch (ms); "
           "scan: HIP-event time of the filter-scan kernel and the bytes it reads", "configs": []}
    idx = FlatIPIndex(a.dim, dtype="f16")
    idx.reserve(a.rows)
    idx.add(gen_rows(torch, a.rows, a.dim, 1))
    q = gen_rows(torch, a.batch, a.dim, 2)
    kg = (a.dim + 127) // 128 * 8
    blocks = (a.rows + 31) // 32
    doc["read_probe"] = idx.read_probe()
    for k in a.k:
        fk = funnel_default_fetch_k(k)
        base = {"k": k, "search_ms": timed(torch, lambda: idx.search(q, k), a.rounds),
                "search_fetch_ms": timed(torch, lambda: idx.search(q, fk), a.rounds)}
        ms = scan_kernel_ms(torch, idx, lambda: idx.search(q, k, classic=True), a.rounds)
        base["full_scan"] = {"kernel_ms": ms, "bytes": blocks * kg * 1024, "gbps": blocks * kg * 1024 / (ms * 1e-3) / 1e9}
        print(json.dumps({"k": k, "search_ms": base["search_ms"]["median"], "full_scan": base["full_scan"]}), flush=True)
        for dims in a.dims:
            r = dict(base, dims=dims, fetch_k=fk)
            r["search_prefix_ms"] = timed(torch, lambda: idx.search_prefix(q, fk, dims), a.rounds)
            cand = idx.search_prefix(q, fk, dims)[1]
            r["rescore_ms"] = timed(torch, lambda: idx.rescore(q, cand, k), a.rounds)
            r["search_funnel_ms"] = timed(torch, lambda: idx.search_funnel(q, k, dims), a.rounds)
            r["prefix_path"] = idx.last_funnel_info()["prefix_path"]
            ms = scan_kernel_ms(torch, idx, lambda: idx.search_prefix(q, fk, dims), a.rounds)
            nbytes = blocks * (dims // 16) * 1024
            r["prefix_scan"] = {"kernel_ms": ms, "bytes": nbytes, "gbps": nbytes / (ms * 1e-3) / 1e9}
            r["prefix_scan_over_full_scan"] = ms / base["full_scan"]["kernel_ms"]
            r["funnel_over_search"] = r["search_funnel_ms"]["median"] / r["search_ms"]["median"]
            doc["configs"].append(r)
            print(json.dumps({k_: (v["median"] if isinstance(v, dict) and "median" in v else v) for k_, v in r.items()
                              if k_ not in ("search_fetch_ms",)}), flush=True)
    doc["recall"] = {"note": "SYNTHETIC inputs only; nothing here says anything about a trained encoder's recall",
                     "random_unit_rows": {"rows": a.rows, "results": recall(torch, idx, q, a.dims, a.k)}}
    idx.close()
    del idx
    torch.cuda.empty_cache()
    idx = FlatIPIndex(a.dim, dtype="f16")
    idx.add(gen_rows(torch, a.recall_rows, a.dim, 3, decay=True))
    qd = gen_rows(torch, a.batch, a.dim, 4, decay=True)
    doc["recall"]["decaying_scale_rows"] = {"rows": a.recall_rows, "scale": "(1 + j)^-1/2 per dimension j, then unit norm",
                                            "results": recall(torch, idx, qd, a.dims, a.k)}
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
