"""Diversified search (MMR) timed on one GPU: per storage dtype and fetch_k the plain search, search_mmr,
the three MMR kernels from HIP events, and the same selection written in torch (what a user would write without it:
rows out of reconstruct_n by indexing, bmm for the Gram matrices, the greedy loop in torch ops).  One JSON document.

  python tools/mmr_probe.py --rows 1000000 --dim 768 --out profiles/mmr_probe.json
"""
import argparse
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


def torch_mmr(torch, rows, D, I, k, lam):
    """The baseline: gather by indexing, bmm, greedy loop in torch ops (f32).  rows: the stored rows as a device
    tensor (what reconstruct_n returns, uploaded once; the upload is not timed)."""
    X = rows[I.clamp(min=0)].float()                                 # [B, C, d]
    S = torch.bmm(X, X.transpose(1, 2))                              # [B, C, C]
    B, C = I.shape
    free = I >= 0
    maxsim = torch.full((B, C), float("-inf"), device=I.device)
    out = torch.full((B, k), -1, dtype=torch.int64, device=I.device)
    ar = torch.arange(B, device=I.device)
    for t in range(k):
        obj = D if t == 0 else lam * D - (1.0 - lam) * maxsim
        obj = torch.where(free, obj, torch.full_like(obj, float("-inf")))
        p = obj.argmax(dim=1)
        out[:, t] = I[ar, p]
        free[ar, p] = False
        maxsim = torch.maximum(maxsim, S[ar, p])
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--fetch", type=int, nargs="+", default=[100, 1024])
    ap.add_argument("--dtypes", nargs="+", default=["f16", "fp8"])
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default="profiles/mmr_probe.json")
    a = ap.parse_args()
    import torch
    from tristage_rag_amd.index import FlatIPIndex
    x = gen_rows(torch, a.rows, a.dim, 1)
    q = gen_rows(torch, a.batch, a.dim, 2)
    doc = {"rows": a.rows, "dim": a.dim, "batch": a.batch, "k": a.k, "lambda": a.lam, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "configs": []}
    for dt in a.dtypes:
        idx = FlatIPIndex(a.dim, dtype=dt)
        idx.reserve(a.rows)
        idx.add(x)
        # the baseline's rows: the stored values (fp8: decoded), kept as f16 on the device (exact for both dtypes)
        rows = x if dt == "f16" else torch.from_numpy(idx.reconstruct_n(0, a.rows)).cuda().half()
        for fk in a.fetch:
            r = {"dtype": dt, "fetch_k": fk}
            r["search_ms"] = timed(torch, lambda: idx.search(q, fk), a.rounds)
            r["search_mmr_ms"] = timed(torch, lambda: idx.search_mmr(q, a.k, fk, a.lam), a.rounds)
            D, I = idx.search(q, fk)
            r["mmr_ms"] = timed(torch, lambda: idx.mmr(I, D, a.k, a.lam), a.rounds)
            idx.mmr_timings(on=True)
            for _ in range(a.rounds):
                idx.mmr(I, D, a.k, a.lam)
            t = idx.mmr_timings(on=False)
            r["kernels_ms"] = {key: t[key] / max(t["calls"], 1) for key in ("gather_ms", "gram_ms", "greedy_ms")}
            r["torch_mmr_ms"] = timed(torch, lambda: torch_mmr(torch, rows, D, I, a.k, a.lam), a.rounds)
            got = idx.mmr(I, D, a.k, a.lam)[1]
            ref = torch_mmr(torch, rows, D, I, a.k, a.lam)
            r["picks_equal_torch"] = float((got == ref).float().mean().item())
            r["mmr_over_search"] = r["search_mmr_ms"]["median"] / r["search_ms"]["median"]
            r["torch_over_mmr"] = r["torch_mmr_ms"]["median"] / r["mmr_ms"]["median"]
            doc["configs"].append(r)
            print(json.dumps({k_: (v["median"] if isinstance(v, dict) and "median" in v else v) for k_, v in r.items()}),
                  flush=True)
        idx.close()
        del rows
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
