"""Removal on the bench shape (10 M x 768 f16, B = 64, k = 1000, one GPU): ms per batch of FlatIPIndex.search after
remove_ids, synchronous and asynchronous (wide coalesced passes where the index has no removed row; back to back, one
finish()), for the cases of DESIGN.md 4.11, plus the time of remove_ids for 100 k ids and of compact() at 1 %.

    python tools/remove_probe.py [--rows N] [--steps S] [--out profiles/remove_probe.json]

Every case is checked once before it is timed: no removed id comes back, and the result equals the filtered search
of the live rows (scores and ids bit for bit)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def gen_rows(torch, n, d, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=device, dtype=torch.float32)
    return (x / (x.norm(dim=1, keepdim=True) + 1e-8)).half()


def build(torch, args, dev):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(args.dim, dtype="f16", device=0)
    idx.reserve(args.rows)
    blk = 1 << 20
    for r0 in range(0, args.rows, blk):
        idx.add(gen_rows(torch, min(blk, args.rows - r0), args.dim, 1234 + r0 // blk, dev))
    torch.cuda.synchronize()
    return idx


def time_case(torch, idx, qs, args, removed):
    # correctness once
    D, I = idx.search(qs[0], args.k)
    path = idx.last_search_info()["path"]
    if removed is not None and removed.size:
        assert not np.isin(I.cpu().numpy(), removed).any()
        live = idx.live_mask()
        D2, I2 = idx.search(qs[0], args.k, allowed=live)
        assert torch.equal(I, I2) and torch.equal(D.view(torch.int32), D2.view(torch.int32))
    for _ in range(3):
        idx.search(qs[1], args.k)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for s in range(args.steps):
        idx.search(qs[s % len(qs)], args.k)
    torch.cuda.synchronize()
    sync_ms = (time.perf_counter() - t) * 1e3 / args.steps
    idx.wide_passes = True
    for s in range(6):
        idx.search(qs[s % len(qs)], args.k, async_=True)
    idx.finish()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for s in range(args.steps):
        idx.search(qs[s % len(qs)], args.k, async_=True)
    redone = idx.finish()
    torch.cuda.synchronize()
    async_ms = (time.perf_counter() - t) * 1e3 / args.steps
    idx.wide_passes = "auto"
    return {"removed": 0 if removed is None else int(removed.size), "nlive": idx.nlive, "path_sync": path,
            "ms_per_batch_sync": round(sync_ms, 4), "ms_per_batch_async_wide": round(async_ms, 4),
            "async_redone": len(redone)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    n = args.rows
    qs = [gen_rows(torch, args.batch, args.dim, 99 + s, dev) for s in range(6)]
    out = {"shape": {"rows": n, "dim": args.dim, "batch": args.batch, "k": args.k, "dtype": "f16"}, "cases": {}}
    rng = np.random.default_rng(7)
    prio = rng.random(n)

    def record(name, rec):
        out["cases"][name] = rec
        print(name, json.dumps(rec), flush=True)

    # nested random removals on one index: none, 0.1 %, 1 %, 10 %
    idx = build(torch, args, dev)
    record("none", time_case(torch, idx, qs, args, None))
    done = np.zeros(n, bool)
    for frac, name in ((0.001, "random_0.1pct"), (0.01, "random_1pct"), (0.10, "random_10pct")):
        ids = np.flatnonzero((prio < frac) & ~done)
        torch.cuda.synchronize()
        t = time.perf_counter()
        got = idx.remove_ids(ids)
        rm_ms = (time.perf_counter() - t) * 1e3
        assert got == ids.size
        done[ids] = True
        rec = time_case(torch, idx, qs, args, np.flatnonzero(done))
        rec["remove_ids_ms"] = round(rm_ms, 3)
        rec["remove_ids_count"] = int(ids.size)
        record(name, rec)
    idx.close()
    # contiguous 10 %
    idx = build(torch, args, dev)
    ids = np.arange(n // 2, n // 2 + n // 10)
    idx.remove_ids(ids)
    record("contiguous_10pct", time_case(torch, idx, qs, args, ids))
    idx.close()
    # adversarial: every query's own exact top-k of the timed batches
    idx = build(torch, args, dev)
    ids = np.unique(np.concatenate([idx.search(q, args.k)[1].cpu().numpy().reshape(-1) for q in qs]))
    idx.remove_ids(ids)
    record("adversarial_topk", time_case(torch, idx, qs, args, ids))
    idx.close()
    # remove_ids of 100 k ids on a fresh index (the first removal writes the bitmap), then compact() at 1 %
    idx = build(torch, args, dev)
    ids = np.flatnonzero(prio < 0.01)[:100_000]
    torch.cuda.synchronize()
    t = time.perf_counter()
    idx.remove_ids(ids)
    out["remove_ids_100k_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    ids = np.flatnonzero(prio < 0.01)
    idx.remove_ids(ids)
    live = np.ones(n, bool)
    live[ids] = False
    sample = np.sort(rng.choice(np.flatnonzero(live), 2000, replace=False))
    rows_before = np.concatenate([idx.reconstruct_n(int(r), 1) for r in sample])
    pre_D, pre_I = idx.search(qs[0], args.k)
    torch.cuda.synchronize()
    t = time.perf_counter()
    old2new = idx.compact()
    torch.cuda.synchronize()
    out["compact_1pct_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    out["compact_1pct_moved_bytes"] = int(np.count_nonzero(old2new[old2new >= 0] != np.flatnonzero(old2new >= 0))) * args.dim * 2
    assert idx.ntotal == n - ids.size
    assert np.array_equal(old2new[live], np.arange(n - ids.size)) and (old2new[~live] == -1).all()
    assert np.array_equal(np.concatenate([idx.reconstruct_n(int(old2new[r]), 1) for r in sample]), rows_before)
    D, I = idx.search(qs[0], args.k)
    pi = pre_I.cpu().numpy()
    assert np.array_equal(I.cpu().numpy(), old2new[pi]) and torch.equal(D.view(torch.int32), pre_D.view(torch.int32))
    # after compaction the index has no removed row: the unfiltered paths again
    record("after_compact_1pct", time_case(torch, idx, qs, args, None))
    idx.close()
    print("remove_ids_100k_ms", out["remove_ids_100k_ms"], "compact_1pct_ms", out["compact_1pct_ms"], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
