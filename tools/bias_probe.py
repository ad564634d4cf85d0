"""Boosted search on the bench shape (10 M x 768 f16, B = 64, k = 1000, one GPU), in the protocol of
tools/filter_probe.py: ms per batch, synchronous and 20 batches back to back, in one process, of

    search                 FlatIPIndex.search
    search_all_ones        FlatIPIndex.search(allowed = every row): the masked scan over every row block (the yardstick)
    biased                 FlatIPIndex.search_biased, bias ~ normal(0, 0.05)
    biased_random_10pct    the same bias and a 10 % random mask
    torch_scores_topk      scores() + bias, torch.topk: what a caller can do without search_biased

    python tools/bias_probe.py [--rows N] [--steps S] [--out profiles/bias_probe.json]
    python tools/bias_probe.py --only biased --steps 3      (one row, for a rocprofv3 --pmc FETCH_SIZE run)

search_biased is synchronous (it returns with its stream drained), so its back-to-back figure is the loop of
synchronous calls; search / search(allowed=) are measured with async_=True and one finish(), as filter_probe.py does.
Every boosted row is checked once against scores() + bias (values bit for bit) before it is timed.
tools/filter_pmc_summary.py adds the FETCH_SIZE of such a run to the JSON (its kernel filter matches the biased scan)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ROWS = ["search", "search_all_ones", "biased", "biased_random_10pct", "torch_scores_topk"]


def gen_rows(torch, n, d, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=device, dtype=torch.float32)
    return (x / (x.norm(dim=1, keepdim=True) + 1e-8)).half()


def packed(torch, m, n, device):
    from tristage_rag_amd.index import pack_allowed
    return torch.from_numpy(pack_allowed(m.cpu().numpy(), n).view(np.int32)).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, choices=ROWS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from tristage_rag_amd.index import FlatIPIndex
    dev = torch.device("cuda", 0)
    n = args.rows
    idx = FlatIPIndex(args.dim, dtype="f16", device=0)
    idx.reserve(n)
    blk = 1 << 20
    for r0 in range(0, n, blk):
        idx.add(gen_rows(torch, min(blk, n - r0), args.dim, 1234 + r0 // blk, dev))
    torch.cuda.synchronize()
    qs = [gen_rows(torch, args.batch, args.dim, 99 + s, dev) for s in range(4)]
    g = torch.Generator(device=dev).manual_seed(7)
    bias = 0.05 * torch.randn(n, generator=g, device=dev, dtype=torch.float32)
    ones = packed(torch, torch.ones(n, dtype=torch.bool, device=dev), n, dev)
    tenth_mask = torch.rand(n, generator=g, device=dev) < 0.10
    tenth = packed(torch, tenth_mask, n, dev)
    total_blocks = (n + 31) // 32
    out = {"shape": {"rows": n, "dim": args.dim, "batch": args.batch, "k": args.k, "dtype": "f16"},
           "total_blocks": total_blocks, "corpus_bytes": total_blocks * 32 * args.dim * 2, "bias_bytes": 4 * n, "rows": {}}

    def torch_topk(q):
        s = idx.scores(q)
        s += bias
        return torch.topk(s, args.k, dim=1)

    calls = {
        "search": (lambda q, **kw: idx.search(q, args.k, **kw), True),
        "search_all_ones": (lambda q, **kw: idx.search(q, args.k, allowed=ones, **kw), True),
        "biased": (lambda q: idx.search_biased(q, args.k, bias, check_finite=False), False),
        "biased_random_10pct": (lambda q: idx.search_biased(q, args.k, bias, allowed=tenth, check_finite=False), False),
        "torch_scores_topk": (torch_topk, False),
    }
    for row in ([args.only] if args.only else ROWS):
        call, has_async = calls[row]
        rec = {}
        if row.startswith("biased"):
            # correctness once, on four queries: the values of scores() + bias, bit for bit, and the torch selection's ids
            D, I = call(qs[0])
            S = idx.scores(qs[0][:4]) + bias
            if row == "biased_random_10pct":
                S = torch.where(tenth_mask[None, :], S, torch.full_like(S, -3.0e38))
            for q in range(4):
                assert torch.equal(S[q, I[q]].view(torch.int32), D[q].view(torch.int32)), row
                assert torch.equal(torch.topk(S[q], args.k).values.view(torch.int32), D[q].view(torch.int32)), row
            del S
            info = idx.last_bias_info()
            # (live_bytes: the row blocks the scan read and their 128 bytes of bias each; tools/filter_pmc_summary.py puts
            # the FETCH_SIZE of a rocprofv3 --pmc run over it)
            rec.update(info, read_fraction=round(info["blocks_read"] / total_blocks, 5),
                       live_bytes=info["blocks_read"] * (32 * args.dim * 2 + 128))
        for _ in range(3):
            call(qs[1])
        torch.cuda.synchronize()
        t = time.perf_counter()
        for s in range(args.steps):
            call(qs[s % 4])
        torch.cuda.synchronize()
        rec["ms_per_batch_sync"] = round((time.perf_counter() - t) * 1e3 / args.steps, 4)
        if has_async:
            idx.finish()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for s in range(args.steps):
                call(qs[s % 4], async_=True)
            rec["async_redone"] = len(idx.finish())
            torch.cuda.synchronize()
            rec["ms_per_batch_async"] = round((time.perf_counter() - t) * 1e3 / args.steps, 4)
        else:
            rec["ms_per_batch_async"] = None      # no asynchronous form: back to back is the synchronous loop
        out["rows"][row] = rec
        print(row, json.dumps(rec), flush=True)
    idx.close()
    r = out["rows"]
    if not args.only:
        out["summary"] = {
            "biased_over_all_ones_sync": round(r["biased"]["ms_per_batch_sync"] / r["search_all_ones"]["ms_per_batch_sync"], 4),
            "biased_sync_over_all_ones_async": round(r["biased"]["ms_per_batch_sync"] / r["search_all_ones"]["ms_per_batch_async"], 4),
            "torch_over_biased_sync": round(r["torch_scores_topk"]["ms_per_batch_sync"] / r["biased"]["ms_per_batch_sync"], 2),
        }
        print("summary", json.dumps(out["summary"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
