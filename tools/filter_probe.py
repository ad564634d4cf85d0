"""Filtered search on the bench shape (10 M x 768 f16, B = 64, k = 1000, one GPU): ms per batch of
FlatIPIndex.search(..., allowed=) for the rows of the filter table in DESIGN.md (section 4.8), synchronous and
asynchronous (back to back, one finish()), with the row blocks the masked scan read.

    python tools/filter_probe.py [--rows N] [--steps S] [--out profiles/filter_probe.json]
    python tools/filter_probe.py --only ROW --steps 3      (one row, for a rocprofv3 --pmc FETCH_SIZE run)

Every row is checked once against the unfiltered search on its allowed ids (scores bit for bit) before it is timed.
The unfiltered line (no allowed=) is measured the same way as the reference point."""
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


def masks_for(row, n, torch, device):
    """-> (allowed for search(), fraction of rows allowed)"""
    g = torch.Generator(device=device).manual_seed(7)
    if row == "unfiltered":
        return None, 1.0
    if row == "all_100pct":
        m = torch.ones(n, dtype=torch.bool, device=device)
    elif row == "random_10pct":
        m = torch.rand(n, generator=g, device=device) < 0.10
    elif row == "contiguous_1pct":
        m = torch.zeros(n, dtype=torch.bool, device=device)
        m[n // 2: n // 2 + n // 100] = True
    elif row == "tenant_10k":
        m = torch.zeros(n, dtype=torch.bool, device=device)
        m[3 * n // 4: 3 * n // 4 + 10_000] = True
    elif row == "random_0.1pct":
        m = torch.rand(n, generator=g, device=device) < 0.001
    else:
        raise ValueError(row)
    from tristage_rag_amd.index import pack_allowed
    words = pack_allowed(m.cpu().numpy(), n)
    return torch.from_numpy(words.view(np.int32)).to(device), float(m.float().mean())


ROWS = ["unfiltered", "all_100pct", "random_10pct", "contiguous_1pct", "tenant_10k", "random_0.1pct"]


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
    idx = FlatIPIndex(args.dim, dtype="f16", device=0)
    idx.reserve(args.rows)
    blk = 1 << 20
    for r0 in range(0, args.rows, blk):
        idx.add(gen_rows(torch, min(blk, args.rows - r0), args.dim, 1234 + r0 // blk, dev))
    torch.cuda.synchronize()
    qs = [gen_rows(torch, args.batch, args.dim, 99 + s, dev) for s in range(4)]
    D0, I0 = idx.search(qs[0], args.k)
    S0 = None
    out = {"shape": {"rows": args.rows, "dim": args.dim, "batch": args.batch, "k": args.k, "dtype": "f16"},
           "total_blocks": (args.rows + 31) // 32, "rows": {}}
    for row in ([args.only] if args.only else ROWS):
        allowed, frac = masks_for(row, args.rows, torch, dev)
        kw = {} if allowed is None else {"allowed": allowed}
        # correctness once: every returned score has the bits of the unfiltered scan's score of that row
        D, I = idx.search(qs[0], args.k, **kw)
        if allowed is not None:
            if S0 is None:
                S0 = idx.scores(qs[0][:4])
            for q in range(4):
                ok = I[q] >= 0
                assert torch.equal(S0[q, I[q][ok]].view(torch.int32), D[q][ok].view(torch.int32)), row
        info = idx.last_filter_info() if allowed is not None else None
        path = idx.last_search_info()["path"]
        for _ in range(3):
            idx.search(qs[1], args.k, **kw)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for s in range(args.steps):
            idx.search(qs[s % 4], args.k, **kw)
        torch.cuda.synchronize()
        sync_ms = (time.perf_counter() - t) * 1e3 / args.steps
        idx.finish()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for s in range(args.steps):
            idx.search(qs[s % 4], args.k, async_=True, **kw)
        redone = idx.finish()
        torch.cuda.synchronize()
        async_ms = (time.perf_counter() - t) * 1e3 / args.steps
        rec = {"allowed_fraction": frac, "ms_per_batch_sync": round(sync_ms, 4), "ms_per_batch_async": round(async_ms, 4),
               "path": path, "async_redone": len(redone)}
        if info is not None:
            rec.update(live_blocks=info["live_blocks"], live_fraction=round(info["live_blocks"] / out["total_blocks"], 5),
                       live_bytes=info["live_blocks"] * 32 * args.dim * 2)
        out["rows"][row] = rec
        print(row, json.dumps(rec), flush=True)
    idx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
