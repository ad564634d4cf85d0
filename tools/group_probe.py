"""Grouped search timed on one GPU with HIP events: per group table (1, 4 and 64 rows per group) the
plain search at the fetch grouped search starts with, search_grouped and its rounds; per list length the collapse alone
(group_topk) and the same collapse written in torch ops (what a user would write without it: a stable sort by group, a
segmented cummax, two prefix sums, scatters), with whether the two agree.  One JSON document.

  python tools/group_probe.py --rows 1000000 --dim 768 --out profiles/group_probe.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gen_rows(torch, n, d, seed, chunk=1 << 20):
    """bench.py's generator (unit-norm Gaussian rows), f16, in chunks."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((n, d), dtype=torch.float16, device="cuda")
    for r0 in range(0, n, chunk):
        x = torch.randn((min(n, r0 + chunk) - r0, d), generator=g, device="cuda", dtype=torch.float32)
        out[r0:r0 + x.shape[0]] = (x / (x.norm(dim=1, keepdim=True) + 1e-8)).half()
    return out


def torch_group_topk(torch, D, I, tab, k, gs, id_base=0):
    """The baseline: the collapse of group_topk in torch ops -> (D, I, G) [B, k * gs]."""
    B, C = I.shape
    dev = I.device
    pos = torch.arange(C, device=dev).expand(B, C)
    row = I - id_base
    valid = (I != -1) & (row >= 0) & (row < tab.shape[0])
    g = tab[row.clamp(0, max(tab.shape[0] - 1, 0))].to(torch.int64)
    key = torch.where(g >= 0, g, (1 << 32) + pos)                    # an entry without a group: a key of its own
    key = torch.where(valid, key, torch.full_like(key, 1 << 40))     # invalid entries sort last
    skey, perm = torch.sort(key, dim=1, stable=True)                 # equal keys keep ascending positions
    head = torch.ones_like(skey, dtype=torch.bool)
    head[:, 1:] = skey[:, 1:] != skey[:, :-1]
    start = torch.cummax(torch.where(head, pos, torch.zeros_like(pos)), dim=1).values
    occ_s = pos - start
    first_s = torch.gather(perm, 1, start)
    svalid = skey < (1 << 40)
    occ = torch.empty_like(pos).scatter_(1, perm, occ_s)
    first = torch.empty_like(pos).scatter_(1, perm, first_s)
    isfirst = torch.zeros((B, C), dtype=torch.int64, device=dev).scatter_(1, perm, (head & svalid).to(torch.int64))
    before = torch.cumsum(isfirst, dim=1) - isfirst                  # groups that start before position p
    rank = torch.gather(before, 1, first)
    keep = valid & (rank < k) & (occ < gs)
    slot = torch.cumsum(keep.to(torch.int64), dim=1) - 1
    W = k * gs
    slot = torch.where(keep, slot, torch.full_like(slot, W))         # dropped entries go to a column that is cut off
    oD = torch.full((B, W + 1), -3.4028234663852886e38, dtype=torch.float32, device=dev).scatter_(1, slot, D)
    oI = torch.full((B, W + 1), -1, dtype=torch.int64, device=dev).scatter_(1, slot, I)
    oG = torch.full((B, W + 1), -1, dtype=torch.int64, device=dev).scatter_(1, slot, g.clamp(min=-1))
    return oD[:, :W], oI[:, :W], oG[:, :W].to(torch.int32)


def timed(torch, fn, rounds, inner=1):
    """Milliseconds per call from HIP events around ``inner`` back-to-back calls, ``rounds`` times after a warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "inner": inner, "runs": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--group-size", type=int, default=1)
    ap.add_argument("--rows-per-group", type=int, nargs="+", default=[1, 4, 64])
    ap.add_argument("--lists", type=int, nargs="+", default=[128, 1024, 16384])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default="profiles/group_probe.json")
    a = ap.parse_args()
    import torch
    from tristage_rag_amd.index import FlatIPIndex, group_default_fetch_k, group_topk
    x = gen_rows(torch, a.rows, a.dim, 1)
    q = gen_rows(torch, a.batch, a.dim, 2)
    idx = FlatIPIndex(a.dim, dtype="f16")
    idx.reserve(a.rows)
    idx.add(x)
    k, gs = a.k, a.group_size
    doc = {"rows": a.rows, "dim": a.dim, "batch": a.batch, "k": k, "group_size": gs, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "tables": [], "lists": []}
    fetch0 = group_default_fetch_k(k, gs)
    doc["search_ms"] = {str(f): timed(torch, lambda f=f: idx.search(q, f), a.rounds) for f in sorted({fetch0, *a.lists})}
    for rpg in a.rows_per_group:
        tab = (torch.arange(a.rows, device="cuda") // rpg).to(torch.int32)
        r = {"rows_per_group": rpg, "first_fetch": fetch0}
        r["search_grouped_ms"] = timed(torch, lambda: idx.search_grouped(q, k, tab, group_size=gs), a.rounds)
        info = idx.last_group_info()
        r["rounds_taken"], r["fetched"] = info["rounds"], info["fetched"]
        r["complete"] = bool(info["complete"].all())
        r["grouped_over_search"] = r["search_grouped_ms"]["median"] / doc["search_ms"][str(fetch0)]["median"]
        doc["tables"].append(r)
        print(json.dumps({k_: (v["median"] if isinstance(v, dict) else v) for k_, v in r.items()}), flush=True)
        for C in a.lists:
            D, I = idx.search(q, C)
            e = {"rows_per_group": rpg, "C": C}
            e["group_topk_ms"] = timed(torch, lambda: group_topk(I, D, tab, k, gs), a.rounds, inner=20)
            e["torch_ms"] = timed(torch, lambda: torch_group_topk(torch, D, I, tab, k, gs), a.rounds)
            got = group_topk(I, D, tab, k, gs)
            ref = torch_group_topk(torch, D, I, tab, k, gs)
            e["equals_torch"] = bool(all(torch.equal(g_, r_) for g_, r_ in zip(got[:3], ref)))
            e["torch_over_kernel"] = e["torch_ms"]["median"] / e["group_topk_ms"]["median"]
            doc["lists"].append(e)
            print(json.dumps({k_: (v["median"] if isinstance(v, dict) else v) for k_, v in e.items()}), flush=True)
    idx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
