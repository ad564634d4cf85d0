"""Best passage per hit timed on one GPU with HIP events: a bf16 token store of documents with 64 to
192 token rows, H = 768, 64 queries of 32 tokens, window 32; per candidate count (20, 100, 1000 per query) the batch call
alone (maxsim_passages_indexed_batch), the same selection written in torch ops in the same process (what a caller
would write without it: gather the candidates' rows into a padded tensor, two norms, a matmul, unfold, amax, sum,
argmax; fp32 so that the products are the kernel's) — once for the whole batch with one padded bmm, where the padded
fp32 tensor is at most --batched-max-pairs pairs (3.8 GB at 6400), and once query by query, which at few candidates
measures launches more than the selection —, the plain maxsim_indexed_batch on the same candidates, and whether the
torch baseline's starts equal the kernel's.  The ratio is taken against the faster baseline.  One JSON document.

  python tools/passage_probe.py --out profiles/passage_probe.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, rounds):
    """Milliseconds per call from HIP events, ``rounds`` times after a warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


def torch_passages(torch, q, q_off, store, starts, lens, c_off, w, lmax):
    """The baseline -> (start int64 [n], score f32 [n]).  Every candidate here has at least w rows."""
    F = torch.nn.functional
    ar = torch.arange(lmax, device=store.device)
    out_p, out_s = [], []
    for j in range(len(q_off) - 1):
        qn = F.normalize(q[q_off[j]: q_off[j + 1]].float(), dim=1, eps=1e-12)                       # [Lq, H]
        s, l = starts[c_off[j]: c_off[j + 1]], lens[c_off[j]: c_off[j + 1]].to(torch.int64)
        valid = ar[None, :] < l[:, None]                                                            # [C, lmax]
        rows = (s[:, None] + torch.where(valid, ar[None, :], torch.zeros_like(ar)[None, :]))
        d = F.normalize(store[rows].float(), dim=2, eps=1e-12)                                      # [C, lmax, H]
        c = torch.matmul(d, qn.t()).masked_fill(~valid[:, :, None], float("-inf"))                  # [C, lmax, Lq]
        S = c.unfold(1, w, 1).amax(dim=3).sum(dim=2)                                                # [C, lmax - w + 1]
        S = S.masked_fill(ar[None, : lmax - w + 1] > (l - w)[:, None], float("-inf"))
        best = S.max(dim=1)
        # (max() gives AN index of the maximum; the lowest one, as the kernel's rule wants, by a second pass)
        first = (S == best.values[:, None]).to(torch.int64).argmax(dim=1)
        out_p.append(first)
        out_s.append(best.values / (q_off[j + 1] - q_off[j]))
    return torch.cat(out_p), torch.cat(out_s)


def torch_passages_batched(torch, q, lq, nq, store, starts, lens, per_query, w, lmax):
    """The baseline over the whole batch at once (every query has lq tokens and per_query candidates)."""
    F = torch.nn.functional
    ar = torch.arange(lmax, device=store.device)
    qn = F.normalize(q.float(), dim=1, eps=1e-12).view(nq, lq, -1)                                  # [nq, Lq, H]
    l = lens.to(torch.int64)
    valid = ar[None, :] < l[:, None]                                                                # [P, lmax]
    rows = starts[:, None] + torch.where(valid, ar[None, :], torch.zeros_like(ar)[None, :])
    d = F.normalize(store[rows].float(), dim=2, eps=1e-12).view(nq, per_query * lmax, -1)           # [nq, C lmax, H]
    c = torch.bmm(d, qn.transpose(1, 2)).view(nq * per_query, lmax, lq)                             # [P, lmax, Lq]
    c = c.masked_fill(~valid[:, :, None], float("-inf"))
    S = c.unfold(1, w, 1).amax(dim=3).sum(dim=2)
    S = S.masked_fill(ar[None, : lmax - w + 1] > (l - w)[:, None], float("-inf"))
    best = S.max(dim=1)
    first = (S == best.values[:, None]).to(torch.int64).argmax(dim=1)
    return first, best.values / lq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--lq", type=int, default=32)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--cands", type=int, nargs="+", default=[20, 100, 1000])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batched-max-pairs", type=int, default=6400)
    ap.add_argument("--out", default="profiles/passage_probe.json")
    a = ap.parse_args()
    import torch
    from tristage_rag_amd.index import maxsim_indexed_batch, maxsim_passages_indexed_batch
    g = torch.Generator(device="cuda").manual_seed(1)
    lens_all = torch.randint(64, 193, (a.docs,), generator=g, device="cuda", dtype=torch.int64)
    starts_all = torch.cumsum(lens_all, 0) - lens_all
    rows = int(lens_all.sum().item())
    store = torch.empty((rows, a.dim), dtype=torch.bfloat16, device="cuda")
    for r0 in range(0, rows, 1 << 18):
        x = torch.randn((min(rows, r0 + (1 << 18)) - r0, a.dim), generator=g, device="cuda")
        store[r0: r0 + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).bfloat16()
    x = torch.randn((a.queries * a.lq, a.dim), generator=g, device="cuda")
    q = (x / x.norm(dim=1, keepdim=True)).bfloat16()
    q_off = [j * a.lq for j in range(a.queries + 1)]
    doc = {"docs": a.docs, "store_rows": rows, "dim": a.dim, "queries": a.queries, "lq": a.lq, "window": a.window,
           "store_dtype": "bf16", "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": []}
    for C in a.cands:
        pick = torch.randint(0, a.docs, (a.queries * C,), generator=g, device="cuda")
        starts, lens = starts_all[pick].contiguous(), lens_all[pick].to(torch.int32).contiguous()
        c_off = [j * C for j in range(a.queries + 1)]
        e = {"candidates_per_query": C, "pairs": a.queries * C,
             "candidate_bytes": int(lens.sum().item()) * a.dim * 2}
        call = lambda: maxsim_passages_indexed_batch(q, q_off, store, starts, lens, c_off, a.window, max_len=192)
        e["passages_ms"] = timed(torch, call, a.rounds)
        e["passages_align_ms"] = timed(torch, lambda: maxsim_passages_indexed_batch(
            q, q_off, store, starts, lens, c_off, a.window, align=True, max_len=192), a.rounds)
        e["maxsim_ms"] = timed(torch, lambda: maxsim_indexed_batch(q, q_off, store, starts, lens, c_off), a.rounds)
        base = lambda: torch_passages(torch, q, q_off, store, starts, lens, c_off, a.window, 192)
        e["torch_loop_ms"] = timed(torch, base, a.rounds)
        got, ref = call(), base()
        same = got[0].to(torch.int64) == ref[0]
        e["torch_starts_equal"] = bool(same.all().item())
        e["torch_starts_differing"] = int((~same).sum().item())
        e["max_score_difference"] = float((got[2] - ref[1]).abs().max().item())
        fastest = e["torch_loop_ms"]["median"]
        if a.queries * C <= a.batched_max_pairs:
            bat = lambda: torch_passages_batched(torch, q, a.lq, a.queries, store, starts, lens, C, a.window, 192)
            e["torch_batched_ms"] = timed(torch, bat, a.rounds)
            e["torch_batched_starts_equal"] = bool((bat()[0] == got[0].to(torch.int64)).all().item())
            fastest = min(fastest, e["torch_batched_ms"]["median"])
        e["torch_over_kernel"] = fastest / e["passages_ms"]["median"]
        e["kernel_over_maxsim"] = e["passages_ms"]["median"] / e["maxsim_ms"]["median"]
        e["kernel_GBps"] = e["candidate_bytes"] / e["passages_ms"]["median"] / 1e6
        doc["rows"].append(e)
        print(json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in e.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
