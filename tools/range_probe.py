"""Range search on the bench shape (10 M x 768 f16, B = 64, one GPU): ms per call of FlatIPIndex.range_search beside
FlatIPIndex.search(q, 1000) (synchronous) in the same run, for the three rows of DESIGN.md 4.13:

  selective     radius = each query's 1000th best score (about 1000 results per query): the filter path
  tombstones    the same after 1 % of the rows were removed: the masked filter path
  unselective   radius at rank 100 000: the filter scan overflows, the pass is redone on the dense path

    python tools/range_probe.py [--rows N] [--steps S] [--parent-lib libtristage_of_the_parent.so] [--out FILE]

Every row is checked once before it is timed: the sorted range result starts with the top-k result bit for bit, and
no removed id comes back.  With --parent-lib the time of search(q, 1000) is also taken in child processes that load
this tree's library and the parent commit's (TRISTAGE_LIB) in turn, twice each: the alternating run."""
import argparse
import json
import os
import subprocess
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


def timed(torch, fn, steps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def search_ms(torch, idx, q, args):
    return round(timed(torch, lambda: idx.search(q, args.k), args.steps), 4)


def call_and_fetch_ms(torch, idx, q, radius, steps):
    """The two library calls of FlatIPIndex.range_search, each timed alone: ts_index_range_search (query image, scan,
    the host's read of the counts, sort or count / prefix / fill; synchronous) and ts_index_range_fetch to device memory."""
    import ctypes
    from tristage_rag_amd import _lib
    B = int(q.shape[0])
    rad = np.ascontiguousarray(radius.float().cpu().numpy())
    lims = np.zeros(B + 1, dtype=np.int64)
    st = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream)) if torch.cuda.current_stream().cuda_stream else None

    def call():
        _lib.check(idx._lib.ts_index_range_search(idx._h, ctypes.c_void_p(q.data_ptr()), B, _lib.TS_F16,
                                                  rad.ctypes.data_as(ctypes.c_void_p), None, 0, 0, None, 0,
                                                  lims.ctypes.data_as(ctypes.c_void_p), 0, st))
    call_ms = timed(torch, call, steps, warm=2)
    total = int(lims[B])
    D = torch.empty(total, dtype=torch.float32, device=q.device)
    I = torch.empty(total, dtype=torch.int64, device=q.device)
    fetch_ms = timed(torch, lambda: _lib.check(idx._lib.ts_index_range_fetch(
        idx._h, ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(I.data_ptr()), total, 0, st)), steps, warm=2)
    return round(call_ms, 4), round(fetch_ms, 4)


def range_row(torch, idx, q, radius, args, steps, check_k=None, removed=None):
    lims, D, I = idx.range_search(q, radius, sort=check_k is not None)
    info = idx.last_range_info()
    lims_h = lims.cpu().numpy()
    if check_k is not None:   # the sorted segments start with the top-k result
        Dk, Ik = idx.search(q, check_k)
        for b in range(q.shape[0]):
            s = int(lims_h[b])
            assert torch.equal(D[s:s + check_k].view(torch.int32), Dk[b].view(torch.int32)) and torch.equal(I[s:s + check_k], Ik[b])
    if removed is not None:
        assert not np.isin(I.cpu().numpy(), removed).any()
    total = int(lims_h[-1])
    ms = timed(torch, lambda: idx.range_search(q, radius), steps, warm=2)
    call_ms, fetch_ms = call_and_fetch_ms(torch, idx, q, radius, steps)
    return {"library_call_ms": call_ms, "fetch_ms": fetch_ms,
            "results": total, "results_per_query_min": int(np.diff(lims_h).min()), "results_per_query_max": int(np.diff(lims_h).max()),
            "result_bytes": total * 12, "ms_per_call": round(ms, 4), **info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--wide-rank", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--search-only", action="store_true", help="print the time of search(q, k) and exit (the alternating run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    n = args.rows
    if args.search_only:
        # (the parent's library lacks the entry points this tree added: they leave this child's binding table)
        import ctypes
        from tristage_rag_amd import _lib
        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in [s for s in _lib.SIGNATURES if not hasattr(probe, s)]:
            del _lib.SIGNATURES[name]
    q = gen_rows(torch, args.batch, args.dim, 99, dev)
    idx = build(torch, args, dev)
    if args.search_only:
        print(json.dumps({"search_ms": search_ms(torch, idx, q, args)}), flush=True)
        idx.close()
        return
    out = {"shape": {"rows": n, "dim": args.dim, "batch": args.batch, "k": args.k, "dtype": "f16"}, "rows": {}}

    def record(name, rec):
        rec["ratio_to_search"] = round(rec["ms_per_call"] / rec["search_ms_same_run"], 3)
        out["rows"][name] = rec
        print(name, json.dumps(rec), flush=True)

    # 1: selective
    D, _ = idx.search(q, args.k)
    rec = range_row(torch, idx, q, D[:, args.k - 1].clone(), args, args.steps, check_k=args.k)
    rec["search_ms_same_run"] = search_ms(torch, idx, q, args)
    record("selective", rec)
    # 3: unselective (before the removal, on the same index): radius at rank --wide-rank from the dense scores
    rad = []
    for b0 in range(0, args.batch, 8):
        S = idx.scores(q[b0:b0 + 8])
        rad.append(torch.topk(S, args.wide_rank, dim=1).values[:, -1].clone())
        del S
    rec = range_row(torch, idx, q, torch.cat(rad), args, max(2, args.steps // 5))
    rec["search_ms_same_run"] = out["rows"]["selective"]["search_ms_same_run"]
    rec["dense_scores_bytes_per_chunk"] = args.batch * (1 << 20) * 4
    record("unselective", rec)
    # 2: 1 % of the rows removed
    removed = np.flatnonzero(np.random.default_rng(7).random(n) < 0.01)
    assert idx.remove_ids(removed) == removed.size
    D, _ = idx.search(q, args.k)
    rec = range_row(torch, idx, q, D[:, args.k - 1].clone(), args, args.steps, check_k=args.k, removed=removed)
    rec["search_ms_same_run"] = search_ms(torch, idx, q, args)
    rec["removed"] = int(removed.size)
    record("tombstones_1pct", rec)
    idx.close()
    del idx
    torch.cuda.empty_cache()
    if args.parent_lib:
        # the alternating run: fresh child processes, this tree's library and the parent's in turn
        alt = {"this": [], "parent": []}
        base = [sys.executable, os.path.abspath(__file__), "--search-only", "--rows", str(n), "--dim", str(args.dim),
                "--batch", str(args.batch), "--k", str(args.k), "--steps", str(args.steps)]
        for _ in range(2):
            for who in ("parent", "this"):
                env = dict(os.environ)
                if who == "parent":
                    env["TRISTAGE_LIB"] = os.path.abspath(args.parent_lib)
                else:
                    env.pop("TRISTAGE_LIB", None)
                r = subprocess.run(base, env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(f"the {who} run failed ({r.returncode}): {r.stderr[-2000:]}")
                alt[who].append(json.loads(r.stdout.strip().splitlines()[-1])["search_ms"])
                print("alternating", who, alt[who][-1], flush=True)
        out["search_ms_alternating"] = alt
        parent = float(np.mean(alt["parent"]))
        for rec in out["rows"].values():
            rec["ratio_to_parent_search"] = round(rec["ms_per_call"] / parent, 3)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
