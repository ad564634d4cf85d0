"""IVFFlatIndex.compact() on one GPU: its time after random removals and after updates, next to
FlatIPIndex.compact() on the same rows with the same ids removed in the same run, the split between device and host
time, the corpus bytes it reads and writes, and live blocks / ms per search before and after.

  python tools/ivf_compact_probe.py --rows 10000000 --dim 768 --out profiles/ivf_compact_probe.json

Every compaction is checked: the id map against the removed set (and against the flat index's map), sampled rows, and
a search against the index before it.  The device time of one further compaction per case is the sum of the kernels and
copies torch.profiler records inside the call (null where the profiler records none); host time is the rest of that
call's wall time."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivf_probe import clustered, timed  # noqa: E402
from tristage_rag_amd.index import FlatIPIndex, IVFFlatIndex  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def device_split(fn):
    """-> (result, wall ms, device ms or None, {kernel name: ms} of the compaction kernels)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            out, ms = wall_ms(fn)
        dev_us, mine = 0.0, {}
        for ka in prof.key_averages():
            us = getattr(ka, "self_device_time_total", None)
            if us is None:
                us = getattr(ka, "self_cuda_time_total", 0.0)
            dev_us += us
            if "ivfc_" in ka.key or "compact_" in ka.key or "Memcpy" in ka.key or "Memset" in ka.key:
                mine[ka.key[:60]] = round(mine.get(ka.key[:60], 0.0) + us / 1e3, 3)
        return out, ms, (round(dev_us / 1e3, 3) if dev_us > 0 else None), mine
    except Exception as e:   # (a profiler that cannot attach: the wall time alone)
        print("profiler unavailable:", repr(e), flush=True)
        out, ms = wall_ms(fn)
        return out, ms, None, {}


def blocks_needed(ivf):
    return int(((ivf.list_sizes() + 31) // 32).sum())


def search_state(ivf, q, k, reps):
    D, I = ivf.search(q, k)
    info = ivf.last_search_info()
    ms = 1e3 * timed(lambda: ivf.search(q, k), reps)
    return (D, I), {"live_blocks": info["live_blocks"], "b64_ms": round(ms, 4), "filter_passes": info["filter_passes"],
                    "redone": info["redone"]}


def corpus_bytes(ivf, dim):
    dpad = (dim + 127) // 128 * 128
    return {"read": int(ivf.nlive) * dpad * 2, "written": blocks_needed(ivf) * 32 * dpad * 2}


def check_rows(ivf, before_rows, sample, old2new):
    got = np.concatenate([ivf.reconstruct_n(int(old2new[r]), 1) for r in sample])
    assert np.array_equal(got, before_rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--centers", type=int, default=2000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--niter", type=int, default=25)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/ivf_compact_probe.json")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = clustered(a.rows, a.dim, a.centers, gen)
    q = clustered(64, a.dim, a.centers, torch.Generator(device="cuda").manual_seed(1))
    rng = np.random.default_rng(7)
    ivf = IVFFlatIndex(a.dim, a.nlist, dtype="f16", nprobe=a.nprobe)
    ivf.niter = a.niter
    ivf.train(x)
    ivf.add(x)
    flat = FlatIPIndex(a.dim, dtype="f16")
    flat.add(x)
    res = {"shape": {"rows": a.rows, "dim": a.dim, "dtype": "f16", "nlist": a.nlist, "nprobe": a.nprobe, "batch": 64,
                     "k": a.k}, "removal_1pct": {"runs": []}, "update_10pct": {"runs": []}}
    _, res["fresh"] = search_state(ivf, q, a.k, 5)
    print("fresh", json.dumps(res["fresh"]), flush=True)

    # ---- 1 % random removals, the same ids from both indexes; reps timed runs and one under the profiler
    for rep in range(a.reps + 1):
        n = ivf.ntotal
        assert flat.ntotal == n
        ids = np.sort(rng.choice(n, n // 100, replace=False))
        assert ivf.remove_ids(ids) == ids.size == flat.remove_ids(ids)
        live = np.ones(n, bool)
        live[ids] = False
        sample = np.sort(rng.choice(np.flatnonzero(live), 500, replace=False))
        rows = np.concatenate([ivf.reconstruct_n(int(r), 1) for r in sample])
        pre, before = search_state(ivf, q, a.k, 5)
        run = {"removed": int(ids.size), "ntotal_before": int(n), "before": before, "bytes": None}
        if rep < a.reps:
            old2new, run["ivf_compact_ms"] = wall_ms(ivf.compact)
        else:
            old2new, run["ivf_compact_ms"], run["device_ms"], run["device_parts_ms"] = device_split(ivf.compact)
            run["host_ms"] = None if run["device_ms"] is None else round(run["ivf_compact_ms"] - run["device_ms"], 3)
        flat_map, run["flat_compact_ms"] = wall_ms(flat.compact)
        run["bytes"] = corpus_bytes(ivf, a.dim)
        assert np.array_equal(old2new, flat_map)
        assert (old2new[~live] == -1).all() and np.array_equal(old2new[live], np.arange(n - ids.size))
        assert ivf.ntotal == ivf.nlive == n - ids.size
        check_rows(ivf, rows, sample, old2new)
        post, run["after"] = search_state(ivf, q, a.k, 5)
        pi = pre[1].cpu().numpy()
        assert np.array_equal(post[1].cpu().numpy(), np.where(pi >= 0, old2new[np.maximum(pi, 0)], -1))
        assert torch.equal(post[0].view(torch.int32), pre[0].view(torch.int32))
        assert run["after"]["live_blocks"] <= blocks_needed(ivf)
        run["blocks_needed_after"] = blocks_needed(ivf)
        for key in ("ivf_compact_ms", "flat_compact_ms"):
            run[key] = round(run[key], 3)
        (res["removal_1pct"]["runs"] if rep < a.reps else res["removal_1pct"].setdefault("profiled", [])).append(run)
        print("removal", rep, json.dumps(run), flush=True)
    flat.close()
    del flat

    # ---- 10 % of the rows updated with the content of other rows (rows change lists and leave holes)
    for rep in range(a.reps + 1):
        n = ivf.ntotal
        ids = np.sort(rng.choice(n, n // 10, replace=False))
        src = torch.from_numpy(rng.integers(0, a.rows, ids.size)).cuda()
        ivf.update_rows(ids, x[src])
        del src
        sample = np.sort(rng.choice(n, 500, replace=False))
        rows = np.concatenate([ivf.reconstruct_n(int(r), 1) for r in sample])
        pre, before = search_state(ivf, q, a.k, 5)
        run = {"updated": int(ids.size), "ntotal": int(n), "before": before}
        if rep < a.reps:
            old2new, run["ivf_compact_ms"] = wall_ms(ivf.compact)
        else:
            old2new, run["ivf_compact_ms"], run["device_ms"], run["device_parts_ms"] = device_split(ivf.compact)
            run["host_ms"] = None if run["device_ms"] is None else round(run["ivf_compact_ms"] - run["device_ms"], 3)
        run["ivf_compact_ms"] = round(run["ivf_compact_ms"], 3)
        run["bytes"] = corpus_bytes(ivf, a.dim)
        assert np.array_equal(old2new, np.arange(n)) and ivf.ntotal == ivf.nlive == n
        check_rows(ivf, rows, sample, old2new)
        post, run["after"] = search_state(ivf, q, a.k, 5)
        assert torch.equal(post[1], pre[1]) and torch.equal(post[0].view(torch.int32), pre[0].view(torch.int32))
        run["blocks_needed_after"] = blocks_needed(ivf)
        (res["update_10pct"]["runs"] if rep < a.reps else res["update_10pct"].setdefault("profiled", [])).append(run)
        print("update", rep, json.dumps(run), flush=True)

    for case in ("removal_1pct", "update_10pct"):
        ms = [r["ivf_compact_ms"] for r in res[case]["runs"]]
        res[case]["ivf_compact_ms_best"], res[case]["ivf_compact_ms_avg"] = min(ms), round(sum(ms) / len(ms), 3)
    fm = [r["flat_compact_ms"] for r in res["removal_1pct"]["runs"]]
    res["removal_1pct"]["flat_compact_ms_best"], res["removal_1pct"]["flat_compact_ms_avg"] = min(fm), round(sum(fm) / len(fm), 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "shape"})[:400], flush=True)


if __name__ == "__main__":
    main()
