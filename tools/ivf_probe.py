"""IVF-Flat against the exact flat scan on one GPU: clustered synthetic corpus, per (nlist, nprobe) the train time, add
rate, B = 1 latency, B = 64 throughput at k = 1000, recall@100 / @1000 against exact and the live blocks per pass.
Writes one JSON document.

  python tools/ivf_probe.py --rows 10000000 --dim 768 --out profiles/ivf_probe.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tristage_rag_amd.index import FlatIPIndex, IVFFlatIndex  # noqa: E402


def clustered(n, d, centers, gen, spread=0.5, chunk=1 << 20):
    """Gaussian mixture on the sphere, f16, generated on the device in chunks."""
    c = torch.randn((centers, d), generator=gen, device="cuda")
    c /= c.norm(dim=1, keepdim=True)
    out = torch.empty((n, d), dtype=torch.float16, device="cuda")
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        lab = torch.randint(0, centers, (r1 - r0,), generator=gen, device="cuda")
        x = c[lab] + spread * torch.randn((r1 - r0, d), generator=gen, device="cuda") / d ** 0.5 * 4
        out[r0:r1] = (x / x.norm(dim=1, keepdim=True)).half()
    return out


def timed(fn, reps):
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def recall(I, I0, k):
    I, I0 = I[:, :k].cpu(), I0[:, :k].cpu()
    return float(sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(I, I0)) / (k * I.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--centers", type=int, default=2000)
    ap.add_argument("--configs", default="100:10,1024:16,4096:32,16384:64")
    ap.add_argument("--niter", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/ivf_probe.json")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = clustered(a.rows, a.dim, a.centers, gen)
    q = clustered(64, a.dim, a.centers, torch.Generator(device="cuda").manual_seed(1))
    flat = FlatIPIndex(a.dim, dtype="f16")
    flat.add(x)
    D0, I0 = flat.search(q, 1000)
    res = {"rows": a.rows, "dim": a.dim, "dtype": "f16", "centers": a.centers, "niter": a.niter,
           "corpus_bytes": a.rows * a.dim * 2,
           "flat": {"b1_ms": 1e3 * timed(lambda: flat.search(q[:1], 100), a.reps),
                    "b64_k1000_ms": 1e3 * timed(lambda: flat.search(q, 1000), a.reps)},
           "configs": []}
    del flat
    torch.cuda.empty_cache()
    block_bytes = 32 * ((a.dim + 127) // 128 * 128) * 2
    for spec in a.configs.split(","):
        nlist, nprobe = (int(v) for v in spec.split(":"))
        ivf = IVFFlatIndex(a.dim, nlist, dtype="f16", nprobe=nprobe)
        ivf.niter = a.niter
        train_s = timed(lambda: ivf.train(x), 1)
        add_s = timed(lambda: ivf.add(x), 1)
        D, I = ivf.search(q, 1000)
        live64 = ivf.last_search_info()["live_blocks"]
        ivf.search(q[:1], 100)
        live1 = ivf.last_search_info()["live_blocks"]
        sizes = ivf.list_sizes()
        probed = ivf.probe(q)[1].cpu().numpy()
        b1 = timed(lambda: ivf.search(q[:1], 100), a.reps)
        b64 = timed(lambda: ivf.search(q, 1000), a.reps)
        info = ivf.last_search_info()
        row = {"nlist": nlist, "nprobe": nprobe, "train_s": train_s, "add_rows_per_s": a.rows / add_s,
               "b1_k100_ms": 1e3 * b1, "b64_k1000_ms": 1e3 * b64, "b64_qps": 64 / b64,
               "recall_at_100": recall(I, I0, 100), "recall_at_1000": recall(I, I0, 1000),
               "probed_rows_per_query_mean": float(sizes[probed].sum(axis=1).mean()),
               "live_blocks_b1": live1, "live_blocks_b64": live64,
               "live_fraction_b64": live64 * 32 / a.rows, "live_bytes_b64": live64 * block_bytes,
               "redone_passes_b64": info["redone"], "list_size_min_max": [int(sizes.min()), int(sizes.max())]}
        res["configs"].append(row)
        print(json.dumps(row), flush=True)
        del ivf
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res["flat"]))


if __name__ == "__main__":
    main()
