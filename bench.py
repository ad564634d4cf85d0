#!/usr/bin/env python3
"""bench.py — stage-1 brute-force top-k throughput on MI355X (the hot path of
BASELINE.json's north_star; workload = configs[3]: synthetic 10M x 768 fp16
corpus, batch-64 queries, top-1000, row-sharded over N GPUs with one RCCL
all-gather + merge per batch).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A "step" = one batch of 64 queries searched against the whole corpus: local
shard scan + exact top-k on every rank, all-gather of the partial lists, merge.
Corpus and queries are resident in HBM before the timed region.  The total
corpus is fixed as N grows (strong scaling: the metric is quoted "@10Mx768
corpus, 1/2/4/8 GPU").

One JSON line on rank 0.  A plain run does what the headline needs and no more:
set up, warm up, time the K steps, dump the outputs if asked, print the line.
Besides the driver's contract the line carries
  roofline      the fused scan+filter kernel: algorithmic bytes per launch
                (shard rows x padded dim x 2 B, the corpus read once) / its mean
                duration measured with HIP events on the launch stream, inside
                the timed steps; `traffic` is the number kept in
                profiles/traffic.json for the shape

--full adds everything that takes runs of its own (and the --no-* switches and
--traffic choose among those):
  roofline      `traffic` measured live (two rocprofv3 --pmc child runs) and
                `measured_read_peak` (a read-only pass over the corpus)
  secondary     the search fed by a bi-encoder forward, and the three-stage
                pipeline on the configs[2] shape (N=1 only)
  cpu_baseline  the same search on the host cores (oracle.ip_topk_blas: blocked
                SGEMM + partial sort, what faiss-cpu IndexFlatIP does) on a
                bounded row sample, scaled to the full corpus.  N=1 only.
Without --full, `secondary` and `cpu_baseline` are null.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec (6.29 TB/s measured copy ceiling)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10_000_000, help="total corpus rows")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32"])
    ap.add_argument("--full", action="store_true",
                    help="also everything beside the headline that takes runs of its own: cpu_baseline, the secondary legs "
                         "(encoder + search, three-stage pipeline), the read probe and live PMC traffic of the roofline.  "
                         "Off by default: a plain run sets up, warms up, times the steps and prints its line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--sync", action="store_true",
                    help="wait for every batch before issuing the next (default: batches are enqueued "
                         "back to back and completed + verified by finish() inside the timed region)")
    ap.add_argument("--pipeline", choices=["auto", "on", "off"], default="auto",
                    help="overlap the small kernels of neighbouring batches with the scan (internal streams). "
                         "auto: on for N>1 (short per-rank scans, where the fixed part matters: +10 %% at "
                         "1.25 M rows per rank), off for N=1 (no gain at 10 M rows and the overlapped scan "
                         "runs 2-3 %% slower)")
    ap.add_argument("--no-profile", action="store_true", help="no HIP-event timing of the scan kernel")
    ap.add_argument("--force-exchange", action="store_true",
                    help="diagnostic: with one rank, still run the RCCL all-gather + merge every step")
    ap.add_argument("--submit-stream", choices=["auto", "null", "side"], default="auto",
                    help="stream the searches are submitted from.  auto: a non-default stream when pipelining "
                         "(the NULL stream synchronises implicitly with every blocking stream of the process: "
                         "0.332 -> 0.324 ms per batch at 1.25 M rows per rank), the NULL stream otherwise")
    ap.add_argument("--cpu-sample-rows", type=int, default=400_000)
    ap.add_argument("--one-launch", action="store_true",
                    help="A/B: the one-launch scan (query image + thresholds + scan+filter in one kernel) also where the "
                         "five-launch path is the default (pipelined submission, corpora above 4 M rows)")
    ap.add_argument("--classic", action="store_true",
                    help="A/B: the five-launch filter path (query prep, sample scan, thresholds, scan+filter, select) "
                         "instead of the one-launch scan")
    ap.add_argument("--step-events", choices=["auto", "on", "off"], default="auto",
                    help="one HIP event per timed step on the submitting stream -> ms_per_step_min/max "
                         "(a few microseconds each in-stream).  auto: on for N=1, off for N>1")
    ap.add_argument("--dump-steps", action="store_true",
                    help="diagnostic: the per-step event intervals (ms) and the steps at which the collective finish() ran, "
                         "as config.step_ms / config.finish_at")
    ap.add_argument("--no-encode-leg", action="store_true",
                    help="with --full: skip the secondary leg (bi-encoder forward of the 64 query texts + the same search)")
    ap.add_argument("--no-pipeline-leg", action="store_true",
                    help="with --full: skip the secondary legs that run the full three-stage pipeline (configs[2] shape, search_many of 64 "
                         "queries, BM25 off and on); N=1 only")
    ap.add_argument("--no-read-probe", action="store_true",
                    help="with --full: skip the read-only pass over the corpus that gives roofline.measured_read_peak")
    ap.add_argument("--traffic", choices=["auto", "live", "static", "off"], default="auto",
                    help="roofline.traffic: live = two rocprofv3 --pmc child runs of this script (FETCH_SIZE, WRITE_SIZE; "
                         "about half a minute each), static = the number kept in profiles/traffic.json for this shape, "
                         "auto = live with --full when rocprofv3 is on PATH and N=1, else static; live needs --full")
    ap.add_argument("--encoder", default=None,
                    help="bi-encoder of the secondary leg (default: random:bert with hidden = --dim)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's result (scores.npy, ids.npy) to DIR: the inputs "
                         "are seeded, so two builds run with the same arguments can be compared output for output")
    args = ap.parse_args(argv)
    if not args.full:
        # a plain run: nothing but the headline's own set-up, warm-up and timed steps
        if args.traffic == "live":
            ap.error("--traffic live takes two profiler runs of its own: it needs --full")
        args.no_cpu_baseline = args.no_encode_leg = args.no_pipeline_leg = args.no_read_probe = True
        if args.traffic == "auto":
            args.traffic = "static"
    return args


DUMP_BYTES_MAX = 64_000_000


def dump_outputs(out_dir, D, I):
    """--dump-outputs: the (D, I) a caller of the search receives — scores.npy float32 [B, k] and ids.npy, the int64
    row ids as float64 (exact below 2**53).  Beyond DUMP_BYTES_MAX in all, a fixed seeded sample of the query rows is
    kept and named in query_rows.npy; a single row still too large keeps its leading (best-scoring) columns."""
    import numpy as np
    B, k = D.shape
    cols = max(1, min(k, (DUMP_BYTES_MAX - 8) // 12))
    n_rows = max(1, DUMP_BYTES_MAX // (12 * cols + 8))
    rows = np.arange(B)
    os.makedirs(out_dir, exist_ok=True)
    if n_rows < B:
        rows = np.sort(np.random.default_rng(0).choice(B, n_rows, replace=False))
        np.save(os.path.join(out_dir, "query_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(out_dir, "scores.npy"), np.ascontiguousarray(D[rows, :cols], dtype=np.float32))
    np.save(os.path.join(out_dir, "ids.npy"), np.ascontiguousarray(I[rows, :cols], dtype=np.float64))


def visible_gpus():
    """Number of HIP devices, counted in a CHILD process: the launcher itself must never initialise the
    GPU (a process that has may not start the ranks on this pool, and forked HIP state is unusable)."""
    code = "import torch,sys; sys.stdout.write(str(torch.cuda.device_count()))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("could not count GPUs: " + r.stderr[-400:])
    return int(r.stdout.strip().splitlines()[-1])


def spawn_ranks(n, cmd, env=None, relay=sys.stdout, log=sys.stderr, timeout=None):
    """Start `cmd` n times as fresh processes with the torchrun environment (RANK, LOCAL_RANK, WORLD_SIZE,
    LOCAL_WORLD_SIZE, MASTER_ADDR=127.0.0.1, a free MASTER_PORT), relay rank 0's stdout to `relay` and every
    other stream to `log`, and return the exit code: 0 only if EVERY rank exited 0.  When one rank fails the
    others are terminated by their own pids (they would wait for it in the next collective forever)."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    base = dict(os.environ if env is None else env)
    base.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "WORLD_SIZE": str(n),
                 "LOCAL_WORLD_SIZE": str(n), "HSA_ENABLE_IPC_MODE_LEGACY": base.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
                 "TS_BENCH_LAUNCHED_BY": "bench.py"})
    procs, pumps = [], []

    def pump(src, dst, tag):
        for line in iter(src.readline, ""):
            # rank 0's stdout carries THE json line; anything else a library prints there (gloo's "[Gloo] Rank 0 is
            # connected ..." for one) goes to the log, so that the caller's stdout is exactly one line
            if not tag and dst is relay and not line.lstrip().startswith("{"):
                log.write("[rank 0] " + line)
                log.flush()
                continue
            dst.write(tag + line if tag else line)
            dst.flush()
        src.close()

    for r in range(n):
        e = dict(base, RANK=str(r), LOCAL_RANK=str(r))
        p = subprocess.Popen(cmd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, bufsize=1)
        procs.append(p)
        for src, dst, tag in ((p.stdout, relay if r == 0 else log, "" if r == 0 else f"[rank {r}] "),
                              (p.stderr, log, f"[rank {r}] ")):
            t = threading.Thread(target=pump, args=(src, dst, tag), daemon=True)
            t.start()
            pumps.append(t)
    deadline = None if timeout is None else time.time() + timeout
    rc = 0
    live = set(range(n))
    while live:
        for r in sorted(live):
            c = procs[r].poll()
            if c is None:
                continue
            live.discard(r)
            if c != 0 and rc == 0:
                rc = c if c > 0 else 1
                log.write(f"bench.py launcher: rank {r} exited with {c}; stopping the other ranks\n")
        if (rc != 0 or (deadline is not None and time.time() > deadline)) and live:
            if rc == 0:
                rc = 124
                log.write("bench.py launcher: timeout; stopping the ranks\n")
            for r in live:
                procs[r].terminate()
            t_end = time.time() + 10
            for r in list(live):
                try:
                    procs[r].wait(max(0.1, t_end - time.time()))
                except subprocess.TimeoutExpired:
                    procs[r].kill()
                    procs[r].wait()
            live.clear()
        if live:
            time.sleep(0.05)
    for t in pumps:
        t.join(timeout=5)
    return rc


def launch_self(args):
    """`python bench.py --gpus N` without a launcher around it: become the launcher.  Nothing in this
    process has touched HIP (torch is not even imported yet)."""
    backend = os.environ.get("TS_BENCH_BACKEND", "nccl")
    if args.gpus > 1 and backend == "nccl":
        have = visible_gpus()
        if have < args.gpus:
            sys.stderr.write(f"bench.py: --gpus {args.gpus} but only {have} GPU(s) are visible; refusing to print a "
                             f"line that would be mislabelled (TS_BENCH_BACKEND=gloo rehearses the {args.gpus}-rank "
                             "code path on fewer devices)\n")
            return 2
    return spawn_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:])


def gen_rows(torch, n, d, seed, dtype, device):
    """Synthetic unit-norm rows, generated on the GPU in blocks."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=device, dtype=torch.float32)
    x = x / (x.norm(dim=1, keepdim=True) + 1e-8)
    return x.to(dtype)


def cpu_baseline(args, torch):
    import numpy as np
    from oracle import oracle
    n = min(args.cpu_sample_rows, args.rows)
    rng = np.random.default_rng(1234)
    c = rng.standard_normal((n, args.dim), dtype=np.float32)
    c /= (np.linalg.norm(c, axis=1, keepdims=True) + 1e-8)
    q = rng.standard_normal((args.batch, args.dim), dtype=np.float32)
    q /= (np.linalg.norm(q, axis=1, keepdims=True) + 1e-8)
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    try:  # the SGEMM runs in numpy's BLAS: report the threads THAT pool uses (it may cap below the core count)
        from threadpoolctl import threadpool_info
        blas = [int(p["num_threads"]) for p in threadpool_info() if p.get("user_api") == "blas"]
        if blas:
            cores = min(cores, max(blas))
    except Exception:
        pass
    k = min(args.k, n)
    oracle.ip_topk_blas(c, q, k)  # warm-up (BLAS thread pool, page faults)
    reps, t_total = 0, 0.0
    while t_total < 10.0 and reps < 50:
        t0 = time.perf_counter()
        oracle.ip_topk_blas(c, q, k)
        t_total += time.perf_counter() - t0
        reps += 1
    t = t_total / reps
    scale = args.rows / n
    return {
        "value": args.batch / (t * scale),
        "unit": "queries/s",
        "cores": cores,
        "kind": "port",
        "sample": (f"{n} of {args.rows} rows x {args.dim} fp32, batch {args.batch}, top-{k}; "
                   f"{reps} reps of {t * 1e3:.1f} ms, scaled x{scale:.1f} to the full corpus"),
    }


def encode_leg(args, torch, index, device, tdt, steps, world):
    """Secondary, separately reported: the same stage-1 search fed by the bi-encoder instead of
    pre-encoded queries — tokenise 64 synthetic query texts, one bf16 forward of a randomly
    initialised BERT-base-shaped encoder (no weights exist offline), x/(|x|+1e-8), cast to the
    index dtype, search.  Every rank encodes the (replicated) queries itself, as in §8e."""
    import numpy as np
    from tristage_rag_amd.encoders import SentenceEncoder
    if args.dim % 64:
        return None
    spec = args.encoder or f"random:bert:{args.dim}:12:{args.dim // 64}"
    # (the eager written-out forward.  Replaying the 64-query forward from a HIP graph was measured twice this round:
    # 17.5 k queries/s on the search's stream, 18.5 k on a second stream, against 18.8 k / 20.2 k eager — the forward's
    # 1.3 ms of GPU time does not hide under a scan that occupies 7/8 of the CUs)
    enc = SentenceEncoder(spec, device=str(device))
    rng = np.random.default_rng(99)
    vocab = [f"w{i}" for i in range(5000)]
    texts = [[" ".join(rng.choice(vocab, size=int(rng.integers(4, 16)))) for _ in range(args.batch)] for _ in range(4)]

    # The query forward of batch i+1 runs on its OWN stream beside the scan of batch i (the scan leaves an eighth of the
    # CUs free and is HBM-bound; the forward is ~180 small kernels): on one stream the GPU ran them one after the other,
    # 3.39 ms per step of which 2.2 ms are the scan.  The search waits for the batch's query tensor through an event.
    main = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device=device)

    def one(i, async_):
        side.wait_stream(main) if not async_ else None
        with torch.cuda.stream(side):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                e = enc.encode(texts[i % 4], batch_size=args.batch, convert_to_numpy=False, convert_to_tensor=True)
            q = (e / (e.norm(dim=1, keepdim=True) + 1e-8)).to(tdt)
            ready = torch.cuda.Event()
            ready.record(side)
        main.wait_event(ready)
        q.record_stream(main)
        return index.search(q, args.k, async_=True) if async_ else index.search(q, args.k)

    for i in range(2):
        one(i, False)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        one(i, True)
    index.finish()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    te = time.perf_counter()
    for i in range(4):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            enc.encode(texts[i % 4], batch_size=args.batch, convert_to_numpy=False, convert_to_tensor=True)
    torch.cuda.synchronize()
    enc_ms = (time.perf_counter() - te) / 4 * 1e3
    return {"encode_plus_stage1_qps": round(args.batch * steps / dt, 2), "steps": steps,
            "ms_per_step": round(dt / steps * 1e3, 4), "encode_ms_per_batch": round(enc_ms, 4),
            "encoder": spec + " (random init, hash tokenizer, bf16 autocast; forward of batch i+1 on a second stream beside the scan of batch i)"}


def pipeline_legs(torch):
    """Secondary, separately reported: the whole three-stage pipeline on the configs[2] shape —
    3 633 synthetic documents, stage 1 top-1000 -> stage 2 (resident token store, MaxSim) keep 100 -> stage 3
    (cross-encoder on cached token ids) top-10, bf16, 256 queries through RetrievalPipeline.search_many in calls of
    64 — with randomly initialised models of the reference's architectures (no weights exist offline: throughput
    only), once as the benchmark configuration has it (dense stage 1) and once with the reference's default
    BM25 + RRF fusion.  Exactly bench_pipeline.py's settings for its headline line (`--store --many 64 --ids --graphs`: the
    batched query forwards of stages 1 and 2 are replayed from HIP graphs — launch-bound otherwise — and give the eager
    results, tests/test_pipeline_gpu.py::test_hip_graph_query_forwards_match_eager)."""
    import bench_pipeline
    out = {}
    for name, extra in (("pipeline_search_many_qps", []), ("pipeline_search_many_bm25_rrf_qps", ["--bm25"])):
        r = bench_pipeline.run(bench_pipeline.parse_args(["--queries", "256", "--store", "--many", "64", "--ids", "--graphs"] + extra))
        out[name] = r["value"]
        out[name.replace("_qps", "_stage_ms_per_query")] = {k.replace("_time", ""): round(v * 1e3, 4)
                                                             for k, v in r["mean_stage_seconds"].items()}
        if "pipeline_config" not in out:
            out["pipeline_config"] = dict(r["config"], index_build_s=r["index_build_s"], queries=256,
                                          models="random init, hash tokenizer (throughput only)")
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return out


def live_traffic(args):
    """HBM bytes per launch of the dominant kernel from the PMC counters, measured NOW on this box: two child runs
    of this script under `rocprofv3 --pmc` (FETCH_SIZE and WRITE_SIZE need separate passes: MI355X_MICROARCH.md),
    FETCH_SIZE doubled (gfx950 counts 64 B per 128-B request of a wide streaming read), per launch like `achieved`.
    The kernel is the one with the largest FETCH_SIZE among the scan kernels (the filter scan reads the whole
    corpus, the sample scan 0.7 % of it).  Returns (bytes or None, detail)."""
    import csv
    import glob
    import shutil
    import signal
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, {"error": "rocprofv3 not on PATH"}
    tmp = tempfile.mkdtemp(prefix="ts_pmc_", dir="/tmp")
    raw = {}
    kernel = None
    t0 = time.time()
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            # the program itself follows `--` (no env/bash hop: the profiler's preload initialises the GPU first)
            cmd = [exe, "--pmc", counter, "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--steps", "3", "--warmup", "1", "--rows", str(args.rows), "--dim", str(args.dim), "--batch", str(args.batch),
                   "--k", str(args.k), "--dtype", args.dtype, "--no-cpu-baseline", "--no-encode-leg", "--no-pipeline-leg",
                   "--no-read-probe", "--traffic", "off", "--no-profile", "--step-events", "off"]
            if args.classic:
                cmd.append("--classic")
            if args.one_launch:
                cmd.append("--one-launch")
            env = dict(os.environ, TMPDIR="/tmp")
            p = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                                 start_new_session=True)
            try:
                _, err = p.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)     # exactly the process group started above
                p.wait()
                return None, {"error": f"{counter} pass exceeded 240 s"}
            if p.returncode != 0:
                return None, {"error": f"{counter} pass exited with {p.returncode}: {err[-300:]}"}
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if not files:
                return None, {"error": f"{counter} pass wrote no counter_collection.csv"}
            per = {}
            for r in csv.DictReader(open(files[0])):
                if r.get("Counter_Name") != counter:
                    continue
                per.setdefault(r["Kernel_Name"], []).append(float(r["Counter_Value"]))
            scans = {k: sum(v) / len(v) for k, v in per.items() if "scan" in k or "fused_kernel" in k}
            if not scans:
                return None, {"error": f"no scan kernel in the {counter} pass"}
            if kernel is None:
                kernel = max(scans, key=scans.get)
            raw[counter] = (scans.get(kernel, 0.0), len(per.get(kernel, [])))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    total = round(2 * raw["FETCH_SIZE"][0] * 1024 + raw["WRITE_SIZE"][0] * 1024)
    return total, {"source": "live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child runs of this bench (3 steps each)",
                   "kernel": kernel[:60], "FETCH_SIZE_KB_raw": round(raw["FETCH_SIZE"][0], 1),
                   "WRITE_SIZE_KB_raw": round(raw["WRITE_SIZE"][0], 1), "dispatches": raw["FETCH_SIZE"][1],
                   "correction": "2*FETCH_SIZE*1024 + WRITE_SIZE*1024 (gfx950: FETCH_SIZE counts 64 B per 128-B request)",
                   "seconds": round(time.time() - t0, 1)}


def main():
    args = parse_args()
    if args.gpus < 1:
        sys.stderr.write("bench.py: --gpus must be >= 1\n")
        return 2
    if args.steps < 1 or args.warmup < 0:
        sys.stderr.write("bench.py: --steps must be >= 1 and --warmup >= 0\n")
        return 2
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_self(args)      # N fresh ranks (RCCL), rank 0's JSON line relayed; non-zero if any rank fails
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        # never measure one thing and label it another
        if int(os.environ.get("RANK", "0")) == 0:
            sys.stderr.write(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} rank(s)\n")
        return 2
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # TS_BENCH_BACKEND=gloo: rehearsal of the N > 1 code path on a box with fewer GPUs than ranks
    # (ranks share devices, the exchange is staged through the host); never the measured setup
    backend = os.environ.get("TS_BENCH_BACKEND", "nccl")
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend != "nccl":
            local_rank = local_rank % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    else:
        torch.cuda.set_device(0)
        local_rank = 0
        if args.force_exchange:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29577")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    if world > 1 and dist.get_world_size() != args.gpus:
        raise RuntimeError(f"process group has {dist.get_world_size()} ranks, --gpus {args.gpus}")
    device = torch.device("cuda", local_rank)
    # RCCL needs one device per rank (it refuses duplicates); the gloo rehearsal lets ranks share devices
    n_devices = world if (backend == "nccl" or world == 1) else min(world, torch.cuda.device_count())
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[args.dtype]

    from tristage_rag_amd.index import FlatIPIndex
    from tristage_rag_amd.sharded import ShardedFlatIPIndex, shard_bounds

    # ---- build the (sharded) index; nothing here is timed
    lo, hi = shard_bounds(args.rows, world, rank)
    local = FlatIPIndex(args.dim, dtype=args.dtype, device=local_rank)
    local.classic_filter = args.classic or bool(os.environ.get("TS_BENCH_CLASSIC"))
    local.one_launch_filter = args.one_launch
    local.reserve(max(hi - lo, 1))
    blk = 500_000
    for r0 in range(lo, hi, blk):
        n = min(blk, hi - r0)
        local.add(gen_rows(torch, n, args.dim, 1234 + r0 // blk, tdt, device))
    if world > 1 or args.force_exchange:
        index = ShardedFlatIPIndex(args.dim, args.rows, dtype=args.dtype, device=local_rank,
                                   local_index=local)
        index.always_exchange = args.force_exchange
    else:
        index = local
    queries = [gen_rows(torch, args.batch, args.dim, 4321 + i, tdt, device) for i in range(4)]
    torch.cuda.synchronize()

    pipeline = (args.pipeline == "on") or (args.pipeline == "auto" and (world > 1 or args.force_exchange))

    def step(i):
        if args.sync:
            return index.search(queries[i % len(queries)], args.k)
        # the query tensors were materialised (and synchronised) before the loop
        return index.search(queries[i % len(queries)], args.k, async_=True, inputs_ready=pipeline)

    finish_at = []

    def finish():
        if not args.sync:
            index.finish()

    if args.dump_steps and hasattr(index, "_exchange_and_merge"):   # note when the wrapper's own (collective) finish() runs
        _wrapped_finish = index.finish

        def _noting_finish():
            finish_at.append(len(finish_at_steps))
            return _wrapped_finish()
        finish_at_steps = []
        index.finish = _noting_finish

    if args.submit_stream == "side" or (args.submit_stream == "auto" and pipeline):
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        torch.cuda.set_stream(side)
    for i in range(args.warmup):
        step(i)
    finish()
    # (stays in a plain run: five searches, some 10 ms at the default shape, and the timed steps below start from the
    # clocks and caches these leave, as they always have)
    # per-batch latency with a host sync after every batch (reported, not the metric)
    torch.cuda.synchronize()
    tl = time.perf_counter()
    for i in range(5):
        index.search(queries[i % len(queries)], args.k)
    torch.cuda.synchronize()
    sync_latency_ms = (time.perf_counter() - tl) / 5 * 1e3
    # every 4th batch is bracketed by HIP events on the scan stream (a timing event costs ~5 us
    # in-stream; the sampled launches are still inside the timed region)
    local.set_profiling(not args.no_profile, every=1 if args.sync else 4)
    local.timings(reset=True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    step_events = args.step_events == "on" or (args.step_events == "auto" and world == 1)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)] if step_events else []
    t0 = time.perf_counter()
    if evs:
        evs[0].record()
    for i in range(args.steps):
        if args.dump_steps and hasattr(index, "_exchange_and_merge"):
            finish_at_steps.append(i)
        D, I = step(i)
        if evs:
            evs[i + 1].record()   # on the submitting stream, which every batch's result is ordered on
    finish()                     # completes AND verifies every batch of the timed region
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    step_ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)] if evs else []
    tm = local.timings(reset=True)
    info = local.last_search_info()
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:   # the merged result is the same on every rank
        dump_outputs(args.dump_outputs, D.cpu().numpy(), I.cpu().numpy())

    # ---- roofline of the dominant kernel (this rank's shard)
    esize = 4 if args.dtype == "f32" else 2
    gran = 64 if args.dtype == "f32" else 128
    dpad = -(-args.dim // gran) * gran
    shard_rows = hi - lo
    alg_bytes = float(-(-shard_rows // 32) * 32) * dpad * esize
    scan_ms, scan_cnt = tm["filter_scan"] if tm["filter_scan"][1] else tm["dense"]
    kernel = (("fused_kernel (query image + thresholds + scan+filter)" if info.get("one_launch") else "scan_kernel<filter>")
              if tm["filter_scan"][1] else "dense path (scan+select)")
    roof = None
    if scan_cnt:
        avg_ms = scan_ms / scan_cnt
        achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
        traffic, traffic_detail = None, None
        want_live = args.traffic == "live" or (args.traffic == "auto" and world == 1)
        if want_live and rank == 0:
            try:
                traffic, traffic_detail = live_traffic(args)
            except Exception as e:   # never take the headline down
                traffic, traffic_detail = None, {"error": repr(e)}
        if traffic is None and args.traffic != "off":
            tpath = os.path.join(ROOT, "profiles", "traffic.json")
            if os.path.exists(tpath):
                try:
                    traffic = json.load(open(tpath)).get(f"{args.rows // world}x{args.dim}x{args.dtype}")
                    if traffic is not None:
                        traffic_detail = dict(traffic_detail or {}, source="static: profiles/traffic.json "
                                              "(rocprofv3 --pmc passes of an earlier session, same shape)")
                except Exception:
                    traffic = None
        roof = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_detail": traffic_detail,
                "kernel": kernel, "avg_kernel_ms": round(avg_ms, 4), "launches": scan_cnt,
                "algorithmic_bytes_per_launch": alg_bytes}
        if not args.no_read_probe:
            try:   # the streaming ceiling of THIS box: the scan's access pattern with the arithmetic taken out
                local.read_probe(reps=3)          # (the probe follows seconds of host work: clocks and DRAM pages warm first)
                pr = local.read_probe(reps=10)
                roof["measured_read_peak"] = round(pr["gbps_avg"], 1)
                roof["measured_read_peak_best"] = round(pr["gbps_best"], 1)
                roof["frac_of_measured_read_peak"] = round(achieved / pr["gbps_avg"], 4)
                if achieved > pr["gbps_best"]:
                    # seen on some boxes (up to 3 %): the pure-load probe runs slower than the scan that does the same loads AND
                    # the arithmetic — a reference point of this box, not an upper bound
                    roof["read_probe_note"] = "the probe's best pass is below the scan's rate on this box: a reference point, not a bound"
                roof["read_probe"] = ("ts_index_read_probe: read-only kernel over this index's tiled corpus, same grid / "
                                      "block order / nt loads as the scan, 3 warm-up + 10 timed passes, HIP events")
            except Exception as e:
                roof["measured_read_peak"] = None
                roof["read_probe_error"] = repr(e)

    enc_leg = None
    if not args.no_encode_leg:
        try:
            enc_leg = encode_leg(args, torch, index, device, tdt, max(4, min(args.steps, 20)), world)
        except Exception as e:  # the secondary leg must never take the headline measurement down
            enc_leg = {"error": repr(e)}

    if world == 1 and not args.no_pipeline_leg:
        try:
            legs = pipeline_legs(torch)
            enc_leg = dict(enc_leg or {}, **legs)
        except Exception as e:
            enc_leg = dict(enc_leg or {}, pipeline_error=repr(e))

    def _rows_label(n):
        return f"{n // 1_000_000}M" if n % 1_000_000 == 0 and n >= 1_000_000 else (
            f"{n / 1e6:g}M" if n >= 1_000_000 else str(n))

    if rank == 0:
        out = {
            "metric": (f"end-to-end queries/sec @{_rows_label(args.rows)}x{args.dim} corpus "
                       "(stage-1 exact top-k, pre-encoded HBM-resident queries)"),
            "value": round(args.batch * args.steps / elapsed, 2),
            "unit": "queries/s",
            "n_gpus": world,
            "world_size": dist.get_world_size() if dist.is_initialized() else 1,
            "backend": (("rccl (torch.distributed nccl)" if backend == "nccl" else backend) if dist.is_initialized()
                        else "none (single process)"),
            "distinct_devices": n_devices,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "ms_per_step_min": round(min(step_ms), 4) if step_ms else None,
            "ms_per_step_max": round(max(step_ms), 4) if step_ms else None,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {"workload": (f"synthetic {args.rows}x{args.dim} {args.dtype} corpus, batch-{args.batch} "
                                    f"queries, stage-1 exact top-{args.k}, row-sharded over {world} GPU(s)"
                                    + ((", RCCL all-gather + HIP merge" if backend == "nccl" else
                                        f", REHEARSAL: {backend} group, ranks share devices, host-staged exchange")
                                       if world > 1 else "")),
                       "rows": args.rows, "dim": args.dim, "batch": args.batch, "k": args.k,
                       "submission": "synchronous per batch" if args.sync else
                                     ("batches enqueued back to back (async" + ("" if not pipeline else ", pipelined: prep/select of "
                                      "neighbouring batches overlap the scan") + "), verified by finish() in the timed region"),
                       "sync_batch_latency_ms": round(sync_latency_ms, 4),
                       "search_path": info["path"] + (" (one launch: query image + thresholds + scan+filter)"
                                                      if info.get("one_launch") else ""),
                       "max_candidates_per_query": info["max_candidates"],
                       "phase_ms_per_step": {p: round(v[0] / max(v[1], 1), 4) for p, v in tm.items() if v[1]},
                       **({"step_ms": [round(x, 3) for x in step_ms], "finish_at": finish_at} if args.dump_steps else {})},
            "roofline": roof,
            "secondary": enc_leg,
        }
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args, torch)
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)
