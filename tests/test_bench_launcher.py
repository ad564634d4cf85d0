"""bench.py's own launcher (`python bench.py --gpus N` with no torchrun around it): the plumbing on the
CPU — the ranks get the torchrun environment, rank 0's stdout is what the caller sees, one failing rank
fails the job and stops the others — and, under -m gpu, the gloo rehearsal of the 2-rank bench started
through exactly that code path."""
import io
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)     # top level imports the standard library only: no torch, no HIP
    return m


def test_launcher_module_imports_without_torch():
    code = ("import sys, importlib.util as u; s = u.spec_from_file_location('b', sys.argv[1]); m = u.module_from_spec(s); "
            "s.loader.exec_module(m); assert 'torch' not in sys.modules, 'the launcher must not import torch'")
    subprocess.run([sys.executable, "-c", code, BENCH], check=True)


def test_ranks_see_the_torchrun_environment():
    b = _bench_module()
    out, log = io.StringIO(), io.StringIO()
    child = ("import os, json; print('[lib] chatter on stdout'); print(json.dumps({k: os.environ.get(k) for k in "
             "('RANK','LOCAL_RANK','WORLD_SIZE','LOCAL_WORLD_SIZE','MASTER_ADDR','MASTER_PORT','HSA_ENABLE_IPC_MODE_LEGACY')}))")
    rc = b.spawn_ranks(3, [sys.executable, "-c", child], relay=out, log=log)
    assert rc == 0
    assert out.getvalue().count("\n") == 1 and "[rank 0] [lib] chatter" in log.getvalue()   # exactly one line reaches the caller
    mine = json.loads(out.getvalue())                       # rank 0's json line only
    assert mine["RANK"] == "0" and mine["LOCAL_RANK"] == "0" and mine["WORLD_SIZE"] == "3"
    assert mine["MASTER_ADDR"] == "127.0.0.1" and int(mine["MASTER_PORT"]) > 0 and mine["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    others = [json.loads(l.split("] ", 1)[1]) for l in log.getvalue().splitlines()
              if l.startswith("[rank ") and not l.startswith("[rank 0]") and "{" in l]
    assert sorted(o["RANK"] for o in others) == ["1", "2"]
    assert all(o["MASTER_PORT"] == mine["MASTER_PORT"] and o["WORLD_SIZE"] == "3" for o in others)


def test_one_failing_rank_fails_the_job_and_stops_the_others():
    b = _bench_module()
    out, log = io.StringIO(), io.StringIO()
    child = ("import os, sys, time\n"
             "if os.environ['RANK'] == '1': sys.exit(7)\n"
             "time.sleep(120)\n")              # a rank waiting in a collective for the dead one
    t0 = time.time()
    rc = b.spawn_ranks(2, [sys.executable, "-c", child], relay=out, log=log)
    assert rc == 7 and time.time() - t0 < 60
    assert "rank 1 exited with 7" in log.getvalue()


def test_refuses_a_world_size_that_is_not_gpus():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4"], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout.strip() == "" and "WORLD_SIZE=2" in r.stderr


def test_refuses_more_gpus_than_visible():
    """No launcher around it and fewer devices than --gpus: a non-zero exit and NO json line (round 2 printed a
    one-GPU line labelled by a stderr warning)."""
    import torch
    have = torch.cuda.device_count()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TS_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(have + 2), "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and r.stdout.strip() == "" and "visible" in r.stderr


def test_refuses_zero_steps():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout.strip() == "" and "--steps" in r.stderr


def test_plain_run_measures_the_headline_only_and_full_adds_the_rest():
    """Without --full nothing that takes runs of its own is on (CPU baseline, encoder and pipeline legs, read probe,
    live PMC traffic); --full turns all of it on, and the --no-* switches and --traffic choose among it."""
    b = _bench_module()
    plain = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "3"])
    assert not plain.full
    assert plain.no_cpu_baseline and plain.no_encode_leg and plain.no_pipeline_leg and plain.no_read_probe
    assert plain.traffic == "static" and not plain.no_profile and plain.dump_outputs is None
    assert (plain.steps, plain.warmup, plain.rows, plain.dim, plain.batch, plain.k, plain.dtype) == (20, 3, 10_000_000, 768, 64, 1000, "f16")
    assert b.parse_args(["--traffic", "off"]).traffic == "off"
    full = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "3", "--full"])
    assert full.full and full.traffic == "auto"
    assert not (full.no_cpu_baseline or full.no_encode_leg or full.no_pipeline_leg or full.no_read_probe)
    assert (full.steps, full.warmup, full.rows, full.dim, full.batch, full.k, full.dtype) == (20, 3, 10_000_000, 768, 64, 1000, "f16")
    some = b.parse_args(["--full", "--no-pipeline-leg", "--traffic", "live"])
    assert some.no_pipeline_leg and not some.no_encode_leg and some.traffic == "live"


def test_live_traffic_without_full_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--traffic", "live"], capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout.strip() == "" and "--full" in r.stderr


def test_dump_outputs_dtypes_and_size_cap(tmp_path):
    import numpy as np
    b = _bench_module()
    rng = np.random.default_rng(3)
    D = rng.standard_normal((8, 5)).astype(np.float32)
    I = rng.integers(0, 10_000_000, size=(8, 5))
    b.dump_outputs(str(tmp_path / "small"), D, I)
    assert sorted(os.listdir(tmp_path / "small")) == ["ids.npy", "scores.npy"]
    s, i = np.load(tmp_path / "small" / "scores.npy"), np.load(tmp_path / "small" / "ids.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64
    assert np.array_equal(s, D) and np.array_equal(i, I.astype(np.float64))
    # beyond the cap: the same seeded sample of query rows every time, named in query_rows.npy, within the cap
    b.DUMP_BYTES_MAX = 3 * (12 * 5 + 8)
    for name in ("a", "b"):
        b.dump_outputs(str(tmp_path / name), D, I)
    rows = np.load(tmp_path / "a" / "query_rows.npy").astype(np.int64)
    assert len(rows) == 3 and np.array_equal(rows, np.load(tmp_path / "b" / "query_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), D[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "ids.npy"), I[rows].astype(np.float64))
    # one row larger than the cap keeps its leading (best-scoring) columns
    b.DUMP_BYTES_MAX = 12 * 2 + 8
    b.dump_outputs(str(tmp_path / "c"), D, I)
    assert np.array_equal(np.load(tmp_path / "c" / "scores.npy"), D[np.load(tmp_path / "c" / "query_rows.npy").astype(np.int64), :2])


@pytest.mark.gpu
def test_bench_dump_outputs_is_the_last_step_and_repeats(tmp_path):
    """`--dump-outputs DIR`: the result of the last timed step (queries[(steps - 1) % 4] of bench.py's seeded set)
    against the float64 oracle on the same seeded corpus, and the same arrays bit for bit from a second run."""
    import numpy as np
    import torch
    from helpers import check_topk
    b = _bench_module()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    rows, dim, k, steps = 100_000, 128, 100, 7
    dumps = []
    for name in ("a", "b"):
        out_dir = str(tmp_path / name)
        r = subprocess.run([sys.executable, BENCH, "--steps", str(steps), "--warmup", "1", "--rows", str(rows), "--dim",
                            str(dim), "--k", str(k), "--no-cpu-baseline", "--no-encode-leg", "--no-pipeline-leg",
                            "--no-read-probe", "--traffic", "off", "--dump-outputs", out_dir],
                           env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        dumps.append((np.load(os.path.join(out_dir, "scores.npy")), np.load(os.path.join(out_dir, "ids.npy"))))
    (D, I), (D2, I2) = dumps
    assert D.dtype == np.float32 and I.dtype == np.float64 and D.shape == I.shape == (64, k)
    assert np.array_equal(D, D2) and np.array_equal(I, I2)
    dev = torch.device("cuda", 0)
    corpus = b.gen_rows(torch, rows, dim, 1234, torch.float16, dev).float().cpu().numpy()
    q = b.gen_rows(torch, 64, dim, 4321 + (steps - 1) % 4, torch.float16, dev).float().cpu().numpy()
    check_topk(D, I.astype(np.int64), corpus, q, k)


@pytest.mark.gpu
def test_bench_plain_line_is_the_headline_and_full_adds_the_rest():
    """A plain run prints the headline fields and the in-step roofline, with `secondary` and `cpu_baseline` null and no
    read probe; the same command with --full carries all of them (live PMC traffic left to the full-size run:
    `--traffic static`)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    base = [sys.executable, BENCH, "--gpus", "1", "--steps", "8", "--warmup", "2", "--rows", "200000", "--k", "100"]
    lines = []
    for extra in ([], ["--full", "--traffic", "static", "--cpu-sample-rows", "50000"]):
        r = subprocess.run(base + extra, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    plain, full = lines
    for line in lines:
        assert line["metric"].startswith("end-to-end queries/sec @200000x768 corpus") and line["unit"] == "queries/s"
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "f16"
        assert line["steps"] == 8 and line["warmup"] == 2 and line["roofline"]["avg_kernel_ms"] > 0
        assert abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    assert plain["secondary"] is None and plain["cpu_baseline"] is None and "measured_read_peak" not in plain["roofline"]
    assert full["cpu_baseline"]["value"] > 0 and full["roofline"]["measured_read_peak"] > 0
    assert full["secondary"]["encode_plus_stage1_qps"] > 0 and full["secondary"]["pipeline_search_many_qps"] > 0
    assert full["secondary"]["pipeline_search_many_bm25_rrf_qps"] > 0


@pytest.mark.gpu
def test_bench_gpus_2_starts_two_ranks_by_itself():
    """`python bench.py --gpus 2` as the driver types it, TS_BENCH_BACKEND=gloo because the test box has one GPU
    (ranks share it, the exchange is staged through the host): two processes, a 2-rank process group, the line
    says so."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["TS_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "6", "--warmup", "2", "--rows", "400000",
                        "--dim", "256", "--k", "100", "--no-encode-leg", "--no-pipeline-leg", "--no-read-probe"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world_size"] == 2 and out["backend"] == "gloo"
    assert out["distinct_devices"] == 1 and "REHEARSAL" in out["config"]["workload"]
    assert out["value"] > 0 and out["scaling"] == "strong"


@pytest.mark.gpu
def test_bench_pipeline_gpus_2_runs_the_row_sharded_pipeline():
    """`python bench_pipeline.py --gpus 2 --store --ids --many 8` starts its own two ranks (gloo rehearsal: both on the
    one GPU of the test box) and times ShardedRetrievalPipeline.search_many: one JSON line from rank 0, n_gpus 2,
    rank 0 holding half of the rows / token matrices."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["TS_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_pipeline.py"), "--gpus", "2", "--docs", "600", "--queries", "16",
                        "--store", "--ids", "--many", "8", "--stage1", "random:tiny", "--stage2", "random:tiny",
                        "--stage3", "random:tiny"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["config"]["array_path"]
    assert out["rank0_shard"]["rows"] == [0, 300] and out["rank0_shard"]["documents_total"] == 600
    assert out["rank0_shard"]["stage2_token_rows"] > 0 and out["rank0_shard"]["stage3_id_cache_documents"] == 300
