"""Every entry point with a stream parameter held to its contract (tests/stream_order.py) on a NON-BLOCKING side
stream with its inputs arriving late: the decoys are overwritten behind a delay on that stream, the call follows, a
consumer clones the outputs at once.  Results are compared bit for bit with the same call made beforehand on the
default stream with everything synchronised; that expected value is checked once against the family's oracle.

TS_STREAM_ORDER_PROBE=<path>: the measured host time of every enqueue-only call, the delay and this file's total time
are written there as JSON (profiles/stream_order_probe.json)."""
import ctypes
import inspect
import json
import os
import time

import numpy as np
import pytest

import bm25_model as bm
import group_model as gm
import mmr_model as mm
import passage_model as pm
import stream_order as so
from helpers import check_topk, make_corpus
from oracle import oracle

pytestmark = pytest.mark.gpu

B, K, D128 = 64, 10, 128
TIE_TOL = inspect.signature(oracle.check_topk).parameters["tie_tol"].default
CASES = {}


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


class Env:
    """Shared, read-only data of the module: corpora, built indexes, the harness."""

    def __init__(self, torch):
        from tristage_rag_amd import _lib, index
        self.torch, self.index, self._lib, self.lib = torch, index, _lib, _lib.load()
        self.h = so.Harness(torch)
        self._memo = {}
        self.t0 = time.perf_counter()
        self.seconds = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def corpus(self, n, d=D128, seed=11):
        return self.memo(("corpus", n, d, seed), lambda: make_corpus(n, d, seed=seed))

    def corpus_t(self, n, d=D128, seed=11):
        return self.memo(("corpus_t", n, d, seed), lambda: self.torch.from_numpy(self.corpus(n, d, seed)).cuda().half())

    def queries(self, d, seed, n=B, dtype=None):
        t = self.torch.from_numpy(make_corpus(n, d, seed=seed)).cuda()
        return t.to(dtype or self.torch.float16).contiguous()

    def flat(self, dtype, n, d=D128):
        def build():
            idx = self.index.FlatIPIndex(d, dtype=dtype)
            idx.add(self.corpus_t(n, d).float() if dtype == "f32" else self.corpus_t(n, d))
            return idx
        return self.memo(("flat", dtype, n, d), build)

    def sp(self):
        return ctypes.c_void_p(int(self.torch.cuda.current_stream().cuda_stream))

    def sentinels(self, rows, k=K):
        torch = self.torch
        return (torch.full((rows, k), so.SENT_F, dtype=torch.float32, device="cuda"),
                torch.full((rows, k), so.SENT_I, dtype=torch.int64, device="cuda"))

    def close(self):
        for key, v in self._memo.items():
            if hasattr(v, "close"):
                v.close()
            elif key == "bm25":
                self.lib.ts_bm25_destroy(v[1])


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    e = Env(torch)
    yield e
    torch.cuda.synchronize()
    path = os.environ.get("TS_STREAM_ORDER_PROBE")
    if path:
        enq = {k: round(v, 4) for k, v in sorted(e.h.enqueue_ms.items())}
        json.dump({"delay_kind": e.h.delay_kind, "delay_ms_chosen": so.DELAY_MS,
                   "delay_ms_measured": round(e.h.delay_measured_ms, 3),
                   "slowest_enqueue_host_ms": max(enq.values()) if enq else None, "enqueue_host_ms": enq,
                   "file_total_seconds": round(time.perf_counter() - e.t0, 2),
                   "case_seconds": {k: round(v, 3) for k, v in sorted(e.seconds.items())}},
                  open(path, "w"), indent=1)
    e.close()


@pytest.fixture(autouse=True)
def _seconds(env, request):
    """The time of every test that is not a table case goes into the probe file too."""
    t0 = time.perf_counter()
    yield
    if not request.node.name.startswith("test_case["):
        env.seconds[request.node.name] = time.perf_counter() - t0


def _np(t):
    return t.detach().float().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


# =============================================================================================== the harness itself
def test_harness_flags_what_it_must(env):
    """Once per module: the side stream does not block against the null stream; a call that leaks its work to the
    default stream, one that does not make the stream wait for its internal stream and one that waits for the GPU are
    each flagged; an honest call is not."""
    h = env.h
    assert so.DELAY_MS <= so.DELAY_MAX_MS
    assert 0.7 * so.DELAY_MS <= h.delay_measured_ms <= so.DELAY_MAX_MS, h.delay_measured_ms
    rep = h.self_check()
    print(rep)
    assert rep["default_done_while_side_pending"]
    assert rep["honest"] == []
    assert any("decoy" in f for f in rep["leak"]), rep["leak"]
    assert any("consumer" in f for f in rep["no_wait"]), rep["no_wait"]
    assert any("waited for the GPU" in f for f in rep["host_wait"]), rep["host_wait"]


# ======================================================================================================= flat index
def _search_case(env, name, dtype, n, path=None):
    torch, idx = env.torch, env.flat(dtype, n)
    qd = torch.float32 if dtype == "f32" else torch.float16
    real, decoy = {"q": env.queries(D128, 1, dtype=qd)}, {"q": env.queries(D128, 2, dtype=qd)}
    if path is not None:
        assert env.lib.ts_index_filter_path(idx._h, K) == path

    def call(st, b):
        D, I = env.sentinels(B)
        idx.search(b["q"], K, out=(D, I))
        return D, I

    def anchor(real, outs):
        q = _np(real["q"])
        check_topk(_np(outs[0]), outs[1].cpu().numpy(), idx.reconstruct_n(), oracle.quantize(q, "bf16") if dtype == "fp8" else q, K)
    return so.Case(name, lambda: (real, decoy), call, anchor=anchor, final=True)


@case("flat_search_dense")
def _(env):
    return _search_case(env, "flat_search_dense", "f16", 4096, path=0)


@case("flat_search_filter")
def _(env):
    return _search_case(env, "flat_search_filter", "f16", 40960, path=1)


@case("flat_search_fp8")
def _(env):
    return _search_case(env, "flat_search_fp8", "fp8", 40960)


@case("flat_search_f32")
def _(env):
    return _search_case(env, "flat_search_f32", "f32", 4096)


@case("flat_async_finish")
def _(env):
    idx = env.flat("f16", 40960)
    real, decoy = {"q": env.queries(D128, 1)}, {"q": env.queries(D128, 2)}

    def call(st, b):
        idx.coalesce = False
        D, I = env.sentinels(B)
        idx.search(b["q"], K, async_=True, out=(D, I))
        return D, I

    def cleanup(st):
        idx.coalesce = True
    return so.Case("flat_async_finish", lambda: (real, decoy), call, after=lambda st, o: idx.finish(), cleanup=cleanup,
                   early=True, consume_after=True)


@case("flat_stream_order_dense")
def _(env):
    idx = env.flat("f16", 4096)
    assert env.lib.ts_index_filter_path(idx._h, K) == 0
    real, decoy = {"q": env.queries(D128, 1)}, {"q": env.queries(D128, 2)}
    return so.Case("flat_stream_order_dense", lambda: (real, decoy), lambda st, b: idx.search_in_stream_order(b["q"], K),
                   cleanup=lambda st: idx.finish(), early=True)   # consumed in stream order, no finish in between


@case("flat_pipeline_inputs_ready")
def _(env):
    idx = env.flat("f16", 40960)
    real = {"q": env.queries(D128, 1)}

    def call(st, b):
        D, I = env.sentinels(B)
        idx.search(b["q"], K, async_=True, inputs_ready=True, out=(D, I))
        return D, I
    # TS_FLAG_PIPELINE: the caller guarantees complete queries, so nothing arrives late: the early consumer only
    return so.Case("flat_pipeline_inputs_ready", lambda: (real, real), call, after=lambda st, o: idx.finish(), early=True,
                   late=False, consume_after=True)


@case("flat_search_allowed")
def _(env):
    torch, n = env.torch, 40960
    idx = env.flat("f16", n)
    rng = np.random.default_rng(3)
    masks = [rng.random(n) < 0.5 for _ in range(2)]
    packed = [torch.from_numpy(env.index.pack_allowed(m, n).view(np.int32)).cuda() for m in masks]
    real = {"q": env.queries(D128, 1), "mask": packed[0]}
    decoy = {"q": env.queries(D128, 2), "mask": packed[1]}

    def call(st, b):
        D, I = env.sentinels(B)
        idx.search(b["q"], K, allowed=b["mask"], out=(D, I))
        return D, I

    def anchor(real, outs):
        rows = np.flatnonzero(masks[0])
        I = outs[1].cpu().numpy()
        assert np.isin(I, rows).all()
        check_topk(_np(outs[0]), np.searchsorted(rows, I), env.corpus(n)[rows], _np(real["q"]), K)
    return so.Case("flat_search_allowed", lambda: (real, decoy), call, anchor=anchor, final=True)


@case("flat_scores")
def _(env):
    idx = env.flat("f16", 4096)
    real, decoy = {"q": env.queries(D128, 1)}, {"q": env.queries(D128, 2)}

    def anchor(real, outs):
        want = _np(real["q"]).astype(np.float64) @ env.corpus(4096).astype(np.float64).T
        assert np.abs(_np(outs[0]) - want).max() < 1e-3
    return so.Case("flat_scores", lambda: (real, decoy), lambda st, b: (idx.scores(b["q"]),), anchor=anchor, final=True)


@case("flat_range_search")
def _(env):
    idx, radius = env.flat("f16", 40960), 0.2
    real, decoy = {"q": env.queries(D128, 1)}, {"q": env.queries(D128, 2)}

    def anchor(real, outs):
        L, D, I = (o.cpu().numpy() for o in outs)
        s64 = _np(real["q"]).astype(np.float64) @ env.corpus(40960).astype(np.float64).T
        assert L[-1] > B                                         # the radius does select rows
        for b in range(B):
            got = I[L[b]:L[b + 1]]
            assert (s64[b, got] >= radius - 1e-3).all()
            assert np.isin(np.flatnonzero(s64[b] >= radius + 1e-3), got).all()
    return so.Case("flat_range_search", lambda: (real, decoy), lambda st, b: idx.range_search(b["q"], radius),
                   anchor=anchor, final=True)


@case("flat_reconstruct")
def _(env):
    torch, idx = env.torch, env.flat("f16", 4096)

    def call(st, b):
        out = torch.full((300, D128), so.SENT_F, dtype=torch.float32, device="cuda")
        env._lib.check(env.lib.ts_index_reconstruct(idx._h, 100, 300, ctypes.c_void_p(out.data_ptr()), 0, env.sp()))
        return out, idx.reconstruct_n(100, 300)

    def anchor(real, outs):
        assert np.array_equal(_np(outs[0]), env.corpus(4096)[100:400]) and np.array_equal(outs[1], env.corpus(4096)[100:400])
    return so.Case("flat_reconstruct", lambda: ({}, {}), call, anchor=anchor, final=True)


@case("flat_add")
def _(env):
    real, decoy = {"x": env.queries(D128, 21, n=1000)}, {"x": env.queries(D128, 22, n=1000)}

    def call(st, b):
        st.add(b["x"])
        return (st.reconstruct_n(),)
    return so.Case("flat_add", lambda: (real, decoy), call, setup=lambda: env.index.FlatIPIndex(D128, dtype="f16"),
                   cleanup=lambda st: st.close(), final=True,
                   anchor=lambda real, outs: np.testing.assert_array_equal(outs[0], _np(real["x"])))


@case("flat_update")
def _(env):
    ids = np.random.default_rng(5).choice(4096, size=100, replace=False).astype(np.int64)
    real, decoy = {"x": env.queries(D128, 23, n=100)}, {"x": env.queries(D128, 24, n=100)}

    def setup():
        idx = env.index.FlatIPIndex(D128, dtype="f16")
        idx.add(env.corpus_t(4096))
        return idx

    def call(st, b):
        st.update_rows(ids, b["x"])
        return (st.reconstruct_n(),)

    def anchor(real, outs):
        want = env.corpus(4096).copy()
        want[ids] = _np(real["x"])
        assert np.array_equal(outs[0], want)
    return so.Case("flat_update", lambda: (real, decoy), call, setup=setup, cleanup=lambda st: st.close(), anchor=anchor,
                   final=True)


def _mmr_inputs(env, n, C=40):
    torch = env.torch
    out = []
    for seed in (31, 32):
        rng = np.random.default_rng(seed)
        ids = np.stack([rng.permutation(n)[:C] for _ in range(B)]).astype(np.int64)
        rel = rng.random((B, C), dtype=np.float32)
        out.append({"ids": torch.from_numpy(ids).cuda(), "rel": torch.from_numpy(rel).cuda()})
    return out


@case("flat_mmr")
def _(env):
    idx = env.flat("f16", 4096)
    real, decoy = _mmr_inputs(env, 4096)

    def anchor(real, outs):
        X = env.corpus(4096).astype(np.float64)
        ids, rel, D, I = real["ids"].cpu().numpy(), _np(real["rel"]), _np(outs[0]), outs[1].cpu().numpy()
        for b in range(0, B, 8):
            pos = np.array([int(np.nonzero(ids[b] == i)[0][0]) for i in I[b]])
            assert np.array_equal(D[b], rel[b, pos])
            mm.step_valid(rel[b], X[ids[b]] @ X[ids[b]].T, pos, 0.5, TIE_TOL)
    return so.Case("flat_mmr", lambda: (real, decoy), lambda st, b: idx.mmr(b["ids"], b["rel"], K, 0.5), anchor=anchor,
                   early=True)


@case("flat_search_mmr")
def _(env):
    idx = env.flat("f16", 4096)
    real, decoy = {"q": env.queries(D128, 1)}, {"q": env.queries(D128, 2)}
    # a synchronous search with the selection enqueued behind it: consumed in stream order
    return so.Case("flat_search_mmr", lambda: (real, decoy), lambda st, b: idx.search_mmr(b["q"], K, 40, 0.5))


@case("group_topk")
def _(env):
    torch, tabs = env.torch, gm.tables(4096)
    ins = []
    for seed, tab in ((0, "fives"), (1, "three")):
        ids, scores = gm.lists(B, 64, n=4096, seed=seed)
        ins.append({"ids": torch.from_numpy(ids).cuda(), "scores": torch.from_numpy(scores + seed).cuda(),
                    "groups": torch.from_numpy(tabs[tab]).cuda()})

    def anchor(real, outs):
        want = gm.group_topk(real["ids"].cpu().numpy(), _np(real["scores"]), real["groups"].cpu().numpy(), 5, 2)
        for g, w in zip(outs, want):
            assert np.array_equal(g.cpu().numpy(), w)
    return so.Case("group_topk", lambda: tuple(ins),
                   lambda st, b: env.index.group_topk(b["ids"], b["scores"], b["groups"], 5, 2), anchor=anchor, early=True)


@case("flat_search_grouped")
def _(env):
    idx = env.flat("f16", 4096)
    groups = env.torch.from_numpy(gm.tables(4096)["fives"]).cuda()
    real, decoy = {"q": env.queries(D128, 1)}, {"q": env.queries(D128, 2)}
    return so.Case("flat_search_grouped", lambda: (real, decoy), lambda st, b: idx.search_grouped(b["q"], 5, groups, 2))


def _merge_inputs(env, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((4, B, K)).astype(np.float32), rng.integers(0, 10 ** 6, size=(4, B, K)).astype(np.int64)


def _merge_anchor(s, i, outs):
    ws, wi = oracle.merge_topk(s, i, K)
    assert np.array_equal(_np(outs[0]), ws) and np.array_equal(outs[1].cpu().numpy(), wi)


@case("merge_topk")
def _(env):
    torch = env.torch
    data = [_merge_inputs(env, s) for s in (41, 42)]
    ins = [{"s": torch.from_numpy(s).cuda(), "i": torch.from_numpy(i).cuda()} for s, i in data]
    return so.Case("merge_topk", lambda: tuple(ins), lambda st, b: env.index.merge_topk(b["s"], b["i"]),
                   anchor=lambda real, outs: _merge_anchor(*data[0], outs), early=True)


@case("merge_topk_packed")
def _(env):
    torch = env.torch
    data = [_merge_inputs(env, s) for s in (41, 42)]
    ids_at, nbytes = env.index.packed_layout(B, K)
    ins = []
    for s, i in data:
        buf = np.zeros((4, nbytes), dtype=np.uint8)
        for r in range(4):
            buf[r, : 4 * B * K] = s[r].view(np.uint8).reshape(-1)
            buf[r, ids_at:] = i[r].view(np.uint8).reshape(-1)
        ins.append({"g": torch.from_numpy(buf.reshape(-1)).cuda()})
    return so.Case("merge_topk_packed", lambda: tuple(ins), lambda st, b: env.index.merge_topk_packed(b["g"], 4, B, K),
                   anchor=lambda real, outs: _merge_anchor(*data[0], outs), early=True)


# ------------------------------------------------------------------------------------------------ the coalesced queue
def _queue_case(env, name, d, wide):
    idx = env.flat("f16", 40960, d)
    real, decoy = {"q": env.queries(d, 1, n=128)}, {"q": env.queries(d, 2, n=128)}

    def call(st, b):
        idx.classic_filter, idx.coalesce, idx.wide_passes = True, True, wide
        D, I = env.sentinels(128)
        for i in range(0, 128, 32):                       # four batches of 32: the queries are read in stream order
            idx.search(b["q"][i:i + 32], K, async_=True, out=(D[i:i + 32], I[i:i + 32]))
        idx.flush()                                        # held passes launched; the consumer follows in stream order
        return D, I

    def cleanup(st):
        idx.classic_filter, idx.wide_passes = False, "auto"

    def anchor(real, outs):
        check_topk(_np(outs[0]), outs[1].cpu().numpy(), env.corpus(40960, d), _np(real["q"]), K)
    return so.Case(name, lambda: (real, decoy), call, after=lambda st, o: idx.finish(), cleanup=cleanup, anchor=anchor,
                   early=True)


@case("queue_narrow")
def _(env):
    return _queue_case(env, "queue_narrow", D128, False)


@case("queue_wide")
def _(env):
    assert env.lib.ts_coalesce_groups_wide(640, 1) == 6
    return _queue_case(env, "queue_wide", 640, True)


# ================================================================================================================ IVF
NLIST, NPROBE = 8, 3


def _ivf_base(env):
    def build():
        ivf = env.index.IVFFlatIndex(D128, NLIST, dtype="f16", nprobe=NPROBE)
        ivf.train(env.corpus_t(40960)[:4096], niter=4)
        ivf.add(env.corpus_t(40960))
        return ivf
    return env.memo("ivf", build)


def _ivf_fresh(env, rows=None, centroids=True):
    ivf = env.index.IVFFlatIndex(D128, NLIST, dtype="f16", nprobe=NPROBE)
    if centroids:
        ivf.set_centroids(env.memo("cent", lambda: _ivf_base(env).centroids))
    if rows is not None:
        ivf.add(rows)
    return ivf


@case("ivf_search")
def _(env):
    ivf, flat = _ivf_base(env), env.flat("f16", 40960)
    real, decoy = {"q": env.queries(D128, 1)}, {"q": env.queries(D128, 2)}

    def call(st, b):
        D, I = env.sentinels(B)
        ivf.search(b["q"], K, out=(D, I))
        return D, I

    def anchor(real, outs):   # the scores are the flat index's, bit for bit, and descending
        D, I = outs[0].cpu(), outs[1].cpu()
        assert (I >= 0).all() and (D[:, 1:] <= D[:, :-1]).all()
        assert env.torch.equal(flat.scores(real["q"]).cpu().gather(1, I), D)
    return so.Case("ivf_search", lambda: (real, decoy), call, anchor=anchor, final=True)


@case("ivf_probe")
def _(env):
    ivf = _ivf_base(env)
    real, decoy = {"q": env.queries(D128, 1)}, {"q": env.queries(D128, 2)}

    def anchor(real, outs):
        s64 = _np(real["q"]).astype(np.float64) @ ivf.centroids.astype(np.float64).T
        S, L = _np(outs[0]), outs[1].cpu().numpy()
        assert np.abs(np.take_along_axis(s64, L, 1) - S).max() < 1e-3
        assert np.abs(np.sort(s64, 1)[:, ::-1][:, :NPROBE] - S).max() < 1e-3
    return so.Case("ivf_probe", lambda: (real, decoy), lambda st, b: ivf.probe(b["q"], NPROBE), anchor=anchor, final=True)


@case("ivf_add")
def _(env):
    real, decoy = {"x": env.queries(D128, 21, n=1000)}, {"x": env.queries(D128, 22, n=1000)}

    def call(st, b):
        st.add(b["x"])
        return st.reconstruct_n(), st.list_sizes()
    return so.Case("ivf_add", lambda: (real, decoy), call, setup=lambda: _ivf_fresh(env), cleanup=lambda st: st.close(),
                   final=True, anchor=lambda real, outs: np.testing.assert_array_equal(outs[0], _np(real["x"])))


@case("ivf_mmr")
def _(env):
    ivf, flat = _ivf_base(env), env.flat("f16", 40960)
    real, decoy = _mmr_inputs(env, 40960)

    def anchor(real, outs):   # bit for bit what the flat index of the same rows selects
        D, I = flat.mmr(real["ids"], real["rel"], K, 0.5)
        assert env.torch.equal(D, outs[0]) and env.torch.equal(I, outs[1])
    return so.Case("ivf_mmr", lambda: (real, decoy), lambda st, b: ivf.mmr(b["ids"], b["rel"], K, 0.5), anchor=anchor,
                   early=True)


@case("ivf_reset_add_search")
def _(env):
    real = {"x": env.queries(D128, 21, n=3000), "q": env.queries(D128, 1)}
    decoy = {"x": env.queries(D128, 22, n=3000), "q": env.queries(D128, 2)}

    def call(st, b):
        st.reset()                     # clears the device list sizes: the add that follows must find them cleared
        st.add(b["x"])
        D, I = env.sentinels(B)
        st.search(b["q"], K, out=(D, I))
        return D, I, st.list_sizes()

    def anchor(real, outs):
        assert int(outs[2].sum()) == 3000 and int(outs[1].max()) < 3000
    return so.Case("ivf_reset_add_search", lambda: (real, decoy), call, setup=lambda: _ivf_fresh(env, env.corpus_t(40960)[:5000]),
                   cleanup=lambda st: st.close(), anchor=anchor, final=True)


@case("ivf_reconstruct")
def _(env):
    ivf = _ivf_base(env)
    return so.Case("ivf_reconstruct", lambda: ({}, {}), lambda st, b: (ivf.reconstruct_n(100, 300),), final=True,
                   anchor=lambda real, outs: np.testing.assert_array_equal(outs[0], env.corpus(40960)[100:400]))


@case("ivf_centroids")
def _(env):
    torch = env.torch
    real = {"c": torch.from_numpy(make_corpus(NLIST, D128, seed=51, dtype="f32")).cuda()}
    decoy = {"c": torch.from_numpy(make_corpus(NLIST, D128, seed=52, dtype="f32")).cuda()}

    def call(st, b):
        st.set_centroids(b["c"])
        return (st.centroids,)
    return so.Case("ivf_centroids", lambda: (real, decoy), call, setup=lambda: _ivf_fresh(env, centroids=False),
                   cleanup=lambda st: st.close(), final=True,
                   anchor=lambda real, outs: np.testing.assert_allclose(outs[0], _np(real["c"]), atol=1e-6))


@case("ivf_train")
def _(env):
    real, decoy = {"x": env.queries(D128, 61, n=4096)}, {"x": env.queries(D128, 62, n=4096)}

    def call(st, b):
        st.train(b["x"], niter=2)
        return st.centroids, np.array(st.objective)

    def anchor(real, outs):
        assert np.abs(np.linalg.norm(outs[0].astype(np.float64), axis=1) - 1.0).max() < 1e-5
        assert outs[1].shape == (2,) and (outs[1] > 0.0).all()
    return so.Case("ivf_train", lambda: (real, decoy), call, setup=lambda: _ivf_fresh(env, centroids=False),
                   cleanup=lambda st: st.close(), anchor=anchor, final=True)


# ================================================================================================= stateless MaxSim
H, LQ, NDOC, MAXLEN = 128, 32, 64, 150


def _store(env):
    def build():
        torch = env.torch
        rng = np.random.default_rng(71)
        lens = rng.integers(1, MAXLEN + 1, size=NDOC)
        lens[:2] = (MAXLEN, 1)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        rows = int(lens.sum()) + MAXLEN                                  # max_len padding rows behind the last document
        mk = lambda seed, n: torch.from_numpy(oracle.quantize(
            np.random.default_rng(seed).standard_normal((n, H)).astype(np.float32), "bf16")).cuda().bfloat16()
        return {"lens": lens, "starts": starts, "store": (mk(72, rows), mk(73, rows)), "q": (mk(74, LQ), mk(75, LQ)),
                "starts_t": torch.from_numpy(starts.astype(np.int64)).cuda(),
                "lens_t": torch.from_numpy(lens.astype(np.int32)).cuda()}
    return env.memo("store", build)


def _docs(st, store_t, which):
    s = _np(store_t)
    return [s[st["starts"][i]: st["starts"][i] + st["lens"][i]] for i in which]


def _maxsim_case(env, name, fn, fp8=False, groups=((0, LQ, 0, NDOC),)):
    """groups: (q0, q1, c0, c1) per query of the call"""
    st = _store(env)
    conv = env.index.quantize_rows_fp8 if fp8 else (lambda t: t)
    real, decoy = ({"q": st["q"][i], "store": conv(st["store"][i])} for i in (0, 1))

    def anchor(real, outs):
        store = st["store"][0] if not fp8 else real["store"].float()
        for q0, q1, c0, c1 in groups:
            want = oracle.maxsim_scores(_np(real["q"])[q0:q1], _docs(st, store, range(c0, c1)))
            assert np.abs(_np(outs[0])[c0:c1] - want).max() < 1e-4
    return so.Case(name, lambda: (real, decoy), lambda s_, b: (fn(b),), anchor=anchor, early=True)


BATCH = ((0, 12, 0, 40), (12, LQ, 40, NDOC))
Q_OFF, C_OFF = [0, 12, LQ], [0, 40, NDOC]


@case("maxsim")
def _(env):
    st = _store(env)
    n = 20
    end = int(st["starts"][n - 1] + st["lens"][n - 1])
    off = env.torch.from_numpy(np.concatenate([st["starts"][:n], [end]]).astype(np.int32)).cuda()
    real, decoy = ({"q": st["q"][i], "docs": st["store"][i][:end].clone()} for i in (0, 1))

    def anchor(real, outs):
        assert np.abs(_np(outs[0]) - oracle.maxsim_scores(_np(real["q"]), _docs(st, st["store"][0], range(n)))).max() < 1e-4
    return so.Case("maxsim", lambda: (real, decoy), lambda s_, b: (env.index.maxsim(b["q"], b["docs"], off),), anchor=anchor,
                   early=True)


@case("maxsim_indexed")
def _(env):
    st = _store(env)
    return _maxsim_case(env, "maxsim_indexed", lambda b: env.index.maxsim_indexed(b["q"], b["store"], st["starts_t"], st["lens_t"]))


@case("maxsim_indexed_batch")
def _(env):
    st = _store(env)
    return _maxsim_case(env, "maxsim_indexed_batch", lambda b: env.index.maxsim_indexed_batch(
        b["q"], Q_OFF, b["store"], st["starts_t"], st["lens_t"], C_OFF), groups=BATCH)


@case("maxsim_indexed_fp8")
def _(env):
    st = _store(env)
    return _maxsim_case(env, "maxsim_indexed_fp8", lambda b: env.index.maxsim_indexed(b["q"], b["store"], st["starts_t"], st["lens_t"]),
                        fp8=True)


@case("maxsim_indexed_batch_fp8")
def _(env):
    st = _store(env)
    return _maxsim_case(env, "maxsim_indexed_batch_fp8", lambda b: env.index.maxsim_indexed_batch(
        b["q"], Q_OFF, b["store"], st["starts_t"], st["lens_t"], C_OFF), fp8=True, groups=BATCH)


@case("quantize_rows_fp8")
def _(env):
    torch, st = env.torch, _store(env)
    real, decoy = ({"x": st["store"][i]} for i in (0, 1))

    def anchor(real, outs):
        want = env.index.quantize_rows_fp8_reference(real["x"].cpu())
        assert torch.equal(outs[0].cpu().view(torch.uint8), want.view(torch.uint8))
    return so.Case("quantize_rows_fp8", lambda: (real, decoy), lambda s_, b: (env.index.quantize_rows_fp8(b["x"]),),
                   anchor=anchor, early=True)


def _passage_case(env, name, fn, groups):
    st = _store(env)
    real, decoy = ({"q": st["q"][i], "store": st["store"][i]} for i in (0, 1))

    def anchor(real, outs):
        o = [x.cpu().numpy() for x in outs]
        for q0, q1, c0, c1 in groups:
            docs = _docs(st, st["store"][0], range(c0, c1))
            for j, m in enumerate(pm.passages(_np(real["q"])[q0:q1], docs, 8)):
                i = c0 + j
                assert pm.passage_valid((o[0][i], o[1][i], o[2][i], o[3][i][: q1 - q0]), m, pm.TOL_16), (name, i)
    return so.Case(name, lambda: (real, decoy), lambda s_, b: fn(b), anchor=anchor, early=True)


@case("passages_indexed")
def _(env):
    st = _store(env)
    return _passage_case(env, "passages_indexed", lambda b: env.index.maxsim_passages_indexed(
        b["q"], b["store"], st["starts_t"], st["lens_t"], 8, align=True, max_len=MAXLEN), ((0, LQ, 0, NDOC),))


@case("passages_indexed_batch")
def _(env):
    st = _store(env)
    return _passage_case(env, "passages_indexed_batch", lambda b: env.index.maxsim_passages_indexed_batch(
        b["q"], Q_OFF, b["store"], st["starts_t"], st["lens_t"], C_OFF, 8, align=True, max_len=MAXLEN), BATCH)


# =============================================================================================================== BM25
def _bm25(env):
    def build():
        rng = np.random.default_rng(81)
        N, V = 200, 40
        post = []
        for t in range(V):
            d = np.sort(rng.choice(N, size=int(rng.integers(5, 120)), replace=False))
            post.append((d, rng.integers(1, 6, size=len(d)).astype(np.float32)))
        ix = bm.from_postings(N, post, rng.random(V) + 0.1, len_norm=rng.random(N) + 0.5)
        queries = [list(rng.choice(V, size=int(n), replace=False)) for n in (1, 3, 5, 8, 2)]
        return ix, _bm25_handle(env, ix), queries
    return env.memo("bm25", build)


def _bm25_handle(env, ix):
    h = ctypes.c_void_p()
    env._lib.check(env.lib.ts_bm25_create(0, ctypes.byref(h)))
    env._lib.check(env.lib.ts_bm25_set_index(h, ix.N, ix.V, ix.nnz, ix.term_off.ctypes.data, ix.post_doc.ctypes.data,
                                             ix.post_tf.ctypes.data, ix.idf.ctypes.data, ix.len_norm.ctypes.data, ix.k1p1))
    return h


def _bm25_outs(nq, k):
    return np.full((nq, k), np.nan), np.full((nq, k), -7, dtype=np.int64), np.full(nq, -1, dtype=np.int32)


def _bm25_check(ix, queries, k, s, i, n, allowed=None):
    for q, terms in enumerate(queries):
        wi, ws, wn = bm.search(ix, terms, k, allowed)
        assert n[q] == wn and np.array_equal(i[q, :wn], wi) and np.array_equal(s[q, :wn].view(np.uint64), ws.view(np.uint64))


@case("bm25_search")
def _(env):
    ix, h, queries = _bm25(env)
    k = 20
    flat = np.array([t for q in queries for t in q], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)

    def call(st, b):
        s1, i1, _ = _bm25_outs(1, k)
        n1 = ctypes.c_int32(-1)
        t = np.array(queries[2], dtype=np.int32)
        env._lib.check(env.lib.ts_bm25_search(h, t.ctypes.data, len(t), k, s1.ctypes.data, i1.ctypes.data, ctypes.byref(n1), env.sp()))
        s, i, n = _bm25_outs(len(queries), k)
        env._lib.check(env.lib.ts_bm25_search_batch(h, flat.ctypes.data, off.ctypes.data, len(queries), k, s.ctypes.data,
                                                    i.ctypes.data, n.ctypes.data, env.sp()))
        return s1, i1, np.array([n1.value], dtype=np.int32), s, i, n

    def anchor(real, outs):
        _bm25_check(ix, [queries[2]], k, *outs[:3])
        _bm25_check(ix, queries, k, *outs[3:])
    return so.Case("bm25_search", lambda: ({}, {}), call, anchor=anchor, final=True)


@case("bm25_first_batch_on_side_stream")
def _(env):
    """A fresh handle per invocation: its first batch, which grows the handle from one lane to five and zeroes the new
    accumulators and counters, is made on the stream under test (a handle shared by the module would have grown on
    the default stream when the expected value was computed).  The mask arrives late."""
    torch = env.torch
    ix, _, queries = _bm25(env)
    k = 20
    flat = np.array([t for q in queries for t in q], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)
    rng = np.random.default_rng(83)
    masks = [rng.random(ix.N) < 0.5 for _ in range(2)]
    words = (ix.N + 31) // 32
    real, decoy = ({"bits": torch.from_numpy(env.index.pack_allowed(m, ix.N).view(np.int32)).cuda()} for m in masks)
    moq = np.array([0, -1, 0, -1, 0], dtype=np.int32)

    def call(st, b):
        s, i, n = _bm25_outs(len(queries), k)
        env._lib.check(env.lib.ts_bm25_search_batch(st, flat.ctypes.data, off.ctypes.data, len(queries), k, s.ctypes.data,
                                                    i.ctypes.data, n.ctypes.data, env.sp()))
        fs, fi, fn = _bm25_outs(len(queries), k)
        env._lib.check(env.lib.ts_bm25_search_batch_filtered(
            st, flat.ctypes.data, off.ctypes.data, len(queries), k, ctypes.c_void_p(b["bits"].data_ptr()), words, 1,
            moq.ctypes.data, 0, fs.ctypes.data, fi.ctypes.data, fn.ctypes.data, env.sp()))
        return s, i, n, fs, fi, fn

    def anchor(real, outs):
        _bm25_check(ix, queries, k, *outs[:3])
        for q in range(len(queries)):
            _bm25_check(ix, [queries[q]], k, outs[3][q:q + 1], outs[4][q:q + 1], outs[5][q:q + 1],
                        allowed=masks[0] if moq[q] == 0 else None)
    return so.Case("bm25_first_batch_on_side_stream", lambda: (real, decoy), call, setup=lambda: _bm25_handle(env, ix),
                   cleanup=lambda st: env.lib.ts_bm25_destroy(st), anchor=anchor, final=True)


@case("bm25_filtered")
def _(env):
    torch = env.torch
    ix, h, queries = _bm25(env)
    k = 20
    flat = np.array([t for q in queries for t in q], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)
    rng = np.random.default_rng(82)
    masks = [rng.random(ix.N) < 0.5 for _ in range(2)]
    words = (ix.N + 31) // 32
    real, decoy = ({"bits": torch.from_numpy(env.index.pack_allowed(m, ix.N).view(np.int32)).cuda()} for m in masks)
    moq = np.zeros(len(queries), dtype=np.int32)

    def call(st, b):
        s, i, n = _bm25_outs(len(queries), k)
        env._lib.check(env.lib.ts_bm25_search_batch_filtered(
            h, flat.ctypes.data, off.ctypes.data, len(queries), k, ctypes.c_void_p(b["bits"].data_ptr()), words, 1,
            moq.ctypes.data, 0, s.ctypes.data, i.ctypes.data, n.ctypes.data, env.sp()))
        return s, i, n
    return so.Case("bm25_filtered", lambda: (real, decoy), call, final=True,
                   anchor=lambda real, outs: _bm25_check(ix, queries, k, *outs, allowed=masks[0]))


# =================================================================================================== encoder kernels
ROWS = 37


def _g(env, seed):
    return env.torch.Generator(device="cuda").manual_seed(seed)


def _randn(env, shape, seed, dtype=None, scale=1.0):
    t = env.torch.randn(shape, generator=_g(env, seed), device="cuda") * scale
    return t.to(dtype).contiguous() if dtype is not None else t.contiguous()


def _ln_case(env, name, prenorm):
    import encoder_ref as er
    torch = env.torch
    real, decoy = ({"x": _randn(env, (ROWS, 128), 100 + s, torch.float16), "res": _randn(env, (ROWS, 128), 110 + s),
                    "gamma": _randn(env, (128,), 120 + s) + 1.0, "beta": _randn(env, (128,), 130 + s)} for s in (0, 1))

    def anchor(real, outs):
        r32, rln = er.add_layernorm_ref(real["x"], real["res"], real["gamma"], real["beta"], 1e-12, prenorm=prenorm)
        er.check32("stream_" + name, outs[0], r32)
        er.check16("stream_" + name + "_lp", outs[1], er.to16(rln, torch.bfloat16))
    return so.Case(name, lambda: (real, decoy), lambda st, b: env.index.add_layernorm(
        b["x"], b["res"], b["gamma"], b["beta"], 1e-12, lp_dtype=torch.bfloat16, prenorm=prenorm), anchor=anchor, early=True)


@case("add_layernorm")
def _(env):
    return _ln_case(env, "add_layernorm", False)


@case("add_prenorm")
def _(env):
    return _ln_case(env, "add_prenorm", True)


@case("embed_layernorm")
def _(env):
    import encoder_ref as er
    torch = env.torch
    word, pos, typ = _randn(env, (50, 128), 140), _randn(env, (40, 128), 141), _randn(env, (2, 128), 142)
    gamma, beta = _randn(env, (128,), 143) + 1.0, _randn(env, (128,), 144)
    ri = lambda hi, seed: torch.randint(0, hi, (ROWS,), generator=_g(env, seed), device="cuda")
    real, decoy = ({"ids": ri(50, 150 + s), "pos": ri(40, 152 + s), "tt": ri(2, 154 + s)} for s in (0, 1))

    def anchor(real, outs):
        ref = er.embed_layernorm_ref(real["ids"], real["pos"], real["tt"], word, pos, typ, gamma, beta, 1e-12)
        er.check32("stream_embed_layernorm", outs[0], ref)
        er.check16("stream_embed_layernorm_lp", outs[1], er.to16(ref, torch.float16))
    return so.Case("embed_layernorm", lambda: (real, decoy), lambda st, b: env.index.embed_layernorm(
        b["ids"], b["pos"], b["tt"], word, pos, typ, gamma, beta, 1e-12, lp_dtype=torch.float16), anchor=anchor, early=True)


AB, AL, AH, ADH = 2, 40, 2, 32


def _rope_tables(env):
    torch = env.torch
    ang = torch.arange(AL, device="cuda", dtype=torch.float32)[:, None] * torch.exp(
        -torch.arange(ADH, device="cuda", dtype=torch.float32) / ADH)[None, :]
    return torch.cos(ang).contiguous(), torch.sin(ang).contiguous()


@case("rope_inplace")
def _(env):
    import encoder_ref as er
    torch = env.torch
    cos, sin = _rope_tables(env)
    real, decoy = ({"qkv": _randn(env, (AB, AL, 3 * AH * ADH), 160 + s, torch.float16)} for s in (0, 1))

    def anchor(real, outs):
        src, out = real["qkv"].view(AB, AL, 3, AH, ADH), outs[0].view(AB, AL, 3, AH, ADH)
        for which in (0, 1):
            er.check16("stream_rope", out[:, :, which].transpose(1, 2), er.rope_ref(src[:, :, which].transpose(1, 2), cos, sin, torch.float16))
        assert torch.equal(out[:, :, 2], src[:, :, 2])
    return so.Case("rope_inplace", lambda: (real, decoy), lambda st, b: (env.index.rope_inplace(b["qkv"], cos, sin, AH),),
                   anchor=anchor, early=True)


@case("geglu")
def _(env):
    import encoder_ref as er
    torch = env.torch
    real, decoy = ({"u": _randn(env, (ROWS, 128), 170 + s, torch.float16, 2.5)} for s in (0, 1))
    return so.Case("geglu", lambda: (real, decoy), lambda st, b: (env.index.geglu(b["u"]),), early=True,
                   anchor=lambda real, outs: er.check16("stream_geglu", outs[0], er.geglu_ref(real["u"], torch.float16)))


@case("attention_varlen")
def _(env):
    import encoder_ref as er
    torch = env.torch
    lens = torch.tensor([AL, 17], dtype=torch.int32, device="cuda")                 # lengths are not decoyed
    real, decoy = ({"qkv": _randn(env, (AB, AL, 3 * AH * ADH), 180 + s, torch.float16)} for s in (0, 1))

    def anchor(real, outs):
        q, k, v = (real["qkv"].view(AB, AL, 3, AH, ADH)[:, :, i].transpose(1, 2) for i in range(3))
        ref = er.attention_ref(q, k, v, lens, ADH ** -0.5, torch.float16, window=0)
        valid = torch.arange(AL, device="cuda")[None, :] < lens[:, None]
        er.check16("stream_attention", outs[0].view(AB, AL, AH, ADH).transpose(1, 2), ref,
                   where=valid[:, None, :, None].expand(AB, AH, AL, ADH))
    return so.Case("attention_varlen", lambda: (real, decoy), lambda st, b: (env.index.attention_varlen(b["qkv"], lens, AH),),
                   anchor=anchor, early=True)


@case("linear_tile_weight")
def _(env):
    import encoder_ref as er
    torch = env.torch
    real, decoy = ({"w": _randn(env, (32, 128), 190 + s, torch.float16, 0.1)} for s in (0, 1))
    x = _randn(env, (ROWS, 128), 192, torch.float16)
    keep = []

    def call(st, b):
        keep.append(env.index.TiledLinear(b["w"]))      # (the smallest shape usable() accepts)
        return (keep[-1].tiled,)

    def anchor(real, outs):
        lin = env.index.TiledLinear(real["w"])
        assert torch.equal(lin.tiled, outs[0])
        er.check16("stream_tile_weight", lin(x), er.linear_ref(er.exact16(x), real["w"], None, torch.float16))
    return so.Case("linear_tile_weight", lambda: (real, decoy), call, anchor=anchor, early=True)


@case("linear_act")
def _(env):
    import encoder_ref as er
    torch = env.torch
    w, bias = _randn(env, (32, 128), 200, torch.float16, 0.1), _randn(env, (32,), 201, torch.float16)
    lin = env.index.TiledLinear(w, bias)
    real, decoy = ({"x": _randn(env, (ROWS, 128), 202 + s, torch.float16)} for s in (0, 1))
    return so.Case("linear_act", lambda: (real, decoy), lambda st, b: (lin(b["x"], gelu=True),), early=True,
                   anchor=lambda real, outs: er.check16("stream_linear_act", outs[0],
                                                        er.linear_gelu_ref(er.exact16(real["x"]), w, bias, torch.float16)))


@case("linear_add_layernorm")
def _(env):
    import encoder_ref as er
    torch = env.torch
    w, bias = _randn(env, (32, 384), 210, torch.float16, 0.05), _randn(env, (32,), 211, torch.float16)
    gamma, beta = _randn(env, (32,), 212) + 1.0, _randn(env, (32,), 213)
    lin = env.index.TiledLinear(w, bias, with_layernorm=True)
    real, decoy = ({"x": _randn(env, (ROWS, 384), 214 + s, torch.float16), "res": _randn(env, (ROWS, 32), 216 + s)} for s in (0, 1))

    def anchor(real, outs):
        ref = er.proj_ln_ref(real["x"], w, bias, real["res"], gamma, beta, 1e-12, torch.float16)
        er.check32("stream_proj_ln", outs[0], ref)
        er.check16("stream_proj_ln_lp", outs[1], er.to16(ref, torch.float16))
    return so.Case("linear_add_layernorm", lambda: (real, decoy),
                   lambda st, b: lin.add_layernorm(b["x"], b["res"], gamma, beta, 1e-12), anchor=anchor, early=True)


@case("mlp_add_layernorm")
def _(env):
    import encoder_ref as er
    torch = env.torch
    w1, b1 = _randn(env, (384, 384), 220, torch.float16, 0.05), _randn(env, (384,), 221, torch.float16)
    w2, b2 = _randn(env, (384, 384), 222, torch.float16, 0.05), _randn(env, (384,), 223, torch.float16)
    gamma, beta = _randn(env, (384,), 224) + 1.0, _randn(env, (384,), 225)
    up, down = env.index.TiledLinear(w1, b1), env.index.TiledLinear(w2, b2, with_layernorm=True)
    real, decoy = ({"x": _randn(env, (ROWS, 384), 226 + s, torch.float16), "res": _randn(env, (ROWS, 384), 228 + s)} for s in (0, 1))

    def anchor(real, outs):
        ref = er.mlp_ref(real["x"], w1, b1, w2, b2, real["res"], gamma, beta, 1e-12, torch.float16)
        er.check32("stream_mlp", outs[0], ref)
        er.check16("stream_mlp_lp", outs[1], er.to16(ref, torch.float16))
    return so.Case("mlp_add_layernorm", lambda: (real, decoy),
                   lambda st, b: env.index.mlp_add_layernorm(up, down, b["x"], b["res"], gamma, beta, 1e-12), anchor=anchor,
                   early=True)


# ===================================================================================================== the table rows
@pytest.mark.parametrize("name", sorted(CASES))
def test_case(env, name):
    t0 = time.perf_counter()
    fails = env.h.run(CASES[name](env))
    env.seconds[name] = time.perf_counter() - t0
    if name in env.h.enqueue_ms:
        print(f"{name}: the enqueue took {env.h.enqueue_ms[name]:.3f} ms on the host, the delay is {env.h.delay_measured_ms:.1f} ms")
    assert fails == [], f"{name}: " + "; ".join(fails)


def test_every_table_row_names_a_case_of_this_module():
    names = set(CASES) | {"order_" + v for v in ORDER_VARIANTS} | {"flat_remove_compact", "ivf_mutations_A", "ivf_mutations_B"}
    assert so.table_problems(case_names=names) == []


# ================================================================== two side streams at once: per-stream MaxSim scratch
def test_maxsim_on_two_streams_at_once(env):
    """The same MaxSim call on two side streams at once, each behind its own delay, with other candidates and another
    query: the scratch kept per (device, stream) must keep the two apart."""
    torch, st = env.torch, _store(env)
    sets = [np.arange(0, 40), np.arange(24, NDOC)]
    args = [(st["q"][i], torch.from_numpy(st["starts"][s].astype(np.int64)).cuda(),
             torch.from_numpy(st["lens"][s].astype(np.int32)).cuda()) for i, s in enumerate(sets)]
    store = st["store"][0]
    run = lambda q, a: env.index.maxsim_indexed(q, store, a[1], a[2])
    want = [run(a[0], a) for a in args]
    torch.cuda.synchronize()
    assert not torch.equal(want[0], want[1])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [args[1 - i][0].clone() for i in range(2)]          # each starts with the other stream's query as its decoy
    torch.cuda.synchronize()
    outs = [None, None]
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            run(bufs[i], args[i])                              # this stream's scratch exists before anything is timed
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            env.h.delay()
            bufs[i].copy_(args[i][0], non_blocking=True)
            o = run(bufs[i], args[i])
            outs[i] = (o, o.clone())
    for s in streams:
        s.synchronize()
    for i in range(2):
        assert torch.equal(outs[i][0], want[i]) and torch.equal(outs[i][1], want[i]), f"stream {i}"


# ===================================================== remove and update ordered behind earlier searches (any stream)
ORDER_VARIANTS = ["update_dense_A", "update_dense_B", "remove_dense_A", "remove_dense_B", "remove_coalesced_A",
                  "remove_coalesced_B"]
F_ASYNC, F_CLASSIC, F_COALESCE, F_NO_WIDE = 8, 32, 128, 512


def _raw_search(env, idx, q, D, I, flags, stream):
    env._lib.check(env.lib.ts_index_search(idx._h, ctypes.c_void_p(q.data_ptr()), q.shape[0], env._lib.TS_F16, K,
                                           ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(I.data_ptr()), flags,
                                           ctypes.c_void_p(int(stream.cuda_stream))))


def _raw_finish(env, idx, stream):
    failed, nf = (ctypes.c_int64 * 256)(), ctypes.c_int32(0)
    env._lib.check(env.lib.ts_index_finish(idx._h, ctypes.c_void_p(int(stream.cuda_stream)), failed, 256, ctypes.byref(nf)))
    return nf.value


@pytest.mark.parametrize("variant", ["update_dense_A", "update_dense_B", "remove_dense_A", "remove_dense_B", "remove_coalesced_A", "remove_coalesced_B"])
def test_order(env, variant):
    """TS_FLAG_ASYNC searches wait behind a delay on stream A; then ts_index_remove / ts_index_update is called on A or
    on a second non-blocking stream B.  The searches return what the index held before, a search submitted afterwards
    what it holds then.  Expected values: fresh indexes built the old and the new way, searched with nothing else in
    flight.  dense: 4096 rows, plain asynchronous searches (with tombstones: the filtered form, ordered by the event behind
    its effective masks).  coalesced: 40960 rows with tombstones, four batches of 32 sharing one pass of the five-launch
    path, which reads the live bitmap itself: the removal is ordered behind it by the queue's event, which the flush at
    the head of ts_index_remove waits for, as well as by the per-workspace events.  (So the wait for the per-workspace
    events in ts_index_remove is backed up on every path and no variant here depends on it alone; ts_index_update does:
    update_dense_B fails without it.)"""
    torch = env.torch
    what, path, where = variant.split("_")
    n = 4096 if path == "dense" else 40960
    nb, bq = (3, B) if path == "dense" else (4, 32)
    flags = F_ASYNC if path == "dense" else F_ASYNC | F_COALESCE | F_CLASSIC | F_NO_WIDE
    rows = env.corpus_t(n)
    q = env.queries(D128, 1, n=nb * bq)
    q_after = env.queries(D128, 3)
    first = np.arange(5, n, 97, dtype=np.int64)                  # the removal made before everything (remove variants)
    probe = env.flat("f16", n)
    top = np.unique(probe.search(q, 2)[1].cpu().numpy())         # the rows the mutation takes from the searches' results
    top = top[~np.isin(top, first)]
    new_rows = env.queries(D128, 90, n=len(top))

    def build(mutated):
        idx = env.index.FlatIPIndex(D128, dtype="f16")
        idx.add(rows)
        if what == "remove":
            assert idx.remove_ids(first) == len(first)
        if mutated:
            idx.remove_ids(top) if what == "remove" else idx.update_rows(top, new_rows)
        return idx

    def searches(idx, stream, outs):
        for i in range(nb):
            _raw_search(env, idx, q[i * bq:(i + 1) * bq], outs[i][0], outs[i][1], flags, stream)

    def fresh_outs():
        return [env.sentinels(bq) for _ in range(nb)]

    # the old and the new way, each alone
    dflt = torch.cuda.current_stream()
    old, new = build(False), build(True)
    want_old = fresh_outs()
    searches(old, dflt, want_old)
    assert _raw_finish(env, old, dflt) == 0
    want_new = env.sentinels(B)
    _raw_search(env, new, q_after, *want_new, 0, dflt)
    seen_new = fresh_outs()
    searches(new, dflt, seen_new)
    assert _raw_finish(env, new, dflt) == 0
    torch.cuda.synchronize()
    assert not any(torch.equal(a[1], b[1]) for a, b in zip(want_old, seen_new))   # the mutation changes every batch
    old.close(), new.close()

    idx = build(False)
    A, Bs = torch.cuda.Stream(), torch.cuda.Stream()
    warm = fresh_outs()
    searches(idx, A, warm)                                       # workspaces, streams and events exist before the run
    assert _raw_finish(env, idx, A) == 0
    got, got_after = fresh_outs(), env.sentinels(B)
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        env.h.delay()
        pending = torch.cuda.Event()
        pending.record(A)
    searches(idx, A, got)
    assert not pending.query()                                   # the searches are unfinished when the mutation is made
    M = A if where == "A" else Bs
    sp = ctypes.c_void_p(int(M.cuda_stream))
    if what == "remove":
        nrem = ctypes.c_int64(0)
        env._lib.check(env.lib.ts_index_remove(idx._h, top.ctypes.data_as(ctypes.c_void_p), len(top), ctypes.byref(nrem), sp))
        assert nrem.value == len(top)
    else:
        env._lib.check(env.lib.ts_index_update(idx._h, top.ctypes.data_as(ctypes.c_void_p), len(top),
                                               ctypes.c_void_p(new_rows.data_ptr()), env._lib.TS_F16, 0, sp))
    _raw_search(env, idx, q_after, *got_after, 0, M)
    assert _raw_finish(env, idx, A) == 0
    torch.cuda.synchronize()
    for i in range(nb):
        assert torch.equal(got[i][1], want_old[i][1]) and torch.equal(got[i][0], want_old[i][0]), \
            f"batch {i} submitted before the {what} does not show the index as it was"
    assert torch.equal(got_after[1], want_new[1]) and torch.equal(got_after[0], want_new[0])
    idx.close()


def test_flat_remove_compact(env):
    """ts_index_remove, ts_index_live_words and ts_index_compact on a side stream: final at return."""
    torch, n = env.torch, 4096
    ids = np.arange(3, n, 7, dtype=np.int64)
    ref = env.index.FlatIPIndex(D128, dtype="f16")
    ref.add(env.corpus_t(n))
    ref.remove_ids(ids)
    want_words = ref.live_words()
    want_map = ref.compact()
    want_rows = ref.reconstruct_n()
    torch.cuda.synchronize()
    idx = env.index.FlatIPIndex(D128, dtype="f16")
    idx.add(env.corpus_t(n))
    torch.cuda.synchronize()
    with torch.cuda.stream(env.h.S):
        env.h.delay()
        sp = env.sp()
        nrem = ctypes.c_int64(0)
        env._lib.check(env.lib.ts_index_remove(idx._h, ids.ctypes.data_as(ctypes.c_void_p), len(ids), ctypes.byref(nrem), sp))
        words = np.zeros((n + 31) // 32, dtype=np.uint32)
        env._lib.check(env.lib.ts_index_live_words(idx._h, words.ctypes.data_as(ctypes.c_void_p), sp))
        assert nrem.value == len(ids) and np.array_equal(words, want_words)
        o2n = np.full(n, -9, dtype=np.int64)
        env._lib.check(env.lib.ts_index_compact(idx._h, o2n.ctypes.data_as(ctypes.c_void_p), sp))
        assert np.array_equal(o2n, want_map)
    with torch.cuda.stream(env.h.S2):                            # a stream that waits for nothing reads the rows
        out = torch.full((idx.ntotal, D128), so.SENT_F, dtype=torch.float32, device="cuda")
        env._lib.check(env.lib.ts_index_reconstruct(idx._h, 0, idx.ntotal, ctypes.c_void_p(out.data_ptr()), 0, env.sp()))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want_rows) and np.array_equal(want_rows, env.corpus(n)[want_map >= 0])
    ref.close(), idx.close()


@pytest.mark.parametrize("variant", ["A", "B"])
def test_ivf_mutations(env, variant):
    """ts_remove_ivf, ts_update_ivf and ts_compact_ivf behind searches on stream A, once on A itself and once on a second
    non-blocking stream B (IVF searches are synchronous, so nothing of them is pending): every search shows the index
    as it is when it is submitted; the new rows of the update arrive late.  Expected values: fresh indexes with the
    same centroids."""
    torch = env.torch
    rows = env.corpus_t(40960)[:8192]
    q = env.queries(D128, 1)
    ids_rm = np.arange(1, 8192, 5, dtype=np.int64)
    ids_up = np.arange(2, 8192, 11, dtype=np.int64)
    ids_up = ids_up[~np.isin(ids_up, ids_rm)]
    new_rows, decoy_rows = env.queries(D128, 91, n=len(ids_up)), env.queries(D128, 92, n=len(ids_up))

    ref = _ivf_fresh(env, rows)
    want = [ref.search(q, K)]
    ref.remove_ids(ids_rm)
    want.append(ref.search(q, K))
    ref.update_rows(ids_up, new_rows)
    want.append(ref.search(q, K))
    want_map = ref.compact()
    want.append(ref.search(q, K))
    torch.cuda.synchronize()
    assert not torch.equal(want[0][1], want[1][1]) and not torch.equal(want[1][1], want[2][1])

    ivf = _ivf_fresh(env, rows)
    A = torch.cuda.Stream()
    Bs = A if variant == "A" else torch.cuda.Stream()
    buf = decoy_rows.clone()
    got = []
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        env.h.delay()
        got.append(ivf.search(q, K))
    with torch.cuda.stream(Bs):
        assert ivf.remove_ids(ids_rm) == len(ids_rm)
        got.append(ivf.search(q, K))
        env.h.delay()
        buf.copy_(new_rows, non_blocking=True)
        ivf.update_rows(ids_up, buf)
    with torch.cuda.stream(A):
        got.append(ivf.search(q, K))
    with torch.cuda.stream(Bs):
        assert np.array_equal(ivf.compact(), want_map)
    with torch.cuda.stream(A):
        got.append(ivf.search(q, K))
    torch.cuda.synchronize()
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]), f"search {i}"
    ref.close(), ivf.close()
