"""Stage-1 scans against exact results ("exact inputs"): on inputs whose every product and partial sum
is an fp32 number (tests/exact_inputs.py) each scan family must return the float64 scores and the canonical ids bit
for bit — `np.array_equal`, no tolerance — and the intended kernel must have run.  The exceptions are the accuracy of
the bf16x3 split on unit-norm rows (a bound derived from the numpy model of the split, test_exact_scores_host.py) and
the power-of-two scale invariance of every path."""
import functools

import numpy as np
import pytest

import exact_inputs as ex
from helpers import make_corpus
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _t(x, dtype):
    import torch
    dt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[dtype]
    return torch.tensor(np.asarray(x), device="cuda").to(dt)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


@functools.lru_cache(maxsize=4)
def _case(cls, n, d, B):
    """The class's inputs, guarded: nothing reaches the GPU that is not exactly summable."""
    corpus, queries, unit = ex.case(cls, n, d, B)
    ex.assert_exactly_summable(corpus, queries, unit)
    return corpus, queries


def _one_launch_rows(torch):
    return ex.one_launch_rows(torch.cuda.get_device_properties(0).multi_processor_count)


def _flat(d, dtype, corpus):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_t(corpus, dtype))
    return idx


def _exact(got, want, what=""):
    D, I = _np(got[0]), _np(got[1])
    D0, I0 = want
    assert D.shape == D0.shape and I.shape == I0.shape, what
    bad = np.argwhere(I != I0)
    assert bad.size == 0, f"{what}: ids differ first at {bad[0].tolist()}: got {I[tuple(bad[0])]} want {I0[tuple(bad[0])]}"
    bad = np.argwhere(D != D0)
    assert bad.size == 0, f"{what}: scores differ first at {bad[0].tolist()}: got {D[tuple(bad[0])]!r} want {D0[tuple(bad[0])]!r}"
    assert np.array_equal(I, I0) and np.array_equal(D, D0)


def _is_split(dtype, d):
    return dtype == "f32" and 512 < d <= 768


def _coalesced(torch, idx, batches, k, wide):
    """The batches as held asynchronous searches that share corpus passes; (results, scan launches)."""
    idx.classic_filter, idx.coalesce, idx.wide_passes = True, True, wide
    idx.set_profiling(True, every=1)
    idx.timings(reset=True)
    outs = [idx.search(q, k, async_=True) for q in batches]
    redone = idx.finish()
    torch.cuda.synchronize()
    launches = idx.timings(reset=True)["filter_scan"][1]
    idx.set_profiling(False)
    assert redone == []
    return outs, launches


# ------------------------------------------------------------------------------------------ 3a: every scan family
@pytest.mark.parametrize("cls", ["ints", "neg"])
@pytest.mark.parametrize("dtype,d", [(dt, d) for dt in ex.DENSE_D for d in ex.DENSE_D[dt]])
def test_dense_scan_is_exact(torch_mod, dtype, d, cls):
    """scan_kernel DENSE (f16 / bf16; the exact-f32 MFMA and, for 512 < d <= 768, scan_f32s_kernel for f32): the whole
    score matrix and the searches of one, two and three passes, k = 1, 100 and beyond n."""
    n, kmax = ex.N_DENSE, max(ex.DENSE_K)
    corpus, queries = _case(cls, n, d, max(ex.DENSE_B))
    idx = _flat(d, dtype, corpus)
    tq = _t(queries, dtype)
    S = _np(idx.scores(tq))
    want_S = ex.exact_scores(corpus, queries).astype(np.float32)
    assert S.shape == want_S.shape and np.array_equal(S, want_S)
    want = ex.expected_topk(corpus, queries, kmax)
    for B in ex.DENSE_B:
        for k in ex.DENSE_K:
            got = idx.search(tq[:B], k)
            assert idx.last_search_info()["path"] == "dense"
            wD, wI = want[0][:B, :k].copy(), want[1][:B, :k].copy()
            _exact(got, (wD, wI), f"B={B} k={k}")
            if k > n:
                assert (_np(got[1])[:, n:] == -1).all() and (_np(got[0])[:, n:] == -ex.FLT_MAX).all()
    _exact(idx.search(queries, 100), (want[0][:, :100], want[1][:, :100]), "host float32 queries")
    idx.close()


@pytest.mark.parametrize("cls", ["ints", "neg"])
@pytest.mark.parametrize("mode", ["classic", "one_launch"])
@pytest.mark.parametrize("dtype,d,B", ex.FILTER_CASES)
def test_filter_scans_are_exact(torch_mod, dtype, d, B, mode, cls):
    """The five-launch filter path at the smallest corpus it takes, and the one-launch scan at the smallest it takes
    (one row block per scan wave).  fp32 storage with 512 < d <= 768 has no one-launch form: asked for it, the split
    scan runs on five launches."""
    n = ex.N_FILTER if mode == "classic" else _one_launch_rows(torch_mod)
    corpus, queries = _case(cls, n, d, B)
    idx = _flat(d, dtype, corpus)
    tq = _t(queries, dtype)
    want = ex.expected_topk(corpus, queries, max(ex.FILTER_K))
    for k in ex.FILTER_K:
        got = idx.search(tq, k, classic=mode == "classic", one_launch=mode == "one_launch")
        info = idx.last_search_info()
        assert info["path"] == "filter", info            # no dense fallback
        assert info["one_launch"] == (mode == "one_launch" and not _is_split(dtype, d)), info
        _exact(got, (want[0][:, :k], want[1][:, :k]), f"k={k}")
    idx.close()


@pytest.mark.parametrize("cls", ["ints", "neg"])
def test_masked_scan_is_exact(torch_mod, cls):
    """The masked scan (scan_kernel over WalkLive): two random half masks and one unfiltered query in the same pass."""
    n, d, B = ex.N_FILTER, 768, 64
    corpus, queries = _case(cls, n, d, B)
    rng = np.random.default_rng(11)
    m0, m1 = rng.random(n) < 0.5, rng.random(n) < 0.5
    masks = [None if b == 5 else (m0 if b % 2 else m1) for b in range(B)]
    idx = _flat(d, "f16", corpus)
    tq = _t(queries, "f16")
    for k in (1, 100):
        got = idx.search(tq, k, allowed=masks)
        assert idx.last_search_info()["path"] == "filter"
        info = idx.last_filter_info()
        assert info["filter_passes"] == 1 and info["dense_passes"] == 0, info
        _exact(got, ex.expected_topk(corpus, queries, k, allowed=masks), f"k={k}")
    idx.close()


@pytest.mark.parametrize("cls", ["ints", "neg"])
def test_tombstone_scans_are_exact(torch_mod, cls):
    """Every third row removed: the synchronous search (the tombstone bitmap as the only mask) and the coalesced
    asynchronous passes in their tombstone form, LDS-resident and wide."""
    torch = torch_mod
    n, d = ex.N_FILTER, 768
    corpus, queries = _case(cls, n, d, ex.COALESCE_BATCHES * ex.COALESCE_B)
    queries = queries[: 3 * ex.COALESCE_B]
    idx = _flat(d, "f16", corpus)
    gone = np.arange(0, n, 3)
    assert idx.remove_ids(gone) == gone.size
    live = np.ones(n, bool)
    live[gone] = False
    tq = _t(queries, "f16")
    want = ex.expected_topk(corpus, queries, 100, live=live)
    for k in (1, 100):
        got = idx.search(tq[:64], k)
        assert idx.last_search_info()["path"] == "filter"
        _exact(got, (want[0][:64, :k], want[1][:64, :k]), f"sync k={k}")
    batches = [tq[i * 64: (i + 1) * 64] for i in range(3)]      # six groups of 32
    for wide, launches in ((False, 2), (True, 1)):
        outs, n_scan = _coalesced(torch, idx, batches, 100, wide)
        assert n_scan == launches
        assert idx.last_search_info()["path"] == "filter"
        for i, got in enumerate(outs):
            _exact(got, (want[0][i * 64: (i + 1) * 64], want[1][i * 64: (i + 1) * 64]), f"wide={wide} batch {i}")
    idx.close()


@pytest.mark.parametrize("cls", ["ints", "neg"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_coalesced_scans_are_exact(torch_mod, dtype, cls):
    """scan_multi_kernel (three groups per LDS-resident pass at d = 768) and the forced scan_wide_kernel (six): seven
    batches of 64 are fourteen groups, i.e. full passes and a partial one at finish()."""
    torch = torch_mod
    n, d = ex.N_FILTER, 768
    corpus, queries = _case(cls, n, d, ex.COALESCE_BATCHES * ex.COALESCE_B)
    idx = _flat(d, dtype, corpus)
    tq = _t(queries, dtype)
    batches = [tq[i * 64: (i + 1) * 64] for i in range(ex.COALESCE_BATCHES)]
    want = ex.expected_topk(corpus, queries, 100)
    for wide, launches in ((False, 5), (True, 3)):
        outs, n_scan = _coalesced(torch, idx, batches, 100, wide)
        assert n_scan == launches                           # ceil(14 / 3) resident passes, ceil(14 / 6) wide ones
        assert idx.last_search_info()["path"] == "filter"
        for i, got in enumerate(outs):
            _exact(got, (want[0][i * 64: (i + 1) * 64], want[1][i * 64: (i + 1) * 64]), f"wide={wide} batch {i}")
    idx.close()


@pytest.mark.parametrize("cls", ["ints", "neg"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", ex.IVF_D)
@pytest.mark.parametrize("n", [ex.N_IVF, ex.N_FILTER])
def test_ivf_scans_are_exact(torch_mod, n, d, dtype, cls):
    """Every list probed, so the result is the flat one.  5000 rows stay on the IVF index's dense path (below 32768
    slots); scan_ivf_kernel runs from 32768 slots on."""
    from tristage_rag_amd.index import IVFFlatIndex
    corpus, queries = _case(cls, n, d, 64)
    ivf = IVFFlatIndex(d, 8, dtype=dtype, nprobe=8)
    ivf.set_centroids(make_corpus(8, d, seed=3, dtype=dtype))
    ivf.add(_t(corpus, dtype))
    assert ivf.ntotal == n
    tq = _t(queries, dtype)
    want = ex.expected_topk(corpus, queries, 100)
    for k in (1, 100):
        got = ivf.search(tq, k)
        info = ivf.last_search_info()
        assert info["redone"] == 0 and (info["filter_passes"] >= 1) == (n >= 32768), info
        _exact(got, (want[0][:, :k], want[1][:, :k]), f"k={k}")
    ivf.close()


# --------------------------------------------------------------------------------- 3b: the split's terms, f32 storage
def _query_dtypes(cls):
    return {"A": ("f32", "f16", "bf16"), "B": ("f32",), "C": ("f32", "f16")}[cls]   # those the queries survive


@pytest.mark.parametrize("cls", ["A", "B", "C"])
@pytest.mark.parametrize("d", ex.SPLIT_D + ex.EXACT_F32_D)
def test_split_terms_are_exact_on_the_dense_path(torch_mod, d, cls):
    """Classes A, B and C make all six kept partial products of the bf16x3 split live and the three dropped ones zero
    (test_exact_scores_host.py): scan_f32s_kernel at d = 520 and 768, the exact-f32 kernel at 512 and 1024 on the same
    kind of input; float32, float16 and bfloat16 queries (qprep_f32s_kernel's three instantiations)."""
    n, B = ex.N_SPLIT, ex.B_SPLIT
    corpus, queries = _case(cls, n, d, B)
    idx = _flat(d, "f32", corpus)
    want_S = ex.exact_scores(corpus, queries).astype(np.float32)
    want = ex.expected_topk(corpus, queries, 10)
    for qdt in _query_dtypes(cls):
        tq = _t(queries, qdt)
        assert np.array_equal(_np(tq.float()), queries)
        S = _np(idx.scores(tq))
        bad = np.argwhere(S != want_S)
        assert bad.size == 0, f"{qdt} queries: {bad.shape[0]} scores differ, first at {bad[0].tolist()}"
        got = idx.search(tq, 10)
        assert idx.last_search_info()["path"] == "dense"
        _exact(got, want, f"{qdt} queries")
    idx.close()


@pytest.mark.parametrize("cls", ["A", "B", "C"])
@pytest.mark.parametrize("mode", ["classic", "one_launch"])
@pytest.mark.parametrize("d", ex.SPLIT_D + ex.EXACT_F32_D)
def test_split_terms_are_exact_on_the_filter_path(torch_mod, d, mode, cls):
    """The same classes above the filter path's floor.  B's few-hot rows tie in thousands, so its filter may fall back:
    only its result is asserted.  The one-launch scan is asked for at the smallest corpus it takes; the split
    dimensions have none and answer on five launches."""
    n = ex.N_FILTER if mode == "classic" else _one_launch_rows(torch_mod)
    corpus, queries = _case(cls, n, d, ex.B_SPLIT)
    idx = _flat(d, "f32", corpus)
    want = ex.expected_topk(corpus, queries, 100)
    for qdt in _query_dtypes(cls):
        tq = _t(queries, qdt)
        for k in (10, 100):
            got = idx.search(tq, k, classic=mode == "classic", one_launch=mode == "one_launch")
            info = idx.last_search_info()
            if cls != "B":
                assert info["path"] == "filter", info
                assert info["one_launch"] == (mode == "one_launch" and not _is_split("f32", d)), info
            _exact(got, (want[0][:, :k], want[1][:, :k]), f"{qdt} queries k={k}")
    idx.close()


# ------------------------------------------------------------------------- 3c: accuracy on the other tests' data
def test_split_scan_accuracy_on_unit_rows(torch_mod):
    """scan_f32s_kernel on unit-norm rows (20 000 x 768, 8 queries): the rms error of scores() against the float64
    oracle must stay below a third of the smallest rms error that losing one kept term causes in the numpy model of
    the split (about 1.2e-7; the factor 3 sits inside the 27x gap between the correct model and a faulty one).
    Measured on an MI355X: rms 1.10e-8, max 1.09e-7, i.e. 0.87x / 1.06x the rms / max error of a float32 BLAS product
    of the same inputs (1.26e-8 / 1.02e-7)."""
    corpus, queries = ex.accuracy_case()
    losses = ex.single_loss_rms(corpus, queries)
    threshold = ex.split_rms_threshold(losses)
    ref = np.stack([oracle.scores_f64(corpus, q) for q in queries])
    idx = _flat(corpus.shape[1], "f32", corpus)
    S = _np(idx.scores(_t(queries, "f32"))).astype(np.float64)
    idx.close()
    err = S - ref
    blas = (queries @ corpus.T).astype(np.float64) - ref
    print(f"\nsplit scan vs float64: rms {ex.rms(err):.3e} max {np.abs(err).max():.3e}; float32 BLAS: rms "
          f"{ex.rms(blas):.3e} max {np.abs(blas).max():.3e}; ratio rms {ex.rms(err) / ex.rms(blas):.2f} max "
          f"{np.abs(err).max() / np.abs(blas).max():.2f}; model {losses}; threshold {threshold:.3e}")
    assert ex.rms(err) < threshold


# ------------------------------------------------------------------------------- 3d: power-of-two scale invariance
SCALES = {"f16": ((8, 0), (8, 6)),                       # scaling down would leave f16's normal range
          "bf16": ((0, 0), (12, 0), (-12, -7), (20, 20)),
          "f32": ((0, 0), (12, 0), (-12, -7), (20, 20))}
SCALE_D = {"f16": (768,), "bf16": (768,), "f32": (64, 600)}       # fp32: the exact-f32 kernel and the split scan


@functools.lru_cache(maxsize=2)
def _unit_rows(n, d, dtype):
    c, q = make_corpus(n, d, seed=1234, dtype=dtype), make_corpus(ex.COALESCE_BATCHES * 64, d, seed=4321, dtype=dtype)
    c.setflags(write=False)
    q.setflags(write=False)
    return c, q


def _all_paths(torch, dtype, d, corpus, queries):
    """{path: (D, I)} of every scan family of 3a on one corpus."""
    from tristage_rag_amd.index import IVFFlatIndex
    out = {}
    k = 100
    tq = _t(queries, dtype)
    small = _flat(d, dtype, corpus[: ex.N_DENSE])
    out["dense"] = small.search(tq[:65], k)
    assert small.last_search_info()["path"] == "dense"
    out["scores"] = (small.scores(tq[:33]), torch.zeros(1))
    small.close()
    idx = _flat(d, dtype, corpus)
    for mode in ("classic", "one_launch"):
        out[mode] = idx.search(tq[:64], k, classic=mode == "classic", one_launch=mode == "one_launch")
        info = idx.last_search_info()
        assert info["path"] == "filter", info
        assert info["one_launch"] == (mode == "one_launch" and not _is_split(dtype, d)), info
    if dtype != "f32":                                   # masked, coalesced and IVF scans are 16-bit kernels
        n = corpus.shape[0]
        rng = np.random.default_rng(5)
        half = rng.random(n) < 0.5
        out["masked"] = idx.search(tq[:64], k, allowed=[None if b == 0 else half for b in range(64)])
        assert idx.last_filter_info()["filter_passes"] == 1
        batches = [tq[i * 64: (i + 1) * 64] for i in range(ex.COALESCE_BATCHES)]
        for wide in (False, True):
            outs, _ = _coalesced(torch, idx, batches, k, wide)
            out[f"coalesced wide={wide}"] = (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]))
        idx.remove_ids(np.arange(0, n, 3))
        out["tombstones"] = idx.search(tq[:64], k)
        outs, _ = _coalesced(torch, idx, batches[:3], k, True)
        out["tombstones coalesced"] = (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]))
        ivf = IVFFlatIndex(d, 8, dtype=dtype, nprobe=8)
        ivf.set_centroids(make_corpus(8, d, seed=3, dtype=dtype))
        ivf.add(_t(corpus, dtype))
        out["ivf"] = ivf.search(tq[:64], k)
        assert ivf.last_search_info()["filter_passes"] >= 1
        ivf.close()
    idx.close()
    return {name: (_np(D), _np(I)) for name, (D, I) in out.items()}


_BASE = {}


@pytest.mark.parametrize("dtype,d,s,t", [(dt, d, s, t) for dt in SCALES for d in SCALE_D[dt] for s, t in SCALES[dt]])
def test_power_of_two_scaling_changes_nothing_but_the_exponent(torch_mod, dtype, d, s, t):
    """Scaling by a power of two commutes with every rounding while nothing overflows or underflows: an index of
    2^s * corpus searched with 2^t * queries returns the ids of the unscaled search bit for bit and its scores times
    2^(s+t), on every path — thresholds, candidate filter, select keys and padding at |score| >> 1 and << 1."""
    torch = torch_mod
    corpus, queries = _unit_rows(_one_launch_rows(torch), d, dtype)
    key = (dtype, d)
    if key not in _BASE:
        _BASE.clear()
        _BASE[key] = _all_paths(torch, dtype, d, corpus, queries)
    base = _BASE[key]
    sc, sq = np.float32(2.0 ** s) * corpus, np.float32(2.0 ** t) * queries
    assert np.array_equal(oracle.quantize(sc, dtype), sc) and np.array_equal(oracle.quantize(sq, dtype), sq)
    assert np.array_equal(sc.astype(np.float64), corpus.astype(np.float64) * 2.0 ** s)        # no underflow, no overflow
    assert np.array_equal(sq.astype(np.float64), queries.astype(np.float64) * 2.0 ** t)
    got = _all_paths(torch, dtype, d, sc, sq)
    assert got.keys() == base.keys()
    for name in base:
        (D, I), (D0, I0) = got[name], base[name]
        assert np.array_equal(I, I0), name
        real = I0 >= 0 if I0.shape == D0.shape else np.ones(D0.shape, bool)
        assert np.array_equal(D[real].astype(np.float64), D0[real].astype(np.float64) * 2.0 ** (s + t)), name
        assert np.array_equal(D[~real], D0[~real]), name
