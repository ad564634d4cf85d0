"""CPU checks of maximal marginal relevance: the host model of tests/mmr_model.py against the
definition, the exactness of the inputs tests/test_mmr_gpu.py uses, and the boundary (argument errors, refusals,
config defaults, the C ABI) as far as it can be reached without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import exact_inputs as xi
import mmr_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = (0.0, 0.25, 0.5, 0.75, 1.0)
EXACT_D = {"f16": (40, 768, 1024), "bf16": (40, 768, 1024), "f32": (40, 768, 1024), "fp8": (256, 768)}


# ------------------------------------------------------------------ the model
def test_model_equals_brute_force_on_small_cases():
    n = 0
    for rel, S, valid in mm.all_small_cases(6):
        for lam in LAMBDAS:
            for k in range(1, len(rel) + 1):
                want = mm.mmr_brute_force(rel, S, k, lam, valid)
                got = mm.mmr_select(rel, S, k, lam, valid)
                assert got == want, (rel, S, valid, lam, k)
                assert mm.step_valid(rel, S, got, lam, 0.0, valid) == 0.0
                n += 1
    assert n > 3000


def test_batched_model_equals_the_model_per_query():
    rng = np.random.default_rng(9)
    B, C = 7, 40
    X = rng.integers(-3, 4, size=(B, C, 6)).astype(np.float32)
    S = np.einsum("bik,bjk->bij", X, X)
    rel = rng.integers(-5, 6, size=(B, C)).astype(np.float32)
    valid = rng.random((B, C)) < 0.7
    valid[3] = False                                          # a query with no valid candidate at all
    for lam in LAMBDAS:
        got = mm.mmr_select_batch(rel, S, C, lam, valid)
        for b in range(B):
            want = mm.mmr_select(rel[b], S[b], C, lam, valid[b])
            assert got[b, : len(want)].tolist() == want and (got[b, len(want):] == -1).all()
        assert np.array_equal(mm.mmr_select_batch(rel, S, 5, lam, valid), got[:, :5])   # prefixes


def test_lambda_one_is_relevance_order_and_step_zero_is_argmax():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((50, 8))
    S = X @ X.T
    rel = np.sort(rng.standard_normal(50))[::-1].copy()      # a list sorted by relevance, as search returns it
    assert mm.mmr_select(rel, S, 20, 1.0) == list(range(20))
    rel[7] = rel[6]                                           # a tie keeps the lower position first
    assert mm.mmr_select(rel, S, 20, 1.0) == list(range(20))
    shuffled = rng.permutation(rel)
    order = sorted(range(50), key=lambda i: (-shuffled[i], i))
    assert mm.mmr_select(shuffled, S, 50, 1.0) == order
    for lam in LAMBDAS:
        assert mm.mmr_select(shuffled, S, 3, lam)[0] == order[0]
    assert mm.mmr_select(shuffled, S, 1, 0.0) == [order[0]]


def test_duplicates_are_picked_once_and_padding_never():
    rng = np.random.default_rng(6)
    X = rng.integers(-3, 4, size=(12, 5)).astype(np.float64)
    X[4] = X[1]
    X[9] = X[1]                                               # three copies of one row
    rel = X @ X[1]
    S = X @ X.T
    for lam in LAMBDAS:
        picks = mm.mmr_select(rel, S, 12, lam)
        assert sorted(picks) == list(range(12))               # every position exactly once
    picks = mm.mmr_select(rel, S, 3, 0.5)
    assert picks[0] == 1 and not {4, 9} & set(picks[1:])      # the copies lose against anything less similar
    valid = np.ones(12, dtype=bool)
    valid[[0, 1, 11]] = False
    for lam in LAMBDAS:
        picks = mm.mmr_select(rel, S, 12, lam, valid)
        assert len(picks) == 9 and not {0, 1, 11} & set(picks)
    D, I = mm.mmr_output(np.arange(100, 112), rel, picks, 12)
    assert (I[9:] == -1).all() and (D[9:] == -mm.FLT_MAX).all() and (I[:9] == 100 + np.array(picks)).all()


def test_step_valid_rejects_a_wrong_pick_and_accepts_a_near_tie():
    rel = np.array([1.0, 1.0 - 1e-7, 0.2])
    S = np.eye(3)
    assert mm.mmr_select(rel, S, 2, 0.5) == [0, 1]
    assert mm.step_valid(rel, S, [1, 0], 0.5, 2e-6) <= 2e-6    # a float near-tie may go the other way
    with pytest.raises(AssertionError):
        mm.step_valid(rel, S, [2, 0], 0.5, 2e-6)
    with pytest.raises(AssertionError):
        mm.step_valid(rel, S, [0, 0], 0.5, 2e-6)               # picked twice


@pytest.mark.parametrize("dtype", sorted(EXACT_D))
def test_exact_inputs_give_exact_similarities_and_objectives(dtype):
    """The integer rows of the GPU test: every partial sum of a similarity or relevance is an integer below 2^22, and
    lambda * rel - (1 - lambda) * sim with lambda a multiple of 1/4 is a multiple of 1/4 below 2^22: an f32 number,
    whatever the order of the additions.  So the f32 kernels must return the float64 model bit for bit."""
    amp = 15 if dtype == "fp8" else 63
    for d in EXACT_D[dtype]:
        assert amp * amp * d < 2 ** 22
        c, q, _ = xi.gen_ints(64, d, 2)
        if dtype == "fp8":
            c, q = np.clip(c, -15, 15), np.clip(q, -15, 15)
        assert np.abs(c).max() <= amp
        S = c.astype(np.float64) @ c.astype(np.float64).T
        rel = c.astype(np.float64) @ q[0].astype(np.float64)
        assert np.array_equal(S, S.astype(np.float32).astype(np.float64)) and np.abs(S).max() < 2 ** 22
        assert np.array_equal(S, S.T)
        for lam in LAMBDAS:
            lam32, oml32 = np.float32(lam), np.float32(1.0) - np.float32(lam)
            obj64 = lam * rel[:, None] - (1.0 - lam) * S
            obj32 = (lam32 * rel.astype(np.float32))[:, None] - oml32 * S.astype(np.float32)
            assert obj32.dtype == np.float32 and np.array_equal(obj32.astype(np.float64), obj64)


# ------------------------------------------------------------------ the boundary
def test_header_declares_and_library_exports_the_entry_points():
    from tristage_rag_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tristage.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ts_index_mmr", "ts_mmr_ivf"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.header_abi_version() == 4
    assert "ts_mmr.hip" in open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()


def test_entry_points_validate_arguments_without_a_gpu():
    from tristage_rag_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)      # never dereferenced: the calls fail first
    h = ctypes.c_void_p(8192)
    half = ctypes.c_float(0.5)
    for fn in (lib.ts_index_mmr, lib.ts_mmr_ivf):
        assert fn(None, p, p, 1, 10, 5, half, p, p, 0, None) == _lib.TS_ERR_INVALID
        assert b"null handle" in lib.ts_last_error()
        assert fn(h, None, p, 1, 10, 5, half, p, p, 0, None) == _lib.TS_ERR_INVALID
        assert fn(h, p, None, 1, 10, 5, half, p, p, 0, None) == _lib.TS_ERR_INVALID
        assert fn(h, p, p, 1, 10, 5, half, None, p, 0, None) == _lib.TS_ERR_INVALID
        assert fn(h, p, p, 1, 10, 5, half, p, None, 0, None) == _lib.TS_ERR_INVALID
        assert b"null pointer" in lib.ts_last_error()
        assert fn(h, p, p, 1, 10, 11, half, p, p, 0, None) == _lib.TS_ERR_INVALID            # k > fetch_k
        assert b"fetch_k" in lib.ts_last_error()
        assert fn(h, p, p, 1, 10, 0, half, p, p, 0, None) == _lib.TS_ERR_INVALID             # k < 1
        for bad in (-0.01, 1.01, float("nan"), float("inf")):
            assert fn(h, p, p, 1, 10, 5, ctypes.c_float(bad), p, p, 0, None) == _lib.TS_ERR_INVALID
            assert b"lambda" in lib.ts_last_error()
        assert fn(h, p, p, -1, 10, 5, half, p, p, 0, None) == _lib.TS_ERR_INVALID
        assert fn(h, p, p, 1, 1025, 5, half, p, p, 0, None) == _lib.TS_ERR_UNSUPPORTED       # fetch_k > 1024
        assert b"1024" in lib.ts_last_error()


def test_python_argument_errors_are_raised_before_anything_is_launched():
    from tristage_rag_amd import index
    assert index.mmr_default_fetch_k(1) == 20 and index.mmr_default_fetch_k(20) == 80
    assert index.mmr_default_fetch_k(300) == 1024
    assert index.mmr_check(5, 20, 0.5) == (5, 20, 0.5)
    ids = np.zeros((2, 8), dtype=np.int64)
    rel = np.zeros((2, 8), dtype=np.float32)
    q = np.zeros((2, 16), dtype=np.float32)
    for cls in (index.FlatIPIndex, index.IVFFlatIndex):
        ix = cls.__new__(cls)          # no handle: whatever reached the library would fail differently
        for lam in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="lambda_mult"):
                ix.mmr(ids, rel, 4, lambda_mult=lam)
            with pytest.raises(ValueError, match="lambda_mult"):
                ix.search_mmr(q, 4, lambda_mult=lam)
        with pytest.raises(ValueError, match="fetch_k"):
            ix.mmr(ids, rel, 9)                                    # k > fetch_k = 8
        with pytest.raises(ValueError, match="fetch_k"):
            ix.search_mmr(q, 30, fetch_k=20)
        with pytest.raises(ValueError, match="1024"):
            ix.search_mmr(q, 4, fetch_k=1025)
        with pytest.raises(ValueError, match="1024"):
            ix.mmr(np.zeros((1, 1025), np.int64), np.zeros((1, 1025), np.float32), 4)
        with pytest.raises(ValueError, match="positive"):
            ix.mmr(ids, rel, 0)
        with pytest.raises(ValueError, match="shape"):
            ix.mmr(ids, rel[:, :4], 2)
        ix._h = None                   # (__del__ then has nothing to close)


def test_sharded_classes_refuse(tmp_path):
    from tristage_rag_amd.parallel_pipeline import ShardedRetrievalPipeline
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig
    from tristage_rag_amd.sharded import ShardedFlatIPIndex
    sh = ShardedFlatIPIndex.__new__(ShardedFlatIPIndex)
    with pytest.raises(NotImplementedError):
        sh.mmr(np.zeros((1, 4), np.int64), np.zeros((1, 4), np.float32), 2)
    with pytest.raises(NotImplementedError):
        sh.search_mmr(np.zeros((1, 8), np.float32), 2)
    kw = dict(stage1_model="random:tiny", stage2_model="random:tiny", stage3_model="random:tiny", device="cpu",
              cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"), log_file=str(tmp_path / "p.log"))
    p = ShardedRetrievalPipeline(config=PipelineConfig(**kw))
    with pytest.raises(NotImplementedError, match="mmr_lambda"):
        p.search("a query", mmr_lambda=0.5)
    with pytest.raises(NotImplementedError, match="mmr_lambda"):
        p.search_many(["a query"], mmr_lambda=0.5)
    with pytest.raises(NotImplementedError, match="mmr_lambda"):
        p.batch_search(["a query"], mmr_lambda=0.5)
    p2 = ShardedRetrievalPipeline(config=PipelineConfig(mmr_lambda=0.3, **kw))
    with pytest.raises(NotImplementedError, match="mmr_lambda"):
        p2.search("a query")


def test_config_fields_default_to_off_and_bad_lambdas_are_refused(tmp_path):
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    assert Stage1Config().mmr_lambda is None and PipelineConfig().mmr_lambda is None
    r = Stage1Retriever.__new__(Stage1Retriever)
    r.config, r.bm25_index, r.faiss_index = Stage1Config(enable_bm25=False), None, None
    assert r._mmr_lambda(None) is None and r._mmr_lambda(0.25) == 0.25
    for bad in (-0.5, 2.0, float("nan")):
        with pytest.raises(ValueError, match="mmr_lambda"):
            r._mmr_lambda(bad)
    r.config, r.bm25_index = Stage1Config(enable_bm25=True), object()        # BM25 fusion on: dense-only route
    assert r._mmr_lambda(None) is None
    with pytest.raises(ValueError, match="BM25"):
        r._mmr_lambda(0.5)
    p = RetrievalPipeline(config=PipelineConfig(log_file=str(tmp_path / "p.log")))
    assert p._mmr_lambda(None) is None and p._mmr_lambda(1.0) == 1.0
    with pytest.raises(ValueError, match="mmr_lambda"):
        p._mmr_lambda(1.5)
