"""Funnel search on the GPU: ``search_prefix`` against the mirror index it is specified by,
``rescore`` against the numpy model over ``scores()``, ``search_funnel`` against both and against ``search``.
Every comparison of scores and ids is ``np.array_equal``: the prefix pass reads the same stored bytes in the same
k-group order as the mirror's search, and the rescore accumulates the k groups as the scan does."""
import numpy as np
import pytest

import exact_inputs as ei
import funnel_model as fm
from helpers import make_corpus
from pipeline_pairs import gpu_pipeline, synth_docs

pytestmark = pytest.mark.gpu

N_FILTER = 32768 + 37        # just above the filter path's floor, a ragged last block
N_DENSE = 1000               # the dense path
SHAPES = ((256, 128), (384, 256), (768, 512), (1024, 128))     # kg' = 8 (the tail is the whole block), 16, 32, 8 of 64
BATCHES = (1, 7, 32, 33, 64, 65)
KS = (1, 10, 100)


def _torch():
    import torch
    return torch


def _tdtype(dtype):
    torch = _torch()
    return torch.float16 if dtype == "f16" else torch.bfloat16


def _index(rows, dtype):
    from tristage_rag_amd.index import FlatIPIndex
    ix = FlatIPIndex(rows.shape[1], dtype=dtype)
    ix.add(rows)
    return ix


def _dev(x, dtype):
    return _torch().from_numpy(np.array(x, copy=True)).cuda().to(_tdtype(dtype))


def _np(*ts):
    return tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in ts)


def _same(got, want, what=""):
    gd, gi = _np(*got)
    wd, wi = _np(*want)
    assert np.array_equal(gi, wi), f"{what}: ids differ"
    assert np.array_equal(gd, wd), f"{what}: scores differ"


def _filter_path(ix, k):
    return int(ix._lib.ts_index_filter_path(ix._h, int(k)))


# ------------------------------------------------------------------------------------------- prefix equals mirror
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d,dims", SHAPES)
@pytest.mark.parametrize("n", [N_FILTER, N_DENSE])
def test_prefix_equals_mirror(n, d, dims, dtype):
    rows = make_corpus(n, d, seed=d + dims, dtype=dtype)
    q = _dev(make_corpus(max(BATCHES), d, seed=7 * d + 1, dtype=dtype), dtype)
    ix = _index(rows, dtype)
    M = fm.mirror_index(ix, dims)
    try:
        assert M.ntotal == n and M.d == dims
        for k in KS:
            assert _filter_path(ix, k) == (1 if n == N_FILTER else 0)
            for B in BATCHES:
                got = ix.search_prefix(q[:B], k, dims)
                if n == N_FILTER:
                    assert ix.last_search_info()["path"].startswith("filter")
                else:
                    assert ix.last_search_info()["path"] == "dense"
                _same(got, M.search(q[:B, :dims].contiguous(), k), f"n={n} d={d} dims={dims} {dtype} B={B} k={k}")
        # the dense path of a corpus that would take the filter path (TS_FLAG_NO_FILTER), and numpy in -> numpy out
        got = ix.search_prefix(q[:33], 10, dims, exact_dense=True)
        assert ix.last_search_info()["path"] == "dense"
        _same(got, M.search(q[:33, :dims].contiguous(), 10, exact_dense=True), "TS_FLAG_NO_FILTER")
        qn = q[:7].float().cpu().numpy()
        D, I = ix.search_prefix(qn, 10, dims)
        assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
        _same((D, I), M.search(np.ascontiguousarray(qn[:, :dims]), 10), "host pointers")
    finally:
        ix.close()
        M.close()


# ----------------------------------------------------------------------------------------------------- zero tails
@pytest.mark.parametrize("dtype,d,dims", [("f16", 768, 256), ("bf16", 384, 128)])
def test_rows_with_zero_tails_rank_as_the_full_search(dtype, d, dims):
    """Rows whose components beyond ``dims`` are zero: the prefix score IS the score (the k groups beyond the prefix
    add exact zeros), so the prefix pass equals ``search`` and so does the funnel.  No mirror in this one."""
    rows = make_corpus(N_FILTER, d, seed=11, dtype=dtype).copy()
    rows[:, dims:] = 0.0
    q = _dev(make_corpus(65, d, seed=12, dtype=dtype), dtype)
    ix = _index(rows, dtype)
    try:
        for B, k in ((65, 10), (32, 100), (1, 1)):
            want = ix.search(q[:B], k)
            _same(ix.search_prefix(q[:B], k, dims), want, f"prefix B={B} k={k}")
            _same(ix.search_funnel(q[:B], k, dims), want, f"funnel B={B} k={k}")
            info = ix.last_funnel_info()
            assert info == {"dims": dims, "fetch_k": min(2048, max(8 * k, 128)), "prefix_path": "filter"}
    finally:
        ix.close()


# ---------------------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("dtype,d,dims", [("f16", 384, 256), ("bf16", 256, 128)])
def test_masks_equal_the_mirror_with_the_same_masks(dtype, d, dims):
    n, B, k = N_FILTER, 33, 10
    rng = np.random.default_rng(5)
    rows = make_corpus(n, d, seed=21, dtype=dtype)
    q = _dev(make_corpus(B, d, seed=22, dtype=dtype), dtype)
    ix = _index(rows, dtype)
    M = fm.mirror_index(ix, dims)
    half = rng.random(n) < 0.5
    third = rng.random(n) < 0.33
    none = np.zeros(n, dtype=bool)
    tenant = np.zeros(n, dtype=bool)
    tenant[rng.choice(n, size=100, replace=False)] = True       # fewer allowed sample rows than the rank: the exact path
    few = np.zeros(n, dtype=bool)
    few[[3, n - 1]] = True                                       # fewer allowed rows than k: padded
    per_query = [(half, third, None, tenant, none, few)[i % 6] for i in range(B)]
    try:
        for name, allowed in (("one mask", half), ("per query", per_query), ("all false", none), ("tenant", tenant)):
            got = ix.search_prefix(q, k, dims, allowed=allowed)
            _same(got, M.search(q[:, :dims].contiguous(), k, allowed=allowed), name)
            _, I = _np(*got)
            masks = allowed if isinstance(allowed, list) else [allowed] * B
            for b, m in enumerate(masks):
                hit = I[b][I[b] >= 0]
                assert m is None or m[hit].all(), f"{name}: query {b} got a row outside its mask"
        assert (_np(*ix.search_prefix(q, k, dims, allowed=none))[1] == -1).all()
        # the funnel under a mask: the rescore of the masked shortlist
        D, I = ix.search_funnel(q, k, dims, fetch_k=200, allowed=per_query)
        _same((D, I), ix.rescore(q, ix.search_prefix(q, 200, dims, allowed=per_query)[1], k), "masked funnel")
    finally:
        ix.close()
        M.close()


# ------------------------------------------------------------------------------------------------------ mutations
def test_prefix_search_follows_add_remove_update_compact():
    dtype, d, dims, k, B = "f16", 384, 256, 10, 33
    rows = make_corpus(N_FILTER + 500, d, seed=31, dtype=dtype)
    fresh = make_corpus(300, d, seed=32, dtype=dtype)
    q = _dev(make_corpus(B, d, seed=33, dtype=dtype), dtype)
    rng = np.random.default_rng(34)
    from tristage_rag_amd.index import FlatIPIndex
    ix = FlatIPIndex(d, dtype=dtype)
    mirrors = []
    try:
        for lo, hi in ((0, 10_000), (10_000, 10_037), (10_037, N_FILTER)):      # add in three calls
            ix.add(rows[lo:hi])
        top = _np(*ix.search_prefix(q, k, dims))[1]
        gone = np.unique(np.concatenate([top[:, 0], top[:5, 1], rng.choice(N_FILTER, size=700, replace=False)]))
        assert ix.remove_ids(gone) == gone.size
        live_ids = np.setdiff1d(np.arange(N_FILTER), gone)
        upd = rng.choice(live_ids, size=300, replace=False)
        ix.update_rows(upd, fresh)
        ix.add(rows[N_FILTER:])
        assert ix.nlive == N_FILTER + 500 - gone.size
        M = fm.mirror_index(ix, dims)
        mirrors.append(M)
        got = ix.search_prefix(q, k, dims)
        assert not np.isin(_np(*got)[1], gone).any()                              # before compact(): no removed id
        _same(got, M.search(q[:, :dims].contiguous(), k), "tombstones")
        some = rng.random(ix.ntotal) < 0.5
        _same(ix.search_prefix(q, k, dims, allowed=some), M.search(q[:, :dims].contiguous(), k, allowed=some),
              "tombstones and a mask")
        ix.compact()
        assert ix.ntotal == ix.nlive == N_FILTER + 500 - gone.size
        M2 = fm.mirror_index(ix, dims)
        mirrors.append(M2)
        _same(ix.search_prefix(q, k, dims), M2.search(q[:, :dims].contiguous(), k), "after compact()")
    finally:
        ix.close()
        for m in mirrors:
            m.close()


# -------------------------------------------------------------------------------------------------------- rescore
@pytest.fixture(scope="module")
def rescore_case():
    """One index with removed rows, its full score matrix (read once, shared, left unchanged) and the queries."""
    dtype, d, n, B = "f16", 768, 20_000, 65
    rows = make_corpus(n, d, seed=41, dtype=dtype)
    qn = make_corpus(B, d, seed=42, dtype=dtype)
    ix = _index(rows, dtype)
    removed = np.arange(5, n, 97)
    ix.remove_ids(removed)
    live = np.ones(n, dtype=bool)
    live[removed] = False
    q = _dev(qn, dtype)
    S = ix.scores(q).cpu().numpy()
    S.setflags(write=False)
    yield ix, q, qn, S, live
    ix.close()


def _candidates(rng, B, C, n, live):
    ids = rng.integers(0, n, size=(B, C)).astype(np.int64)
    if C >= 8:
        for b in range(B):
            ids[b, rng.integers(0, C)] = -1                               # padding
            ids[b, rng.integers(0, C)] = n + 5                            # out of range
            ids[b, rng.integers(0, C)] = -9
            ids[b, rng.integers(0, C)] = np.flatnonzero(~live)[b % 7]     # a removed row
            ids[b, C - 1] = ids[b, 0]                                     # a duplicate
    return ids


@pytest.mark.parametrize("C,B", [(1, 5), (31, 5), (32, 5), (33, 65), (1000, 33), (16384, 2)])
def test_rescore_equals_the_model_over_scores(rescore_case, C, B):
    ix, q, qn, S, live = rescore_case
    torch = _torch()
    rng = np.random.default_rng(C)
    ids = _candidates(rng, B, C, ix.ntotal, live)
    want = fm.rescore_model(S[:B], ids, live=live)
    got = ix.rescore(q[:B], torch.from_numpy(ids).cuda())                 # CUDA tensors in -> tensors out
    assert got[0].is_cuda and got[1].is_cuda and tuple(got[0].shape) == (B, C)
    _same(got, want, f"C={C} B={B}")
    if C >= 8:
        assert (want[1][:, -1] == -1).all() and (want[1][:, 0] >= 0).all()       # the case has invalid entries
    D, I = ix.rescore(qn[:B], ids)                                        # numpy in -> numpy out
    assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
    _same((D, I), want, f"numpy C={C} B={B}")
    for k in sorted({1, max(1, C // 3), max(1, C - 1)}):                   # k < C (k = 1 = C for one candidate)
        _same(ix.rescore(q[:B], torch.from_numpy(ids).cuda(), k), fm.rescore_model(S[:B], ids, k=k, live=live),
              f"C={C} B={B} k={k}")


def test_rescore_bf16_with_an_id_offset():
    dtype, d, n, B, C = "bf16", 256, 3000, 65, 100
    ix = _index(make_corpus(n, d, seed=51, dtype=dtype), dtype)
    try:
        q = _dev(make_corpus(B, d, seed=52, dtype=dtype), dtype)
        S = ix.scores(q).cpu().numpy()
        ix.set_id_offset(1_000_000)
        rng = np.random.default_rng(53)
        ids = rng.integers(0, n, size=(B, C)).astype(np.int64) + 1_000_000
        ids[:, 3] = 17                                                    # below the offset: out of range
        ids[:, 5] = -1
        _same(ix.rescore(q, ids), fm.rescore_model(S, ids, id_offset=1_000_000), "bf16, offset")
        D, I = _np(*ix.search(q, 10))
        _same(ix.rescore(q, I), (D, I), "the ids and scores search returned")
    finally:
        ix.close()


# --------------------------------------------------------------------------------------------------------- funnel
@pytest.mark.parametrize("dtype,d,dims", [("f16", 768, 256), ("bf16", 384, 256)])
def test_funnel_is_the_rescore_of_the_prefix_shortlist(dtype, d, dims):
    rows = make_corpus(N_FILTER, d, seed=61, dtype=dtype)
    q = _dev(make_corpus(65, d, seed=62, dtype=dtype), dtype)
    ix = _index(rows, dtype)
    try:
        for B, k, fetch in ((65, 10, None), (33, 100, None), (7, 10, 4000), (1, 5, 5)):
            f = min(2048, max(8 * k, 128)) if fetch is None else fetch
            got = ix.search_funnel(q[:B], k, dims, fetch_k=fetch)
            assert ix.last_funnel_info() == {"dims": dims, "fetch_k": f, "prefix_path": "filter" if f <= 2048 else "dense"}
            _same(got, ix.rescore(q[:B], ix.search_prefix(q[:B], f, dims)[1], k), f"B={B} k={k} fetch_k={fetch}")
            D, I = _np(*got)
            full = _np(*ix.search(q[:B], f))                                          # every returned score is the exact one
            for b in range(B):
                pos = {int(i): j for j, i in enumerate(full[1][b])}
                assert all(int(i) not in pos or D[b, j] == full[0][b, pos[int(i)]] for j, i in enumerate(I[b]))
        D, I = ix.search_funnel(q[:7].float().cpu().numpy(), 10, dims)                # numpy in -> numpy out
        assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
        _same((D, I), ix.search_funnel(q[:7], 10, dims), "numpy")
    finally:
        ix.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_funnel_with_an_exhaustive_shortlist_equals_search(dtype):
    d, dims, n, B = 384, 128, 5000, 33
    rows = make_corpus(n, d, seed=71, dtype=dtype)
    q = _dev(make_corpus(B, d, seed=72, dtype=dtype), dtype)
    ix = _index(rows, dtype)
    try:
        rng = np.random.default_rng(73)
        some = rng.random(n) < 0.4
        per_query = [some if b % 2 else None for b in range(B)]
        for k in (1, 10, 100):
            _same(ix.search_funnel(q, k, dims, fetch_k=n), ix.search(q, k), f"k={k}")
            _same(ix.search_funnel(q, k, dims, fetch_k=n + 100, allowed=some), ix.search(q, k, allowed=some), f"mask k={k}")
            _same(ix.search_funnel(q, k, dims, fetch_k=n, allowed=per_query), ix.search(q, k, allowed=per_query),
                  f"per-query masks k={k}")
        gone = rng.choice(n, size=400, replace=False)
        ix.remove_ids(gone)
        assert ix.nlive == n - 400
        for k in (10, 100):
            got = ix.search_funnel(q, k, dims, fetch_k=ix.nlive)
            _same(got, ix.search(q, k), f"removed rows k={k}")
            assert not np.isin(_np(*got)[1], gone).any()
    finally:
        ix.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_planted_ties_go_to_the_lower_id_in_both_passes(dtype):
    """Exactly summable integer rows (tests/exact_inputs.py): every score is exact in fp32 whatever the order, so the
    float64 model is the expected result bit for bit.  Six copies of query 0's best row are planted.  With zero tails
    the prefix score is the score, so a shortlist of four must take the four lowest of the six tied ids (the prefix
    pass) and return them in id order (the rescore)."""
    d, dims, B = 768, 256, 64
    c, q, unit = ei.case("ints", ei.N_FILTER, d, B)
    c = c.copy()
    c[:, dims:] = 0.0
    ei.assert_exactly_summable(c, q, unit)
    s0 = ei.exact_scores(c, q[:1])[0]
    best = int(np.argmax(s0))
    planted = np.array([31, 32, 1000, 20_000, 32_768, ei.N_FILTER - 1])              # two row blocks apart and a block edge
    planted = planted[planted != best]
    c[planted] = c[best]
    tied = np.sort(np.concatenate([[best], planted]))
    ix = _index(c, dtype)
    try:
        qt = _dev(q, dtype)
        for k, fetch in ((4, 4), (4, None), (10, 10), (100, None)):
            want = ei.expected_topk(c, q, k)
            got = ix.search_funnel(qt, k, dims, fetch_k=fetch)
            _same(got, want, f"k={k} fetch_k={fetch}")
            assert _np(*got)[1][0, : min(k, tied.size)].tolist() == tied[: min(k, tied.size)].tolist()
            _same(ix.search_prefix(qt, k, dims), want, f"prefix k={k}")
        # a dense-path corpus with an exhaustive shortlist and full-width rows: ties at every rank of the rescore
        c2, q2, unit2 = ei.case("ints", ei.N_DENSE, d, 33)
        c2 = c2.copy()
        c2[5::7] = c2[3]                                                              # 151 equal rows
        ei.assert_exactly_summable(c2, q2, unit2)
        ix2 = _index(c2, dtype)
        try:
            _same(ix2.search_funnel(_dev(q2, dtype), 200, dims, fetch_k=ei.N_DENSE), ei.expected_topk(c2, q2, 200), "dense")
        finally:
            ix2.close()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ retriever and pipeline
STAGE1 = "random:tiny:256"        # the tiny random encoder at 256 dimensions: the smallest with a prefix (128)
QUERIES = ["neural network attention", "gpu memory index", "language retrieval system"]


def _docs(n=200):
    docs = synth_docs(n, seed=9)
    meta = [{"tenant": i % 3} for i in range(n)]
    return docs, meta


def _retriever(tmp_path, **extra):
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    cfg = dict(model_name=STAGE1, device="cuda", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
               use_fp16=False, index_dtype="f16", funnel_fetch_k=256)
    cfg.update(extra)
    r = Stage1Retriever(Stage1Config(**cfg))
    r.add_documents(*_docs())
    return r


@pytest.mark.parametrize("bm25", [False, True])
def test_retriever_records_with_an_exhaustive_funnel_are_the_plain_ones(tmp_path, bm25):
    r = _retriever(tmp_path, enable_bm25=bm25)
    top_k = 20
    flt = {"tenant": 1}
    for q in QUERIES:
        plain = r.search(q, top_k)
        assert len(plain) == top_k
        assert r.search(q, top_k, funnel_dims=None) == plain                       # None: today's search
        assert r.search(q, top_k, funnel_dims=128) == plain
        assert r.search(q, top_k, filter=flt, funnel_dims=128) == r.search(q, top_k, filter=flt)
        assert all(x["metadata"]["tenant"] == 1 for x in r.search(q, top_k, filter=flt, funnel_dims=128))
    assert r.faiss_index.last_funnel_info()["dims"] == 128 and r.faiss_index.last_funnel_info()["fetch_k"] == 256
    assert r.search_many(QUERIES, top_k, funnel_dims=128) == r.search_many(QUERIES, top_k)
    assert r.search_many(QUERIES, top_k, filter=[flt, None, {"tenant": 2}], funnel_dims=128) == \
        r.search_many(QUERIES, top_k, filter=[flt, None, {"tenant": 2}])
    for kw in ({}, {"filter": flt}):
        a, b = r.search_many_arrays(QUERIES, top_k, funnel_dims=128, **kw), r.search_many_arrays(QUERIES, top_k, **kw)
        assert a is not None and b is not None
        for x, y in zip(a, b):
            assert np.array_equal(*_np(x, y))
    r.config.funnel_dims = 128                                                     # the config's value is the default
    assert r.search(QUERIES[0], top_k) == r.search(QUERIES[0], top_k, funnel_dims=128)
    r.config.funnel_dims = None
    # the refusals
    for dims in (100, 256):
        with pytest.raises(ValueError, match="dims"):
            r.search(QUERIES[0], top_k, funnel_dims=dims)
    if not bm25:
        with pytest.raises(ValueError, match="funnel_dims"):
            r.search(QUERIES[0], top_k, funnel_dims=128, mmr_lambda=0.5)
        with pytest.raises(ValueError, match="funnel_dims"):
            r.search_many(QUERIES, top_k, funnel_dims=128, group_by="tenant")
        with pytest.raises(ValueError, match="funnel_dims"):
            r.search_many_arrays(QUERIES, top_k, funnel_dims=128, group_by="tenant")


def test_retriever_refuses_the_funnel_on_other_indexes(tmp_path):
    f32 = _retriever(tmp_path, enable_bm25=False, index_dtype="f32")
    with pytest.raises(NotImplementedError, match="f32"):
        f32.search(QUERIES[0], 10, funnel_dims=128)
    assert len(f32.search(QUERIES[0], 10)) == 10
    ivf = _retriever(tmp_path, enable_bm25=False, index_type="ivf", nlist=4, nprobe=4)
    with pytest.raises(NotImplementedError, match="IVF"):
        ivf.search(QUERIES[0], 10, funnel_dims=128)
    with pytest.raises(NotImplementedError, match="IVF"):
        ivf.search_many(QUERIES, 10, funnel_dims=128)
    with pytest.raises(NotImplementedError, match="funnel"):
        ivf.faiss_index.search_funnel(np.zeros((1, 256), np.float32), 5, 128)


def _stages(out):
    return {key: out[key] for key in ("results", "stage1_results", "stage2_results")}


def test_pipeline_records_with_an_exhaustive_funnel_are_the_plain_ones(tmp_path):
    docs, meta = _docs()
    kw = dict(models=(STAGE1, "random:tiny", "random:tiny"), stage1_index_dtype="f16", stage1_funnel_fetch_k=256)
    for name, extra in (("fused", {}), ("dense", {"stage1_enable_bm25": False})):
        (tmp_path / name).mkdir()
        p = gpu_pipeline(tmp_path / name, name, **kw, **extra)
        p.add_documents(docs, meta)
        flt = {"tenant": 2}
        for q in QUERIES[:2]:
            plain = p.search(q)
            assert len(plain["results"]) == 5
            assert _stages(p.search(q, funnel_dims=None)) == _stages(plain)
            assert _stages(p.search(q, funnel_dims=128)) == _stages(plain)
            assert _stages(p.search(q, filter=flt, funnel_dims=128)) == _stages(p.search(q, filter=flt))
        assert p.stage1.faiss_index.last_funnel_info() == {"dims": 128, "fetch_k": 256, "prefix_path": "dense"}
        assert [_stages(o) for o in p.search_many(QUERIES, funnel_dims=128)] == [_stages(o) for o in p.search_many(QUERIES)]
        assert [_stages(o) for o in p.batch_search(QUERIES[:2], funnel_dims=128)] == \
            [_stages(o) for o in p.batch_search(QUERIES[:2])]
        with pytest.raises(ValueError, match="funnel_dims"):
            p.search(QUERIES[0], funnel_dims=128, mmr_lambda=0.5)
        with pytest.raises(ValueError, match="funnel_dims"):
            p.search_many(QUERIES, funnel_dims=128, group_by="tenant")
        p.config.stage1_funnel_dims = 128                                          # the config's value is the default
        assert _stages(p.search(QUERIES[0])) == _stages(p.search(QUERIES[0], funnel_dims=128))
        with pytest.raises(ValueError, match="funnel_dims"):
            p.batch_search(QUERIES[:1], mmr_lambda=0.5)
