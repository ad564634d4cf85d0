"""The fp4 (OCP e2m1 elements, one E8M0 scale per 32) stage-1 index on the GPU.

Stored values: ``reconstruct_n()`` equals ``decode(quantize_rows_mxfp4_reference(x))`` bit for bit.
Scores: a bf16 ``FlatIPIndex`` built from the fp4 index's ``reconstruct_n()`` (the mirror) holds exactly the values
the fp4 scan converts its nibbles to, and walks the same k steps, so ids and score bits are EQUAL, with no tolerance,
on every path.  This also decides which nibble of a byte the conversion instruction takes first: reconstruct decodes
with integer operations.  Relevance: the planted case is decided by the model in test_fp4_index_host.py."""
import ctypes

import numpy as np
import pytest

import fp4_index_model as fm

pytestmark = pytest.mark.gpu

N_FILTER, N_DENSE = 40_000, 2_080


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _ix():
    from tristage_rag_amd import index
    return index


def _fp4(d, rows=None, **kw):
    idx = _ix().FlatIPIndex(d, dtype="fp4")
    if rows is not None:
        idx.add(rows, **kw)
    return idx


def _want(x, d):
    ix = _ix()
    return ix.decode_rows_mxfp4(*ix.quantize_rows_mxfp4_reference(x), d)


def _mirror(idx):
    """The bf16 index of the decoded rows; it takes the same five-launch filter path as the fp4 index."""
    m = _ix().FlatIPIndex(idx.d, dtype="bf16")
    m.classic_filter = True
    m.coalesce = False
    rec = idx.reconstruct_n()
    m.add(rec)
    assert np.array_equal(m.reconstruct_n().view(np.uint32), rec.view(np.uint32))   # every decoded value is exact in bf16
    return m


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ids(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _same(got, want):
    (D, I), (Dm, Im) = got, want
    assert np.array_equal(_ids(I), _ids(Im)), "ids"
    assert np.array_equal(_bits(D), _bits(Dm)), "score bits"


def _queries(b, d, seed):
    return fm.clamp_queries(fm.unit_rows(b, d, seed))


class Pair:
    def __init__(self, n, d, seed):
        self.rows = fm.unit_rows(n, d, seed)
        self.idx = _fp4(d, self.rows)
        self.mirror = _mirror(self.idx)
        self.n, self.d = n, d

    def close(self):
        self.idx.close()
        self.mirror.close()


_PAIRS = {}


@pytest.fixture(scope="module")
def pairs():
    """(n, d) -> Pair, built on first use and shared by the tests of this module."""
    def get(n, d):
        if (n, d) not in _PAIRS:
            _PAIRS[(n, d)] = Pair(n, d, seed=n % 97 + d)
        return _PAIRS[(n, d)]
    yield get
    for p in _PAIRS.values():
        p.close()
    _PAIRS.clear()


# ------------------------------------------------------------------ stored values
def _inputs(torch, x):
    with np.errstate(over="ignore"):
        x16 = x.astype(np.float16)
    t = torch.from_numpy(x)
    return {
        "host_f32": (x, x),
        "host_f16": (x16, x16.astype(np.float32)),
        "host_bf16": (t.to(torch.bfloat16), t.to(torch.bfloat16).float().numpy()),
        "dev_f32": (t.cuda(), x),
        "dev_f16": (t.cuda().half(), t.half().float().numpy()),
        "dev_bf16": (t.cuda().bfloat16(), t.bfloat16().float().numpy()),
    }


@pytest.mark.parametrize("d", [64, 100, 768])
def test_reconstruct_equals_the_reference_every_input_dtype_host_and_device(d, torch_mod):
    for n in (1, 31, 32, 33, 1000):
        x = fm.wide_rows(n, d, seed=d + n)
        for name, (given, exact) in _inputs(torch_mod, x).items():
            idx = _fp4(d, given)
            assert idx.storage_dtype == "fp4" and idx.ntotal == n
            want = _want(exact, d)
            got = idx.reconstruct_n()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, n)
            if n == 1000:
                assert np.array_equal(idx.reconstruct_n(33, 100).view(np.uint32), want[33:133].view(np.uint32)), name
            idx.close()


@pytest.mark.parametrize("d", [64, 100, 768])
def test_normalize_quantises_the_f32_quotient(d, torch_mod):
    ix = _ix()
    g = np.random.default_rng(d)
    for n in (1, 31, 32, 33, 1000):
        x = (g.standard_normal((n, d)) * 3).astype(np.float32)
        for name, (given, _) in _inputs(torch_mod, x).items():
            ref = ix.FlatIPIndex(d, dtype="f32")
            ref.add(given, normalize=True)
            quotient = ref.reconstruct_n()
            ref.close()
            idx = _fp4(d, given, normalize=True)
            assert np.array_equal(idx.reconstruct_n().view(np.uint32), _want(quotient, d).view(np.uint32)), (name, n)
            idx.close()


@pytest.mark.parametrize("d", [64, 100, 768])
def test_three_adds_equal_one_add(d, torch_mod):
    x = fm.wide_rows(1000, d, seed=5)
    one = _fp4(d, x)
    three = _fp4(d)
    three.reserve(x.shape[0])
    for a, b in ((0, 33), (33, 64), (64, 1000)):             # 33 + 31 + 936 rows: cuts inside and at a row block
        three.add(torch_mod.from_numpy(x[a:b]).cuda() if a else x[a:b])
    assert np.array_equal(one.reconstruct_n().view(np.uint32), three.reconstruct_n().view(np.uint32))
    assert np.array_equal(one.reconstruct_n().view(np.uint32), _want(x, d).view(np.uint32))
    three.reset()
    assert three.ntotal == 0
    three.add(x[:40])
    assert np.array_equal(three.reconstruct_n().view(np.uint32), _want(x[:40], d).view(np.uint32))
    one.close()
    three.close()


# ------------------------------------------------------------------ scores to the bit
@pytest.mark.parametrize("B", [1, 33, 64, 65, 130])
@pytest.mark.parametrize("k", [1, 10, 1000, 2049])
@pytest.mark.parametrize("d", [64, 100, 768])
def test_search_equals_the_mirror_dense_corpus(pairs, d, B, k):
    p = pairs(N_DENSE, d)
    q = _queries(B, d, seed=B * 11 + k)
    _same(p.idx.search(q, k), p.mirror.search(fm.to_bf16_f32(q), k))
    assert p.idx.last_search_info()["path"] == "dense"


@pytest.mark.parametrize("B", [1, 33, 64, 65, 130])
@pytest.mark.parametrize("k", [1, 10, 1000, 2049])
@pytest.mark.parametrize("d", [64, 768])
def test_search_equals_the_mirror_filter_corpus(pairs, d, B, k):
    p = pairs(N_FILTER, d)
    q = _queries(B, d, seed=B * 7 + k)
    _same(p.idx.search(q, k), p.mirror.search(fm.to_bf16_f32(q), k))
    path = p.idx.last_search_info()["path"]
    # N = 40000: the filter path needs k <= 2048 and N >= 32 k; k = 2049 takes the dense path
    assert path == ("filter" if k <= 1000 else "dense"), path
    assert p.mirror.last_search_info()["path"] == path


def test_largest_dimensions_both_query_halves(torch_mod):
    # d = 2048: the image of 64 queries does not fit the LDS, so B = 64 runs as two 32-query passes
    for d, n, Bs in ((1024, 33_000, (20, 64)), (2048, 33_000, (20, 64))):
        p = Pair(n, d, seed=d)
        for B in Bs:
            q = _queries(B, d, seed=d + B)
            _same(p.idx.search(q, 10), p.mirror.search(fm.to_bf16_f32(q), 10))
            assert p.idx.last_search_info()["path"] == "filter"
            _same(p.idx.search(q, 10, exact_dense=True), p.mirror.search(fm.to_bf16_f32(q), 10, exact_dense=True))
        p.close()


def test_query_dtypes_are_rounded_to_bf16(pairs, torch_mod):
    torch = torch_mod
    for p in (pairs(N_FILTER, 64), pairs(N_DENSE, 100)):
        q = torch.from_numpy(_queries(40, p.d, seed=77)).cuda()
        for qt in (q, q.half(), q.bfloat16()):
            rounded = qt.bfloat16()                    # what the fp4 index does with any query dtype
            _same(p.idx.search(qt, 50), p.mirror.search(rounded, 50))
            _same(p.idx.search(qt, 50, exact_dense=True), p.mirror.search(rounded, 50, exact_dense=True))
        qh = _queries(5, p.d, seed=78).astype(np.float16)
        _same(p.idx.search(qh, 7), p.mirror.search(fm.to_bf16_f32(qh.astype(np.float32)), 7))


def test_scores_matrix(pairs, torch_mod):
    for p in (pairs(N_FILTER, 64), pairs(N_DENSE, 768)):
        q = _queries(33, p.d, seed=5)
        got, want = p.idx.scores(q), p.mirror.scores(fm.to_bf16_f32(q))
        assert got.shape == (33, p.n) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_async_finish_and_ignored_flags(pairs, torch_mod):
    torch = torch_mod
    big = pairs(N_FILTER, 768)
    q = torch.from_numpy(_queries(100, big.d, seed=9)).cuda()
    want = big.mirror.search(q.bfloat16(), 100)
    for kw in ({}, {"inputs_ready": True}, {"one_launch": True}):       # COALESCE / PIPELINE / ONE_LAUNCH: ignored
        D, I = big.idx.search(q, 100, async_=True, **kw)
        assert big.idx.finish() == []
        _same((D, I), want)
    _same(big.idx.search(q, 100, one_launch=True), want)
    info = big.idx.last_search_info()
    assert info["path"] == "filter" and info["one_launch"] is False
    # several asynchronous searches in flight, then one finish
    qs = [torch.from_numpy(_queries(b, big.d, seed=90 + b)).cuda() for b in (1, 33, 64)]
    outs = [big.idx.search(x, 10, async_=True) for x in qs]
    assert big.idx.finish() == []
    for x, o in zip(qs, outs):
        _same(o, big.mirror.search(x.bfloat16(), 10))


def test_id_offset(torch_mod):
    p = Pair(N_FILTER, 64, seed=21)
    p.idx.set_id_offset(7_000_000_000)
    p.mirror.set_id_offset(7_000_000_000)
    q = _queries(33, 64, seed=22)
    got = p.idx.search(q, 20)
    _same(got, p.mirror.search(fm.to_bf16_f32(q), 20))
    assert got[1].min() >= 7_000_000_000
    p.close()


def test_large_k_through_search_large_k(torch_mod):
    p = Pair(20_480, 64, seed=31)
    q = _queries(3, 64, seed=32)
    k = 20_000
    assert k > p.idx.MAX_KERNEL_K
    _same(p.idx.search(q, k), p.mirror.search(fm.to_bf16_f32(q), k))
    p.close()


@pytest.mark.parametrize("which", ["filter", "dense"])
def test_allowed_masks(which, pairs, torch_mod):
    p = pairs(N_FILTER, 768) if which == "filter" else pairs(N_DENSE, 100)
    g = np.random.default_rng(4)
    B = 40
    q = _queries(B, p.d, seed=41)
    qm = fm.to_bf16_f32(q)
    shared = g.random(p.n) < 0.3
    masks = [g.random(p.n) < 0.3, g.random(p.n) < 0.002, np.arange(p.n) % 97 == 0]
    per_q = [None if j % 4 == 3 else masks[j % 3] for j in range(B)]
    # filter: at most 32 queries take the masked scan's 32-query instantiation (OpFp4, WalkLiveFp4, QH = 1), 40 the other
    for b in ((7, 32, B) if which == "filter" else (B,)):
        _same(p.idx.search(q[:b], 25, allowed=shared), p.mirror.search(qm[:b], 25, allowed=shared))
        if which == "filter":
            info = p.idx.last_filter_info()
            assert info["filter_passes"] == 1 and info["dense_passes"] == 0   # the masked scan: one pass
            assert 0 < info["live_blocks"] <= info["total_blocks"] == (p.n + 31) // 32
        _same(p.idx.search(q[:b], 25, allowed=per_q[:b]), p.mirror.search(qm[:b], 25, allowed=per_q[:b]))
    _same(p.idx.search(q, 25, allowed=per_q, exact_dense=True), p.mirror.search(qm, 25, allowed=per_q, exact_dense=True))
    empty = np.zeros(p.n, dtype=bool)
    D, I = p.idx.search(q, 5, allowed=empty)
    assert (I == -1).all()
    _same((D, I), p.mirror.search(qm, 5, allowed=empty))
    few = np.zeros(p.n, dtype=bool)
    few[g.choice(p.n, size=9, replace=False)] = True                          # fewer allowed rows than k
    D, I = p.idx.search(q, 25, allowed=few)
    assert ((I >= 0).sum(axis=1) == 9).all()
    _same((D, I), p.mirror.search(qm, 25, allowed=few))
    tq = torch_mod.from_numpy(q).cuda()
    D, I = p.idx.search(tq, 25, allowed=shared, async_=True)
    p.idx.finish()
    _same((D, I), p.mirror.search(qm, 25, allowed=shared))


def test_ties_overflow_the_candidate_list(torch_mod):
    d = 64
    rows = fm.unit_rows(N_FILTER, d, seed=51)
    rows[10_000:30_000] = rows[10_000]                       # 20000 equal rows: more than the 16384 candidate slots
    idx = _fp4(d, rows)
    mirror = _mirror(idx)
    q = fm.clamp_queries(rows[10_000:10_001] + 0.01 * fm.unit_rows(1, d, 52))
    got = idx.search(q, 100)
    assert idx.last_search_info()["path"] == "filter+dense-fallback"
    _same(got, mirror.search(fm.to_bf16_f32(q), 100))
    assert np.array_equal(got[1][0], np.arange(10_000, 10_100))          # equal scores: ids ascending
    idx.close()
    mirror.close()


def test_grouped_search_is_search_plus_the_collapse(pairs, torch_mod):
    p = pairs(N_FILTER, 64)
    q = _queries(9, p.d, seed=55)
    groups = (np.arange(p.n) // 7).astype(np.int32)
    got = p.idx.search_grouped(q, 10, groups)
    want = p.mirror.search_grouped(fm.to_bf16_f32(q), 10, groups)
    _same(got[:2], want[:2])
    assert np.array_equal(_ids(got[2]), _ids(want[2]))


# ------------------------------------------------------------------ mutations against a fresh index
@pytest.mark.parametrize("d", [64, 768])
def test_remove_update_compact_add(d, torch_mod):
    n = N_FILTER
    rows = fm.unit_rows(n, d, seed=61)
    idx = _fp4(d, rows)
    q = _queries(40, d, seed=62)
    qm = fm.to_bf16_f32(q)
    top = np.unique(idx.search(q, 5)[1])
    gone = np.unique(np.concatenate([top, np.arange(64, 96), np.arange(0, n, 997)]))   # hits, a whole block, a stride
    assert idx.remove_ids(gone) == gone.size and idx.nlive == n - gone.size
    assert not np.isin(idx.search(q, 30)[1], gone).any()
    # update: a whole row block, scattered rows, host and device rows
    ids = np.setdiff1d(np.concatenate([np.arange(128, 160), np.array([1, 5000, 5001, n - 1])]), gone)
    new = fm.unit_rows(ids.size, d, seed=63) * np.float32(1.7)
    new[0] = q[0] / np.linalg.norm(q[0])                     # an updated row that has to enter the results
    idx.update_rows(ids, new)
    rows[ids] = new
    assert ids[0] in idx.search(q, 30)[1][0]
    ids2 = ids[::2]
    new2 = (fm.unit_rows(ids2.size, d, seed=64) * np.float32(0.3)).astype(np.float16)
    idx.update_rows(ids2, torch_mod.from_numpy(new2).cuda())
    rows[ids2] = new2.astype(np.float32)
    assert np.array_equal(idx.reconstruct_n().view(np.uint32), _want(rows, d).view(np.uint32))
    # searches with tombstones equal the mirror with the same tombstones
    mirror = _mirror(idx)
    mirror.remove_ids(gone)
    for kw in ({}, {"exact_dense": True}):
        _same(idx.search(q, 30, **kw), mirror.search(qm, 30, **kw))
    mirror.close()
    old2new = idx.compact()
    keep = np.setdiff1d(np.arange(n), gone)
    assert idx.ntotal == keep.size == idx.nlive and (old2new[gone] == -1).all()
    more = fm.unit_rows(1000 + 7, d, seed=65)
    idx.add(more)
    final = np.concatenate([rows[keep], more])
    fresh = _fp4(d, final)
    assert np.array_equal(idx.reconstruct_n().view(np.uint32), fresh.reconstruct_n().view(np.uint32))
    mirror = _mirror(fresh)
    for kw in ({}, {"exact_dense": True}):
        _same(idx.search(q, 30, **kw), mirror.search(qm, 30, **kw))
    assert idx.last_search_info()["path"] == "dense"
    _same(idx.search(q, 30), fresh.search(q, 30))
    for x in (idx, fresh, mirror):
        x.close()


# ------------------------------------------------------------------ planted relevance, decided by the model
def test_planted_rows_are_the_top_20():
    q, rows, planted = fm.planted_case()
    assert rows.shape == (N_FILTER, 64)
    idx = _fp4(64, rows)
    D, I = idx.search(q, 20)
    assert idx.last_search_info()["path"] == "filter"
    for j in range(q.shape[0]):
        assert np.array_equal(np.sort(I[j]), planted[j]), j
    idx.close()


# ------------------------------------------------------------------ retriever and pipeline
def _pipeline(tmp_path, sub, dtype="fp4", bm25=False, **extra):
    from test_pipeline_gpu import _build
    (tmp_path / sub).mkdir()
    return _build("cuda", tmp_path / sub, doubles=False, stage1_enable_bm25=bm25, stage1_index_dtype=dtype,
                  stage2_precompute_document_embeddings=True, stage3_cache_document_tokens=True, **extra)


PQ = ["neural networks attention", "language retrieval system", "gpu memory index", "token embedding search"]


def _stage1_equals_mirror(p, mirror, filter=None, allowed=None):
    s1 = p.stage1
    k = s1.config.top_k_candidates
    qt = s1._normalized_query_tensor(PQ)
    D, I = mirror.search(qt.bfloat16(), k) if allowed is None else mirror.search(qt.bfloat16(), k, allowed=allowed)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    for j, res in enumerate(s1.search_many(PQ, filter=filter)):
        keep = I[j] >= 0
        assert [r["doc_id"] for r in res] == I[j][keep].tolist()
        assert np.array_equal(np.array([r["stage1_score"] for r in res], dtype=np.float32).view(np.uint32),
                              D[j][keep].view(np.uint32))


def _same_results(a, b):
    for ra, rb in zip(a, b):
        for stage, key in (("stage1_results", "stage1_score"), ("stage2_results", "stage2_score"), ("results", "stage3_score")):
            assert [(r["doc_id"], r[key]) for r in ra[stage]] == [(r["doc_id"], r[key]) for r in rb[stage]], stage


def test_pipeline_with_an_fp4_stage1_index(tmp_path, torch_mod):
    from test_pipeline_gpu import _corpus
    docs = _corpus()
    p = _pipeline(tmp_path, "a")
    p.add_documents(docs)
    idx = p.stage1.faiss_index
    assert type(idx).__name__ == "FlatIPIndex" and idx.storage_dtype == "fp4" and idx.ntotal == len(docs)
    assert p.stage1.config.index_dtype == "fp4"
    mirror = _mirror(idx)
    _stage1_equals_mirror(p, mirror)
    assert all(len(p.search(q)["results"]) > 0 for q in PQ)
    keep = np.arange(len(docs)) % 3 != 0
    _stage1_equals_mirror(p, mirror, filter=keep, allowed=keep)
    with pytest.raises(NotImplementedError):
        p.stage1.range_search(PQ[0], 0.1)
    # save / load: the decoded rows quantise back to the same decoded values
    path = str(tmp_path / "saved" / "pipe.json")
    p.save_index(path)
    r = _pipeline(tmp_path, "b")
    r.load_index(path)
    jdx = r.stage1.faiss_index
    assert jdx.storage_dtype == "fp4" and jdx.ntotal == idx.ntotal
    assert np.array_equal(jdx.reconstruct_n().view(np.uint32), idx.reconstruct_n().view(np.uint32))
    _same_results(p.search_many(PQ), r.search_many(PQ))
    _same_results(p.search_many(PQ, filter=keep), r.search_many(PQ, filter=keep))
    mirror.close()


def test_pipeline_with_bm25_fusion_over_an_fp4_index(tmp_path, torch_mod):
    from test_pipeline_gpu import _corpus
    docs = _corpus()
    p = _pipeline(tmp_path, "a", bm25=True)
    p.add_documents(docs)
    assert p.stage1.faiss_index.storage_dtype == "fp4"
    keep = np.arange(len(docs)) % 3 != 0
    res = p.search_many(PQ)
    assert all(len(x["results"]) > 0 for x in res)
    for x in p.search_many(PQ, filter=keep):
        assert len(x["results"]) > 0 and all(keep[r["doc_id"]] for r in x["stage1_results"])
    path = str(tmp_path / "saved" / "pipe.json")
    p.save_index(path)
    r = _pipeline(tmp_path, "b", bm25=True)
    r.load_index(path)
    _same_results(res, r.search_many(PQ))


def test_ivf_retriever_keeps_its_rule_for_fp4(tmp_path, torch_mod):
    from test_pipeline_gpu import _corpus
    p = _pipeline(tmp_path, "ivf")
    c = p.stage1.config
    c.index_type, c.nlist, c.nprobe = "ivf", 8, 8
    p.add_documents(_corpus(120))
    assert type(p.stage1.faiss_index).__name__ == "IVFFlatIndex" and p.stage1.faiss_index.storage_dtype == "f16"


# ------------------------------------------------------------------ refusals
def test_refusals(torch_mod):
    ix = _ix()
    d = 64
    idx = _fp4(d, fm.unit_rows(100, d, 1))
    q = fm.unit_rows(2, d, 2)
    ids = np.arange(20, dtype=np.int64).reshape(2, 10)
    calls = {
        "range_search": lambda: idx.range_search(q, 0.5),
        "search_prefix": lambda: idx.search_prefix(q, 5, 32),
        "rescore": lambda: idx.rescore(q, ids),
        "search_funnel": lambda: idx.search_funnel(q, 5, 32),
        "search_biased": lambda: idx.search_biased(q, 5, np.zeros(100, np.float32)),
        "mmr": lambda: idx.mmr(ids, np.zeros((2, 10), np.float32), 3),
        "search_mmr": lambda: idx.search_mmr(q, 3),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match="fp4"):
            call()
    from tristage_rag_amd.sharded import ShardedFlatIPIndex
    with pytest.raises(NotImplementedError, match="fp4"):
        ShardedFlatIPIndex(d, 10, local_index=idx)
    with pytest.raises(NotImplementedError, match="fp4"):
        ShardedFlatIPIndex(d, 10, dtype="fp4")
    assert idx.fp8_scale_log2 is None
    _same(idx.search(q, 5), idx.search(q, 5))                 # the index is still usable
    idx.close()
    with pytest.raises(NotImplementedError, match="fp4"):
        ix.FlatIPIndex(2304, dtype="fp4")
    with pytest.raises(NotImplementedError, match="fp4"):
        ix.IVFFlatIndex(d, 4, dtype="fp4")
    ok = ix.FlatIPIndex(2048, dtype="fp4")
    ok.close()


# ------------------------------------------------------------------ the C level
def test_c_abi_create_add_search_with_host_pointers(torch_mod):
    from tristage_rag_amd import _lib
    lib = _lib.load()
    d, n, B, k = 100, N_DENSE, 5, 10
    h = ctypes.c_void_p()
    assert lib.ts_index_create(2304, _lib.TS_MXFP4_E2M1, 0, 0, ctypes.byref(h)) == _lib.TS_ERR_UNSUPPORTED
    assert "mxfp4" in _lib.last_error()
    assert lib.ts_index_create(d, _lib.TS_MXFP4_E2M1, 0, 0, ctypes.byref(h)) == _lib.TS_OK
    assert lib.ts_index_dtype(h) == _lib.TS_MXFP4_E2M1 and lib.ts_index_fp8_scale_log2(h) == -1
    rows = fm.unit_rows(n, d, seed=81)
    q = _queries(B, d, seed=82)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # the dtype is a storage dtype only: never a rows or query dtype
    assert lib.ts_index_add(h, P(rows), n, _lib.TS_MXFP4_E2M1, _lib.TS_FLAG_HOST_PTR, None) == _lib.TS_ERR_INVALID
    assert lib.ts_index_add(h, P(rows), n, _lib.TS_F32, _lib.TS_FLAG_HOST_PTR, None) == _lib.TS_OK
    D, I = np.empty((B, k), np.float32), np.empty((B, k), np.int64)
    assert lib.ts_index_search(h, P(q), B, _lib.TS_MXFP4_E2M1, k, P(D), P(I), _lib.TS_FLAG_HOST_PTR, None) == _lib.TS_ERR_INVALID
    assert lib.ts_index_search(h, P(q), B, _lib.TS_F32, k, P(D), P(I), _lib.TS_FLAG_HOST_PTR, None) == _lib.TS_OK
    rec = np.empty((n, d), np.float32)
    assert lib.ts_index_reconstruct(h, 0, n, P(rec), _lib.TS_FLAG_HOST_PTR, None) == _lib.TS_OK
    lims = np.zeros(B + 1, np.int64)
    rad = np.zeros(B, np.float32)
    assert lib.ts_index_range_search(h, P(q), B, _lib.TS_F32, P(rad), None, 0, 0, None, 0, P(lims),
                                     _lib.TS_FLAG_HOST_PTR, None) == _lib.TS_ERR_UNSUPPORTED
    assert "mxfp4" in _lib.last_error()
    assert lib.ts_index_destroy(h) == _lib.TS_OK
    want = _want(rows, d)
    assert np.array_equal(rec.view(np.uint32), want.view(np.uint32))
    # the host model of that search: float64 scores of the decoded rows against the bf16-rounded queries
    S = fm.to_bf16_f32(q).astype(np.float64) @ want.astype(np.float64).T
    for b in range(B):
        assert np.abs(D[b].astype(np.float64) - S[b][I[b]]).max() <= 1e-5
        assert np.abs(np.sort(S[b])[::-1][:k] - D[b]).max() <= 1e-5
