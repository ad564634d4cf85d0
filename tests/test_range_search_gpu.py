"""Range search on the GPU against the float64 model of tests/range_model.py: `lims`, the ids in
ascending order and the scores to the bit — `np.array_equal`, no tolerance — on exactly summable inputs, on the filter
path, at the candidate cap, on the dense path, for fp32 storage, with tombstones, masks and an id offset; and the path
each case took (tests/test_range_search_host.py fixes it from the model's counts)."""
import ctypes

import numpy as np
import pytest

import exact_inputs as ex
import range_model as rm
from helpers import make_corpus

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


def _flat(d, dtype, corpus):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_t(corpus, dtype))
    return idx


def _equal(got, want, what=""):
    lims, D, I = (_np(x) for x in got)
    lims0, D0, I0 = want
    assert lims.dtype == np.int64 and D.dtype == np.float32 and I.dtype == np.int64, what
    assert np.array_equal(lims, lims0), f"{what}: lims differ: got counts {np.diff(lims)[:8]} want {np.diff(lims0)[:8]}"
    bad = np.flatnonzero(I != I0)
    assert bad.size == 0, f"{what}: ids differ first at entry {bad[0]}: got {I[bad[0]]} want {I0[bad[0]]}"
    bad = np.flatnonzero(D != D0)
    assert bad.size == 0, f"{what}: scores differ first at entry {bad[0]}: got {D[bad[0]]!r} want {D0[bad[0]]!r}"
    assert np.array_equal(I, I0) and np.array_equal(D, D0)


def _check(idx, tq, corpus, queries, radius, dtype, d, live=None, allowed=None, exact_dense=False, what="", offset=0):
    """One range search against the model, and the path it took."""
    want = rm.expected_range(corpus, queries, radius, live=live, allowed=allowed, id_offset=offset)
    got = idx.range_search(tq, radius, allowed=allowed, exact_dense=exact_dense)
    _equal(got, want, what)
    masked = live is not None or (allowed is not None and any(a is not None for a in (
        allowed if isinstance(allowed, (list, tuple)) else [allowed])))
    paths = rm.expected_paths(corpus.shape[0], np.diff(want[0]), dtype, d, masked=masked, exact_dense=exact_dense)
    assert idx.last_range_info() == rm.info_of(paths), (what, idx.last_range_info(), paths)
    return want


def _tied_radius(corpus, queries, b):
    """A score of query b that at least two rows share, near the top of its list."""
    s = np.sort(ex.exact_scores(corpus, queries[b:b + 1])[0])[::-1]
    same = np.flatnonzero(s[1:] == s[:-1])
    same = same[same >= 50]
    assert same.size
    return np.float32(s[same[0]])


# ------------------------------------------------------------------------------------------------- 1: the filter path
@pytest.mark.parametrize("cls", ["ints", "neg"])
@pytest.mark.parametrize("dtype,d", [("f16", 128), ("f16", 768), ("bf16", 128), ("bf16", 768)])
def test_filter_path_is_exact(torch_mod, dtype, d, cls):
    """The filter scan with the radii as thresholds, then range_sort_kernel: per-query radii at ranks 1, 100 and 5000,
    a radius above every score, a radius on a tied score; no pass is redone densely."""
    n, B = ex.N_FILTER, 64
    corpus, queries = rm.guarded_case(cls, n, d, B)
    idx = _flat(d, dtype, corpus)
    tq = _t(queries, dtype)
    rank = np.array([1, 100, 5000])[np.arange(B) % 3]
    radius = rm.rank_radius(corpus, queries, rank)
    want = _check(idx, tq, corpus, queries, radius, dtype, d, what="ranks 1 / 100 / 5000")
    assert (np.diff(want[0]) >= rank).all() and idx.last_range_info()["dense_redo"] == 0
    # above every score: all lims equal, nothing stored
    top = np.float32(ex.exact_scores(corpus, queries).max() + 1)
    lims, D, I = idx.range_search(tq, top)
    assert _np(lims).tolist() == [0] * (B + 1) and D.numel() == 0 and I.numel() == 0
    # exactly on a tied score: the bound is inclusive, every row of the tie comes back
    radius = radius.copy()
    radius[0] = _tied_radius(corpus, queries, 0)
    want = _check(idx, tq, corpus, queries, radius, dtype, d, what="a tied radius")
    seg = want[1][want[0][0]:want[0][1]]
    assert (seg == radius[0]).sum() >= 2
    if cls == "ints" and dtype == "f16" and d == 128:
        # B = 33: two column halves, the second nearly empty; and numpy in -> numpy out
        q33 = np.ascontiguousarray(queries[:33])
        r33 = rm.rank_radius(corpus, q33, 100)
        _check(idx, _t(q33, dtype), corpus, q33, r33, dtype, d, what="B = 33")
        got = idx.range_search(q33, r33)
        assert all(isinstance(x, np.ndarray) for x in got)
        _equal(got, rm.expected_range(corpus, q33, r33), "host queries")
    idx.close()


# ---------------------------------------------------------------------------------------------------- 2: the cap edge
@pytest.mark.parametrize("d", [128, 768])
def test_candidate_cap_edge(torch_mod, d):
    """Radius at rank 16384: queries at exactly the cap and past it in one pass, which is redone densely and is exact
    for every query (the scan's counts past the cap equal the dense path's: the library checks it).  Then a pass whose
    counts are all <= 16384 with queries at exactly 16384: it stays on the filter path."""
    n, B, cap = ex.N_FILTER, 64, rm.CAND_CAP
    corpus, queries = rm.guarded_case("ints", n, d, B)
    idx = _flat(d, "f16", corpus)
    tq = _t(queries, "f16")
    radius = rm.rank_radius(corpus, queries, cap)
    want = _check(idx, tq, corpus, queries, radius, "f16", d, what="rank 16384")
    c = np.diff(want[0])
    assert (c == cap).any() and (c > cap).any()
    assert idx.last_range_info() == {"passes": 1, "filter_passes": 1, "dense_redo": 1}
    at = np.flatnonzero(c == cap)
    rank = np.where(np.isin(np.arange(B), at[:3]), cap, 100)
    want = _check(idx, tq, corpus, queries, rm.rank_radius(corpus, queries, rank), "f16", d, what="at the cap")
    assert np.diff(want[0]).max() == cap
    assert idx.last_range_info() == {"passes": 1, "filter_passes": 1, "dense_redo": 0}
    idx.close()


# --------------------------------------------------------------------------------------------------- 3: the dense path
@pytest.mark.parametrize("cls", ["ints", "neg"])
def test_dense_path_small_corpus(torch_mod, cls):
    n, d = ex.N_DENSE, 128
    corpus, queries = rm.guarded_case(cls, n, d, 65)
    idx = _flat(d, "f16", corpus)
    for B in (1, 65):
        q = np.ascontiguousarray(queries[:B])
        rank = np.array([1, 100, 1000])[np.arange(B) % 3]
        _check(idx, _t(q, "f16"), corpus, q, rm.rank_radius(corpus, q, rank), "f16", d, what=f"B={B}")
        want = _check(idx, _t(q, "f16"), corpus, q, -np.inf, "f16", d, what=f"B={B} -inf")
        assert np.diff(want[0]).tolist() == [n] * B
    idx.close()


def test_no_filter_flag_gives_the_filter_paths_result(torch_mod):
    n, d, B = ex.N_FILTER, 128, 64
    corpus, queries = rm.guarded_case("ints", n, d, B)
    idx = _flat(d, "f16", corpus)
    tq = _t(queries, "f16")
    radius = rm.rank_radius(corpus, queries, np.array([1, 100, 5000])[np.arange(B) % 3])
    a = idx.range_search(tq, radius)
    assert idx.last_range_info() == {"passes": 1, "filter_passes": 1, "dense_redo": 0}
    want = _check(idx, tq, corpus, queries, radius, "f16", d, exact_dense=True, what="TS_FLAG_NO_FILTER")
    _equal(a, want, "filter path")
    idx.close()


def test_dense_path_crosses_a_chunk_boundary(torch_mod):
    """(1 << 20) + 37 rows, two queries at -inf: the output of a query crosses the dense chunk boundary, and all N ids
    come back in order with their scores."""
    n, d = (1 << 20) + 37, 40
    corpus, queries, unit = ex.gen_ints(n, d, 2)
    ex.assert_exactly_summable(corpus, queries, unit)
    idx = _flat(d, "f16", corpus)
    lims, D, I = idx.range_search(_t(queries, "f16"), float("-inf"))
    assert _np(lims).tolist() == [0, n, 2 * n]
    I, D = _np(I), _np(D)
    assert np.array_equal(I, np.tile(np.arange(n, dtype=np.int64), 2))
    assert np.array_equal(D, ex.exact_scores(corpus, queries).astype(np.float32).reshape(-1))
    assert idx.last_range_info() == {"passes": 1, "filter_passes": 1, "dense_redo": 1}
    idx.close()


# -------------------------------------------------------------------------------------------------- 4: fp32 storage
@pytest.mark.parametrize("cls,d,B", [("ints", 64, 64), ("neg", 64, 64), ("A", 600, 70), ("C", 600, 70)])
def test_fp32_storage(torch_mod, cls, d, B):
    """("f32", 64, 64): the exact-f32 MFMA kernel; ("f32", 600, 70): the bf16x3 split scan over three passes."""
    n = ex.N_FILTER
    corpus, queries = rm.guarded_case(cls, n, d, B)
    idx = _flat(d, "f32", corpus)
    tq = _t(queries, "f32")
    rank = np.array([1, 100, 5000])[np.arange(B) % 3]
    _check(idx, tq, corpus, queries, rm.rank_radius(corpus, queries, rank), "f32", d, what="f32")
    assert idx.last_range_info()["passes"] == (3 if d == 600 else 1)
    idx.close()


# ---------------------------------------------------------------------------------------------------- 5: tombstones
@pytest.mark.parametrize("dense", [False, True])
def test_tombstones_compact_and_update(torch_mod, dense):
    n, d, B = ex.N_FILTER, 128, 64
    corpus, queries = rm.guarded_case("ints", n, d, B)
    idx = _flat(d, "f16", corpus)
    tq = _t(queries, "f16")
    gone = np.unique(np.concatenate([np.arange(0, n, 3), np.arange(64, 96), np.arange(32 * 700, 32 * 701)]))
    assert idx.remove_ids(gone) == gone.size
    live = np.ones(n, bool)
    live[gone] = False
    rank = np.array([1, 100, 5000])[np.arange(B) % 3]
    radius = rm.rank_radius(corpus, queries, rank, live=live)
    want = _check(idx, tq, corpus, queries, radius, "f16", d, live=live, exact_dense=dense, what="tombstones")
    assert not np.isin(want[2], gone).any() and not np.isin(_np(idx.range_search(tq, radius, exact_dense=dense)[2]), gone).any()
    # update some live rows in place: the new rows' scores are used
    ids = np.flatnonzero(live)[5:2000:7]
    src = np.flatnonzero(live)[::-1][: ids.size]
    corpus2 = corpus.copy()
    corpus2[ids] = corpus[src]
    idx.update_rows(ids, _t(corpus2[ids], "f16"))
    radius2 = rm.rank_radius(corpus2, queries, rank, live=live)
    _check(idx, tq, corpus2, queries, radius2, "f16", d, live=live, exact_dense=dense, what="after update_rows")
    # compact: the survivors with their new ids (the corpus is now below the filter path's floor: dense)
    old2new = idx.compact()
    assert idx.ntotal == int(live.sum()) and (old2new[gone] == -1).all()
    kept = np.ascontiguousarray(corpus2[live])
    _check(idx, tq, kept, queries, radius2, "f16", d, exact_dense=dense, what="after compact")
    idx.close()


# --------------------------------------------------------------------------------------------------------- 6: masks
@pytest.mark.parametrize("dtype,d", [("f16", 128), ("f32", 64)])
def test_masks_with_removals(torch_mod, dtype, d):
    """One mask per query, some queries unfiltered, some masks empty, combined with removed rows; on an fp32 index the
    pass goes dense, as its filtered top-k search does."""
    n, B = ex.N_FILTER, 64
    corpus, queries = rm.guarded_case("ints", n, d, B)
    idx = _flat(d, dtype, corpus)
    tq = _t(queries, dtype)
    rng = np.random.default_rng(5)
    masks = []
    for b in range(B):
        if b % 5 == 0:
            masks.append(None)
        elif b % 7 == 0:
            masks.append(np.zeros(n, bool))
        else:
            masks.append(rng.random(n) < (0.5 if b % 2 else 0.05))
    rank = np.array([1, 50, 1000])[np.arange(B) % 3]
    # masks alone
    s_rank = [1 if (m is not None and not m.any()) else r for m, r in zip(masks, rank)]
    radius = rm.rank_radius(corpus, queries, np.array(s_rank), allowed=masks)
    radius = np.where(np.isfinite(radius), radius, np.float32(0)).astype(np.float32)   # (an empty mask has no rank)
    _check(idx, tq, corpus, queries, radius, dtype, d, allowed=masks, what="masks")
    # masks ANDed with the live set
    gone = np.arange(1, n, 4)
    assert idx.remove_ids(gone) == gone.size
    live = np.ones(n, bool)
    live[gone] = False
    want = _check(idx, tq, corpus, queries, radius, dtype, d, live=live, allowed=masks, what="masks and removals")
    c = np.diff(want[0])
    assert all(c[b] == 0 for b in range(B) if masks[b] is not None and not masks[b].any()) and c.max() > 0
    idx.close()


# ----------------------------------------------------------------------------------------------------- 7: id offset
def test_id_offset(torch_mod):
    n, d, B = ex.N_FILTER, 128, 64
    corpus, queries = rm.guarded_case("ints", n, d, B)
    idx = _flat(d, "f16", corpus)
    idx.set_id_offset(1000)
    tq = _t(queries, "f16")
    radius = rm.rank_radius(corpus, queries, 100)
    for dense in (False, True):
        want = _check(idx, tq, corpus, queries, radius, "f16", d, exact_dense=dense, offset=1000, what=f"dense={dense}")
        assert want[2].min() >= 1000
    idx.close()


# ------------------------------------------------------------------------------------------------- 8: against search
def test_sorted_range_equals_search(torch_mod):
    torch = torch_mod
    n, d, B, k = 40_000, 128, 8, 100
    corpus = make_corpus(n, d, dtype="f16")
    idx = _flat(d, "f16", corpus)
    tq = torch.from_numpy(make_corpus(B, d, seed=77, dtype="f16")).cuda().half()
    D, I = idx.search(tq, k)
    lims, Dr, Ir = idx.range_search(tq, D[:, k - 1], sort=True)
    lims = _np(lims)
    assert (np.diff(lims) >= k).all()
    for b in range(B):
        assert torch.equal(Dr[lims[b]: lims[b] + k], D[b]) and torch.equal(Ir[lims[b]: lims[b] + k], I[b])
        seg = Dr[lims[b]: lims[b + 1]]
        assert bool((seg[1:] <= seg[:-1]).all())
    # the same from host queries: numpy sort
    ln, Dn, In = idx.range_search(tq.cpu().numpy(), D[:, k - 1].cpu().numpy(), sort=True)
    assert np.array_equal(ln, lims) and np.array_equal(Dn, _np(Dr)) and np.array_equal(In, _np(Ir))
    idx.close()


# -------------------------------------------------------------------------------------------------- 9: before and after
def test_searches_before_and_after_a_range_search_are_identical(torch_mod):
    torch = torch_mod
    n, d, B = 40_000, 128, 64
    idx = _flat(d, "f16", make_corpus(n, d, dtype="f16"))
    tq = torch.from_numpy(make_corpus(B, d, seed=78, dtype="f16")).cuda().half()
    mask = np.random.default_rng(3).random(n) < 0.3
    before = idx.search(tq, 100), idx.search(tq, 100, allowed=mask), idx.search(tq, 100, classic=True)
    for radius in (float(before[0][0][:, 50].min()), float("-inf")):          # the filter path, then a dense redo
        idx.range_search(tq[:8], radius)
        idx.range_search(tq[:8], radius, allowed=mask)
        after = idx.search(tq, 100), idx.search(tq, 100, allowed=mask), idx.search(tq, 100, classic=True)
        for (D0, I0), (D1, I1) in zip(before, after):
            assert torch.equal(D0, D1) and torch.equal(I0, I1)
    idx.close()


# ------------------------------------------------------------------------------------------- 10, 11: limit and capacity
def test_result_limit_and_fetch_capacity(torch_mod):
    from tristage_rag_amd import _lib
    from tristage_rag_amd.index import RangeSearchLimitError
    n, d, B = ex.N_FILTER, 128, 70
    corpus, queries = rm.guarded_case("ints", n, d, B)
    idx = _flat(d, "f16", corpus)
    tq = _t(queries, "f16")
    radius = rm.rank_radius(corpus, queries, 100)
    want = rm.expected_range(corpus, queries, radius)
    total = int(want[0][-1])
    for dense in (False, True):
        with pytest.raises(RangeSearchLimitError, match=rf"{total} results so far exceed the limit of {total - 1}") as e:
            idx.range_search(tq, radius, max_results=total - 1, exact_dense=dense)
        assert e.value.counts.sum() == total                 # the last pass's counts were known when it was refused
        # nothing is stored behind a refused call
        out = ctypes.c_void_p(4096)
        assert idx._lib.ts_index_range_fetch(idx._h, out, out, 1 << 30, 0, None) == _lib.TS_ERR_INVALID
        _equal(idx.range_search(tq, radius, max_results=total, exact_dense=dense), want, "enough room")
    # the limit in the first of two passes: the second pass never runs, its counts stay zero
    first = int(want[0][64])
    with pytest.raises(RangeSearchLimitError) as e:
        idx.range_search(tq, radius, max_results=first - 1)
    assert e.value.counts[:64].sum() == first and e.value.counts[64:].sum() == 0
    _equal(idx.range_search(tq, radius), want, "the index stays usable")
    # fetch: a capacity that is too small
    import torch
    Ds = torch.empty(total, dtype=torch.float32, device="cuda")
    Is = torch.empty(total, dtype=torch.int64, device="cuda")
    fetch = lambda cap: idx._lib.ts_index_range_fetch(idx._h, ctypes.c_void_p(Ds.data_ptr()), ctypes.c_void_p(Is.data_ptr()),
                                                      cap, 0, None)
    assert fetch(total - 1) == _lib.TS_ERR_INVALID and "capacity" in _lib.last_error()
    assert fetch(total) == _lib.TS_OK
    assert np.array_equal(_np(Ds), want[1]) and np.array_equal(_np(Is), want[2])
    # a change of the index drops the stored result
    assert idx.remove_ids([0]) == 1
    assert fetch(total) == _lib.TS_ERR_INVALID
    idx.close()


# ---------------------------------------------------------------------------------------------- 12: Stage1Retriever
def test_stage1_retriever_range_search(tmp_path):
    from tristage_rag_amd.encoders import SentenceEncoder
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    enc = SentenceEncoder("random:tiny", device="cuda")
    docs = [f"document number {i} about topic {i % 7} and subject {i % 11}" for i in range(300)]
    meta = [{"tenant": "a" if i % 3 else "b", "i": i} for i in range(300)]
    cfg = dict(model_name="random:tiny", device="cuda", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
               use_fp16=False, index_dtype="f16", enable_bm25=False)
    s1 = Stage1Retriever(Stage1Config(**cfg), model=enc)
    s1.add_documents(docs, meta)
    queries = ["document about topic 3", "subject 5 of some document"]

    def brute(query, min_score, allowed):
        S = s1.faiss_index.scores(s1._normalized_query_tensor([query]))[0].cpu().numpy()
        ok = S >= np.float32(min_score)
        if allowed is not None:
            ok &= allowed
        ids = np.flatnonzero(ok)
        order = np.lexsort((ids, -S[ids].astype(np.float64)))
        return [(int(i), float(S[i])) for i in ids[order]]

    S0 = s1.faiss_index.scores(s1._normalized_query_tensor(queries[:1]))[0].cpu().numpy()
    min_score = float(np.sort(S0)[-20])
    got = s1.range_search(queries[0], min_score)
    assert [(r["doc_id"], r["score"]) for r in got] == brute(queries[0], min_score, None) and len(got) >= 20
    assert all(r["document"] == docs[r["doc_id"]] and r["metadata"] == meta[r["doc_id"]] and r["stage"] == "stage1"
               and r["stage1_score"] == r["score"] for r in got)
    # a list of queries, a dict filter
    tenant_a = np.array([m["tenant"] == "a" for m in meta])
    many = s1.range_search(queries, min_score, filter={"tenant": "a"})
    assert [[(r["doc_id"], r["score"]) for r in rs] for rs in many] == [brute(q, min_score, tenant_a) for q in queries]
    assert all(meta[r["doc_id"]]["tenant"] == "a" for rs in many for r in rs)
    # removed documents never come back
    gone = [r["doc_id"] for r in got[:5]]
    assert s1.remove_documents(gone) == 5
    live = np.ones(300, bool)
    live[gone] = False
    got2 = s1.range_search(queries[0], min_score)
    assert [(r["doc_id"], r["score"]) for r in got2] == brute(queries[0], min_score, live)
    got3 = s1.range_search(queries[0], min_score, filter={"tenant": "a"})
    assert [(r["doc_id"], r["score"]) for r in got3] == brute(queries[0], min_score, live & tenant_a)
    with pytest.raises(Exception, match="exceed the limit"):
        s1.range_search(queries[0], -1.0, max_results=10)
    # an IVF retriever has no range search
    ivf = Stage1Retriever(Stage1Config(**dict(cfg, index_type="ivf", nlist=4, index_dir=str(tmp_path / "j"))), model=enc)
    ivf.add_documents(docs, meta)
    with pytest.raises(NotImplementedError):
        ivf.range_search(queries[0], min_score)
