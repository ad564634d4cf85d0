"""The BM25 model (tests/bm25_model.py) against the reference's recorded outputs and the host BM25Index, and every
constructed input of tests/test_bm25_kernels_gpu.py against the property it is built for.  No GPU."""
import json
import os

import numpy as np
import pytest

import bm25_cases as bc
import bm25_model as bm

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kat.json")))


def _model_of(index):
    """The CSR BM25Index.fit built -> the model's index and the term ids."""
    terms, off, docs, tfs, idf, ln = index._csr()
    nnz = int(off[-1])
    ix = bm.Csr(index.corpus_size, off, docs[:nnz], tfs[:nnz], idf[:len(terms)], ln[:index.corpus_size], index.k1 + 1)
    return ix, {t: i for i, t in enumerate(terms)}


def _ids_of(index, tid, query):
    return [tid[t] for t in index.tokenize(query) if t in tid]


def _same(got, want):
    ids, scores = got
    assert ids.tolist() == [i for i, _ in want]
    assert scores.view(np.uint64).tolist() == np.array([s for _, s in want], np.float64).view(np.uint64).tolist()


def test_model_reproduces_the_reference_outputs():
    from tristage_rag_amd.stage1_retriever import BM25Index
    b = KAT["bm25"]
    idx = BM25Index()
    idx.fit(b["documents"])
    ix, tid = _model_of(idx)
    for q, want in zip(b["queries"], b["search_top5"]):
        _same(bm.search_all(ix, _ids_of(idx, tid, q), 5), want)


def test_model_reproduces_the_reference_outputs_after_a_second_fit():
    from tristage_rag_amd.stage1_retriever import BM25Index
    b = KAT["bm25_refit"]
    idx = BM25Index(refit_compat=True)
    idx.fit(list(b["first"]))
    idx.fit(list(b["first"]) + list(b["second"]))
    ix, tid = _model_of(idx)
    for q, want in zip(b["queries"], b["search_top6"]):
        _same(bm.search_all(ix, _ids_of(idx, tid, q), 6), want)


def test_model_equals_host_index_on_random_queries_with_masks():
    from tristage_rag_amd.stage1_retriever import BM25Index
    rng = np.random.default_rng(21)
    vocab = [f"w{i}" for i in range(120)]
    p = 1.0 / np.arange(1, 121)
    p /= p.sum()
    docs = [" ".join(rng.choice(vocab, size=int(rng.integers(1, 30)), p=p)) for _ in range(700)]
    idx = BM25Index()
    idx.fit(docs)
    ix, tid = _model_of(idx)
    for qi in range(300):
        q = " ".join(rng.choice(vocab + ["nosuch"], size=int(rng.integers(0, 9))))
        k = int(rng.choice([1, 7, 100, 700, 900]))
        allowed = None if qi % 3 == 0 else rng.random(len(docs)) < (0.02, 0.5)[qi % 2]
        _same(bm.search_all(ix, _ids_of(idx, tid, q), k, allowed), idx.search(q, k, allowed=allowed))
        # the C-level list is the touched part of the full ranking while scores stay above 0.0
        ids, scores, n = bm.search(ix, _ids_of(idx, tid, q), k, allowed)
        full = bm.search_all(ix, _ids_of(idx, tid, q), k, allowed)
        assert (scores > 0).all() and ids.tolist() == full[0][:n].tolist() and (full[1][n:] == 0.0).all()


def test_scalar_loop_equals_the_vectorised_model():
    c = bc.arithmetic_case()
    for s in c.searches[:6]:
        a, ta = bm.accumulate(c.ix, s.terms)
        b, tb = bm.accumulate_scalar(c.ix, s.terms)
        assert a.view(np.uint64).tolist() == b.view(np.uint64).tolist() and ta.tolist() == tb.tolist()
    ix, masks = bc.mask_case()
    a, ta = bm.accumulate(ix, [29, 3, 3, 7], masks[5])
    b, tb = bm.accumulate_scalar(ix, [29, 3, 3, 7], masks[5])
    assert a.view(np.uint64).tolist() == b.view(np.uint64).tolist() and ta.tolist() == tb.tolist()
    n = bc.negative_case()
    for s in n.searches:
        a, _ = bm.accumulate(n.ix, s.terms)
        b, _ = bm.accumulate_scalar(n.ix, s.terms)
        assert a.view(np.uint64).tolist() == b.view(np.uint64).tolist()


# ---- the constructed inputs keep their properties --------------------------------------------------------------------
def _check_properties(case):
    ix = case.ix
    for s in case.searches:
        n, ties, byte = bm.boundary(ix, s.terms, s.k)
        assert s.k <= bm.MAX_K
        if s.touched is not None:
            assert n == s.touched, (s, n)
        if s.ties is not None:
            assert ties == s.ties, (s, ties)
        if s.byte is not None:
            assert byte == s.byte, (s, byte)
        total = ix.total(s.terms)
        if s.path == "short":
            assert n <= bm.PRE_MIN
        elif s.path == "direct":
            assert total <= bm.PRE_MIN
        elif s.path == "skip":
            assert total > bm.PRE_MIN and n <= bm.PRE_MIN
        elif s.path == "cand":
            assert total > bm.PRE_MIN and bm.PRE_MIN < n <= bm.CAND_CAP
            assert -(-4 * s.k * 4096 // n) >= s.k
        elif s.path == "overflow":
            # the threshold is the m-th best sampled key and fewer than m documents score above the tied level, so
            # it is the tied level's key and the whole level (more than CAND_CAP documents) passes the filter
            acc, touched = bm.accumulate(ix, s.terms)
            level = acc[bm.ranked(acc, np.flatnonzero(touched))[s.k - 1]]
            above = int((acc[touched] > level).sum())
            m = min(4096, max(8, -(-4 * s.k * 4096 // n)))
            assert total > bm.PRE_MIN and n > bm.CAND_CAP and above < m and ties > bm.CAND_CAP
            assert int((acc[touched] < level).sum()) == 0        # nothing below it in the sample either
        else:
            assert s.path is None


@pytest.mark.parametrize("byte", range(8))
def test_score_byte_inputs(byte):
    cases = bc.score_byte_case(byte)
    assert [c.searches[0].k for c in cases] == list(bc.KS_RADIX)
    for c in cases:
        _check_properties(c)
        acc, _ = bm.accumulate(c.ix, c.searches[0].terms)
        pats = np.zeros(c.ix.N, dtype=np.int64)
        for t in range(bc.PLANTED_TERMS):
            pats[c.ix.postings(t)[0]] |= 1 << t
        assert acc.view(np.uint64).tolist() == bc.planted_scores(pats).view(np.uint64).tolist()     # planted sums: exact
        back, _ = bm.accumulate(c.ix, c.searches[0].terms[::-1])
        assert acc.view(np.uint64).tolist() == back.view(np.uint64).tolist()                        # ... in any order


def test_short_list_inputs():
    _check_properties(bc.short_list_case())
    assert all(s.touched <= s.k for s in bc.short_list_case().searches)


@pytest.mark.parametrize("byte", sorted(bc.ID_TIE_SHAPES))
def test_id_byte_inputs(byte):
    N, X = bc.ID_TIE_SHAPES[byte]
    for c in bc.id_tie_case(N, X):
        assert c.searches[0].byte == byte
        _check_properties(c)
        ids, scores, n = bm.search(c.ix, c.searches[0].terms, c.searches[0].k + 1)
        assert ids[-2:].tolist() == [X - 1, X] and scores[-2:].tolist() == [1.0, 1.0]


def test_top_id_byte_input():
    (c,) = bc.id_tie_case.__wrapped__(**bc.TOP_ID_BYTE)      # (not cached: 200 MB)
    s = c.searches[0]
    assert s.byte == 8 and c.ix.N > 1 << 24
    acc, touched = bm.accumulate(c.ix, s.terms)      # (ranked from the touched documents: no sort over 2^24 rows)
    order = bm.ranked(acc, np.flatnonzero(touched))
    assert len(order) == s.touched and order[s.k - 1] == (1 << 24) - 1 and order[s.k] == 1 << 24
    assert bm.first_diff_byte(bm.key96(acc[order[s.k - 1]], order[s.k - 1]), bm.key96(acc[order[s.k]], order[s.k])) == 8


@pytest.mark.parametrize("name", bc.PREFILTER_CASES)
def test_prefilter_inputs(name):
    c = bc.prefilter_case(name)
    assert [s.k for s in c.searches[:3]] == list(bc.KS_PRE)
    _check_properties(c)


def test_two_level_inputs_hold_fewer_than_k_above_the_tied_level():
    for name in ("two_level_12000", "two_level_17000"):
        c = bc.prefilter_case(name)
        for s in c.searches:
            acc, touched = bm.accumulate(c.ix, s.terms)
            assert sorted(set(acc[touched].tolist())) == [1.0, 2.0] and int((acc == 2.0).sum()) == 100
            if s.k > 1:
                assert 100 < s.k and s.ties == int(name[-5:])


def test_arithmetic_input_spans_what_it_says():
    c = bc.arithmetic_case()
    ix = c.ix
    tf = ix.post_tf
    assert (tf == np.float32(1e-3)).any() and (tf == np.float32(1e6)).any() and (tf != np.round(tf)).any()
    assert ix.len_norm.min() < 2e-3 and ix.len_norm.max() > 5e2
    assert ix.idf.min() < 1e-300 and ix.idf.max() >= 1e300 and (ix.idf > 0).all()
    assert max(len(s.terms) for s in c.searches) == 40 and any(len(set(s.terms)) < len(s.terms) for s in c.searches)
    subnormal = huge = 0
    tiny = np.finfo(np.float64).tiny
    for s in c.searches:
        acc, touched = bm.accumulate(ix, s.terms)
        assert np.isfinite(acc).all() and (acc[touched] > 0).all()       # no product rounds to zero, nothing overflows
        subnormal += int(((acc > 0) & (acc < tiny)).sum())
        huge += int((acc > 1e299).sum())
    assert subnormal > 50 and huge > 50


def test_lane_batches():
    c = bc.lanes_case()
    assert [len(b) for b in c.searches] == [1, 63, 64, 65, 130, 1]
    long_terms = [t for t in range(c.ix.V) if c.ix.term_off[t + 1] - c.ix.term_off[t] > bm.PRE_MIN]
    assert len(long_terms) == 3
    for b in c.searches[1:5]:
        assert b[1] == [] and c.ix.total(b[0]) > bm.PRE_MIN and c.ix.total(b[2]) > bm.PRE_MIN      # empty between long
        assert any(0 < c.ix.total(q) <= bm.PRE_MIN for q in b)
        assert b[-1] == b[0] and len({tuple(q) for q in b}) < len(b)                               # repeats in other lanes
    big = c.searches[4]
    assert big[0] == big[129] and any(c.ix.total(q) > bm.PRE_MIN for q in big[64:128])


def test_mask_inputs():
    ix, masks = bc.mask_case()
    assert ix.N % 32 != 0
    assert [np.flatnonzero(m).tolist() for m in masks[:4]] == [[31], [32], [ix.N - 1], []] and masks[4].all()
    words = (ix.N + 31) // 32 + 2
    packed = bc.pack_masks(masks, words)
    for m, row in zip(masks, packed):
        assert [bool((row[d >> 5] >> (d & 31)) & 1) for d in range(ix.N)] == m.tolist()
    for m in masks[:3]:        # the one allowed document is in the postings of the term everyone holds
        assert bm.search(ix, [ix.V - 1], 5, m)[2] == 1


def test_negative_inputs():
    c = bc.negative_case()
    _check_properties(c)
    acc, touched = bm.accumulate(c.ix, [3])
    assert (acc[touched] < 0).all() and (~touched).sum() == 390
    acc, touched = bm.accumulate(c.ix, [0, 1])
    back = np.flatnonzero(touched & (acc == 0.0))
    assert back.tolist() == list(range(50, 100)) and not np.signbit(acc[back]).any()
    acc3, _ = bm.accumulate(c.ix, [0, 1, 2])
    assert (acc3[60:70] == 0.5).all() and (acc3[70:100] == 0.0).all()
    # the C-level list (touched only) and the full ranking differ here: what the host path of BM25Index is for
    ids, _, n = bm.search(c.ix, [3], 5)
    assert n == 5 and ids.tolist() == [300, 301, 302, 303, 304]
    assert bm.search_all(c.ix, [3], 5)[0].tolist() == [0, 1, 2, 3, 4]


def test_refit_compat_example_has_a_negative_idf():
    from tristage_rag_amd.stage1_retriever import BM25Index
    first, second = ["alpha"] * 5 + ["x y"], ["zeta eta"]
    idx = BM25Index(refit_compat=True)
    idx.fit(first)
    idx.fit(first + second)
    assert idx.idf["alpha"] < -0.27
    got = idx.search("alpha", 3)
    assert [i for i, _ in got] == [5, 0, 1] and got[0][1] == 0.0 and got[1][1] < -0.33
    ix, tid = _model_of(idx)
    _same(bm.search_all(ix, [tid["alpha"]], 3), got)
