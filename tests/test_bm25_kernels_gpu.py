"""ts_bm25.hip through the C API against the float64 model of tests/bm25_model.py, on the constructed inputs of
tests/bm25_cases.py ("BM25 kernels against a model"): ids, float64 scores and n_out bit for bit.  The
tokenizer and BM25Index stay out of it except in the last tests, which hold the GPU index to the host index where the
C-level contract alone does not give the host's list (non-positive idf, top_k above 2048)."""
import ctypes

import numpy as np
import pytest

import bm25_cases as bc
import bm25_model as bm

pytestmark = pytest.mark.gpu


class Handle:
    """One ts_bm25 handle; every call returns [(ids int64 [n_out], scores float64 [n_out], n_out)] per query."""

    def __init__(self, ix=None):
        from tristage_rag_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.ts_bm25_create(0, ctypes.byref(self.h)))
        if ix is not None:
            self.set_index(ix)

    def set_index(self, ix):
        p = (lambda a: a.ctypes.data if a.size else None)
        self._lib.check(self.lib.ts_bm25_set_index(self.h, ix.N, ix.V, ix.nnz, ix.term_off.ctypes.data, p(ix.post_doc),
                                                   p(ix.post_tf), p(ix.idf), p(ix.len_norm), ix.k1p1))

    def close(self):
        if self.h:
            self.lib.ts_bm25_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _flat(queries):
        off = np.zeros(len(queries) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(q) for q in queries])
        flat = np.array([t for q in queries for t in q] or [0], dtype=np.int32)
        return flat, off

    @staticmethod
    def _rows(out_s, out_i, n_out):
        return [(out_i[q, :n_out[q]].copy(), out_s[q, :n_out[q]].copy(), int(n_out[q])) for q in range(len(n_out))]

    def search(self, terms, k):
        t = np.array(list(terms) or [0], dtype=np.int32)
        out_s, out_i = np.full((1, k), np.nan), np.full((1, k), -7, dtype=np.int64)
        n = ctypes.c_int32(-1)
        self._lib.check(self.lib.ts_bm25_search(self.h, t.ctypes.data, len(terms), k, out_s.ctypes.data, out_i.ctypes.data,
                                                ctypes.byref(n), None))
        return self._rows(out_s, out_i, [n.value])[0]

    def batch_code(self, queries, k, masks=None, mask_of_query=None, words=0, flags=0, bits_ptr=None):
        """(return code, rows).  masks: packed uint32 [n_masks, words] (host) unless bits_ptr (device) is given."""
        flat, off = self._flat(queries)
        nq = len(queries)
        out_s, out_i = np.full((max(nq, 1), k), np.nan), np.full((max(nq, 1), k), -7, dtype=np.int64)
        n_out = np.full(max(nq, 1), -1, dtype=np.int32)
        if mask_of_query is None:
            rc = self.lib.ts_bm25_search_batch(self.h, flat.ctypes.data, off.ctypes.data, nq, k, out_s.ctypes.data,
                                               out_i.ctypes.data, n_out.ctypes.data, None)
        else:
            moq = np.asarray(mask_of_query, dtype=np.int32)
            n_masks = 0 if masks is None else len(masks)
            ptr = bits_ptr if bits_ptr is not None else (masks.ctypes.data if n_masks else None)
            rc = self.lib.ts_bm25_search_batch_filtered(self.h, flat.ctypes.data, off.ctypes.data, nq, k, ptr, words, n_masks,
                                                        moq.ctypes.data, flags, out_s.ctypes.data, out_i.ctypes.data,
                                                        n_out.ctypes.data, None)
        return rc, (self._rows(out_s, out_i, n_out[:nq]) if rc == 0 else None)

    def batch(self, queries, k, **kw):
        rc, rows = self.batch_code(queries, k, **kw)
        self._lib.check(rc)
        return rows


def _assert_same(got, want, what):
    gi, gs, gn = got
    wi, ws, wn = want
    assert gn == wn, f"{what}: n_out {gn}, the model {wn}"
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, (f"{what}: {bad.size} ids differ, first at rank {bad[0]}: got {gi[bad[0]]} "
                           f"(score {gs[bad[0]]!r}), the model {wi[bad[0]]} ({ws[bad[0]]!r})")
    bad = np.flatnonzero(gs.view(np.uint64) != np.asarray(ws, np.float64).view(np.uint64))
    assert bad.size == 0, (f"{what}: {bad.size} scores differ, first at rank {bad[0]} (doc {gi[bad[0]]}): "
                           f"got {float(gs[bad[0]]).hex()}, the model {float(ws[bad[0]]).hex()}")


def _run_case(case, what):
    with Handle(case.ix) as h:
        for s in case.searches:
            _assert_same(h.search(s.terms, s.k), bm.search(case.ix, s.terms, s.k), f"{what} k={s.k} terms={s.terms}")


# ---- 1. radix passes 0-7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", range(8))
def test_boundary_in_each_score_byte(byte):
    for case in bc.score_byte_case(byte):
        _run_case(case, f"score byte {byte}")


def test_k_above_the_touched_count():
    _run_case(bc.short_list_case(), "short list")


# ---- 2. id passes 8-11 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", sorted(bc.ID_TIE_SHAPES))
def test_boundary_in_each_id_byte(byte):
    for case in bc.id_tie_case(*bc.ID_TIE_SHAPES[byte]):
        _run_case(case, f"id byte {byte}")


def test_boundary_in_the_top_id_byte():
    """N = 2^24 + 64: for a smaller N every document shares the top id byte."""
    (case,) = bc.id_tie_case.__wrapped__(**bc.TOP_ID_BYTE)      # (not cached: 200 MB)
    _run_case(case, "id byte 8")


# ---- 3. pre-filter boundaries -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.PREFILTER_CASES)
def test_prefilter_boundaries(name):
    _run_case(bc.prefilter_case(name), name)


# ---- 4. accumulation arithmetic -----------------------------------------------------------------------------------------
def test_accumulation_arithmetic():
    case = bc.arithmetic_case()
    with Handle(case.ix) as h:
        for k in (10, 300, 2048):
            group = [s for s in case.searches if s.k == k]
            rows = h.batch([s.terms for s in group], k)
            for s, got in zip(group, rows):
                want = bm.search(case.ix, s.terms, k)
                _assert_same(got, want, f"arithmetic (batch) terms={s.terms}")
                _assert_same(h.search(s.terms, k), want, f"arithmetic (single) terms={s.terms}")


# ---- 5. lanes and chunks ------------------------------------------------------------------------------------------------
def test_lanes_and_chunks():
    case = bc.lanes_case()
    k = 300
    want = {}
    with Handle(case.ix) as h:
        for batch in case.searches:            # 1, 63, 64, 65, 130 and 1 again: lanes grow, then the wider workspace is reused
            rows = h.batch(batch, k)
            assert len(rows) == len(batch)
            for qi, (q, got) in enumerate(zip(batch, rows)):
                key = tuple(q)
                if key not in want:
                    want[key] = bm.search(case.ix, q, k)
                _assert_same(got, want[key], f"batch of {len(batch)}, query {qi} terms={q}")
        for key in want:
            _assert_same(h.search(list(key), k), want[key], f"single query terms={list(key)}")
        assert h.batch([], k) == []


# ---- 6. state left clean ------------------------------------------------------------------------------------------------
def test_a_rejected_batch_leaves_the_handle_clean():
    from tristage_rag_amd import _lib
    case = bc.lanes_case()
    ix, k = case.ix, 300
    good = case.searches[4][:80]
    with Handle(ix) as h:
        h.batch(good[:64], k)                                  # 64 lanes: the 70th query is in the second chunk
        for bad_id in (ix.V, -1):
            bad = [list(q) for q in good]
            bad[69] = [ix.V - 1, bad_id]                       # rejected on the host between the two chunks' launches
            rc, _ = h.batch_code(bad, k)
            assert rc == _lib.TS_ERR_INVALID and "out of range" in _lib.last_error()
            for q, got in zip(good, h.batch(good, k)):
                _assert_same(got, bm.search(ix, q, k), f"after a rejected batch, terms={q}")
        assert h.batch_code(good, bm.MAX_K + 1)[0] == _lib.TS_ERR_UNSUPPORTED
        _assert_same(h.search(good[0], k), bm.search(ix, good[0], k), "after an unsupported k")


def test_set_index_empty_and_twice():
    a, b = bc.short_list_case().ix, bc.negative_case().ix
    empty_corpus = bm.from_postings(0, [[], []], [1.0, 2.0], np.zeros(0))
    no_postings = bm.from_postings(50, [[], [], []], [1.0, 2.0, 3.0])
    with Handle(empty_corpus) as h:
        assert h.search([0, 1], 5)[2] == 0 and [r[2] for r in h.batch([[0], [], [1, 1]], 5)] == [0, 0, 0]
        h.set_index(no_postings)
        assert h.search([0, 2], 5)[2] == 0 and [r[2] for r in h.batch([[0], [], [1, 2]], 5)] == [0, 0, 0]
        h.set_index(a)
        terms = list(range(bc.PLANTED_TERMS))
        _assert_same(h.search(terms, 255), bm.search(a, terms, 255), "first index")
        h.batch([terms] * 3, 10)
        h.set_index(b)                                         # another N, V and k1p1 on the same handle
        _assert_same(h.search([0, 2], 300), bm.search(b, [0, 2], 300), "second index")
        h.set_index(empty_corpus)
        assert h.search([0], 5)[2] == 0


# ---- 7. masked accumulate -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_masked_batches(where):
    import torch
    from tristage_rag_amd import _lib
    ix, masks = bc.mask_case()
    words = (ix.N + 31) // 32 + 2                              # rows longer than the N bits need
    packed = bc.pack_masks(masks, words)
    rng = np.random.default_rng(8)
    everyone = ix.V - 1
    queries = [[everyone], [everyone, 3], [5, 5, 9], []] + [[int(t) for t in rng.integers(0, ix.V, size=int(rng.integers(1, 6)))]
                                                            for _ in range(126)]
    # 130 queries: masks 0..5 and "none" round and round, so both sides of the 64-lane boundary mix all of them
    moq = [(q % 7) - 1 for q in range(len(queries))]
    assert {moq[62], moq[63], moq[64], moq[65]} >= {-1, 0} and len(set(moq[:64])) == 7 == len(set(moq[64:128]))
    kw = dict(masks=packed, mask_of_query=moq, words=words)
    dev = None
    if where == "device":
        dev = torch.from_numpy(packed.view(np.int32)).cuda()
        torch.cuda.synchronize()
        kw["bits_ptr"] = dev.data_ptr()
    else:
        kw["flags"] = _lib.TS_FLAG_HOST_PTR
    with Handle(ix) as h:
        for k in (1, 300):
            for qi, (q, got) in enumerate(zip(queries, h.batch(queries, k, **kw))):
                allowed = None if moq[qi] < 0 else masks[moq[qi]]
                _assert_same(got, bm.search(ix, q, k, allowed), f"mask {moq[qi]} query {qi} k={k} terms={q}")
        # one query per mask, each alone in its batch, and a batch in which nobody is filtered
        for m in range(len(masks)):
            (got,) = h.batch([[everyone, 3]], 5, **dict(kw, mask_of_query=[m]))
            _assert_same(got, bm.search(ix, [everyone, 3], 5, masks[m]), f"mask {m} alone")
        for q, got in zip(queries[:5], h.batch(queries[:5], 300, **dict(kw, mask_of_query=[-1] * 5))):
            _assert_same(got, bm.search(ix, q, 300), "unfiltered queries of a filtered batch")
    del dev


# ---- 8. negative and cancelling contributions ---------------------------------------------------------------------------
def test_negative_and_cancelling_contributions():
    """Touched documents at 0.0 and below: each is listed once (a document whose sum comes back to exactly 0.0 is not
    touched a second time), untouched ones never, n_out = min(k, touched)."""
    case = bc.negative_case()
    _run_case(case, "negative idf")
    with Handle(case.ix) as h:
        queries = [s.terms for s in case.searches]
        for k in (5, 400):
            for q, got in zip(queries, h.batch(queries * 2, k)):
                _assert_same(got, bm.search(case.ix, q, k), f"negative idf (batch) k={k} terms={q}")
        allowed = np.zeros(case.ix.N, dtype=bool)
        allowed[55:65] = allowed[120] = allowed[200] = True
        words = (case.ix.N + 31) // 32
        (got,) = h.batch([[0, 1, 2]], 400, masks=bc.pack_masks([allowed], words), mask_of_query=[0], words=words, flags=1)
        _assert_same(got, bm.search(case.ix, [0, 1, 2], 400, allowed), "negative idf, masked")


REFIT_FIRST, REFIT_SECOND = ["alpha"] * 5 + ["x y"], ["zeta eta"]


def _refit_pair():
    from tristage_rag_amd.stage1_retriever import BM25Index
    host, gpu = BM25Index(refit_compat=True), BM25Index(gpu_device=0, refit_compat=True)
    for idx in (host, gpu):
        idx.fit(REFIT_FIRST)
        idx.fit(REFIT_FIRST + REFIT_SECOND)
    assert host.idf["alpha"] < 0
    return host, gpu


def test_gpu_index_equals_host_index_with_a_negative_idf():
    """df counts the first fit's entries again (refit_compat), so idf["alpha"] < 0: the documents holding the term
    rank BELOW the ones that do not."""
    host, gpu = _refit_pair()
    queries = ["alpha", "alpha zeta", "zeta", "alpha alpha x", "nosuch", "y alpha"]
    n = host.corpus_size
    allowed = [None, np.arange(n) % 2 == 0, np.arange(n) < 3, None, np.arange(n) > 4, np.zeros(n, dtype=bool)]
    try:
        for k in (1, 3, 7, 50):
            for q, a in zip(queries, allowed):
                assert gpu.search(q, k) == host.search(q, k), (q, k)
                assert gpu.search(q, k, allowed=a) == host.search(q, k, allowed=a), (q, k, "filtered")
            assert gpu.search_many(queries, k) == host.search_many(queries, k), k
            assert gpu.search_many(queries, k, allowed=allowed) == host.search_many(queries, k, allowed=allowed), k
            for filt in (None, allowed):
                for (gi, gs), (hi, hs) in zip(gpu.search_many_arrays(queries, k, allowed=filt),
                                              host.search_many_arrays(queries, k, allowed=filt)):
                    assert gi.dtype == np.int64 and gs.dtype == np.float64
                    assert gi.tolist() == hi.tolist() and gs.tolist() == hs.tolist(), (k, filt is not None)
    finally:
        gpu.close()


# ---- 9. top_k above 2048 ------------------------------------------------------------------------------------------------
def test_gpu_index_equals_host_index_above_2048():
    from tristage_rag_amd.stage1_retriever import BM25Index
    rng = np.random.default_rng(12)
    vocab = [f"w{i}" for i in range(150)]
    p = 1.0 / np.arange(1, 151)
    p /= p.sum()
    docs = [" ".join(rng.choice(vocab, size=int(rng.integers(3, 30)), p=p)) for _ in range(3000)]
    host, gpu = BM25Index(), BM25Index(gpu_device=0)
    host.fit(docs)
    gpu.fit(docs)
    queries = ["w0 w1 w2", "w149", "w3 w3 nosuch w40", ""]
    allowed = [None, np.arange(3000) % 3 != 0, None, np.arange(3000) < 2600]
    try:
        for k in (2048, 2049, 2500, 3000, 5000):
            for q in queries:
                assert gpu.search(q, k) == host.search(q, k), (q, k)
            assert gpu.search_many(queries, k) == host.search_many(queries, k), k
            assert gpu.search_many(queries, k, allowed=allowed) == host.search_many(queries, k, allowed=allowed), k
            for (gi, gs), (hi, hs) in zip(gpu.search_many_arrays(queries, k), host.search_many_arrays(queries, k)):
                assert gi.tolist() == hi.tolist() and gs.tolist() == hs.tolist(), k
    finally:
        gpu.close()
