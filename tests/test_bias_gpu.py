"""Boosted search on the GPU: ``search_biased`` against the model of tests/bias_model.py, which is
built from the product's own dense scores: ``Sb = float32(scores(q) + bias)``, the disallowed and removed rows dropped,
ordered by (Sb descending, id ascending), cut at k and padded.  Every comparison is equality of ids and of score values.

The filter path's sample at N = 40 001: 1251 row blocks, 256 of them sampled (every 4th), so S = 8192 sample rows, and
the threshold is the m-th best boosted sample score with m = max(24, ceil(4 k S / N)) = 24, 24, 82 for k = 1, 10, 100:
about 117, 117 and 400 expected candidates per query, far from both k and the 16 384 candidate slots, so a pass of
these seeded inputs that is redone densely has a wrong threshold."""
import numpy as np
import pytest

import bias_model as bm
import exact_inputs as ei
from helpers import make_corpus

pytestmark = pytest.mark.gpu

N = 40_001                   # above the filter path's floor of 32 768 rows, not a multiple of 32
BATCHES = (1, 31, 64, 100)   # one query half, one (ragged), two, and two passes
KS = (1, 10, 100, 1000, 2048)


def _torch():
    import torch
    return torch


def _index(rows, dtype):
    from tristage_rag_amd.index import FlatIPIndex
    ix = FlatIPIndex(rows.shape[1], dtype=dtype)
    ix.add(rows)
    return ix


def _dev(x, dtype):
    torch = _torch()
    return torch.from_numpy(np.array(x, copy=True)).cuda().to(torch.float16 if dtype == "f16" else torch.bfloat16)


def _bias_dev(b):
    return _torch().from_numpy(np.ascontiguousarray(b, dtype=np.float32)).cuda()


def _fused_only(ix, what):
    info = ix.last_bias_info()
    assert info["passes"] >= 1 and info["fused_passes"] == info["passes"] and info["redone"] == 0, (what, info)
    return info


# ------------------------------------------------------------------------------------------------- the fused path
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [128, 384, 768])
def test_fused_path_equals_the_model(d, dtype):
    rng = np.random.default_rng(1000 + d)
    rows = make_corpus(N, d, seed=d, dtype=dtype)
    q = _dev(make_corpus(max(BATCHES), d, seed=3 * d + 1, dtype=dtype), dtype)
    ix = _index(rows, dtype)
    try:
        S = ix.scores(q).cpu().numpy()
        assert S.dtype == np.float32 and S.shape == (max(BATCHES), N)
        by_raw = np.argsort(S[0], kind="stable")
        spikes = np.zeros(N, np.float32)
        spike_rows = rng.choice(by_raw[:2000], size=50, replace=False)      # among the LOWEST raw scores of query 0
        spikes[spike_rows] = 2.0
        sunk = np.zeros(N, np.float32)
        sunk_rows = by_raw[-100:]                                            # the raw top 100 of query 0
        sunk[sunk_rows] = -2.0
        biases = {"zeros": np.zeros(N, np.float32),
                  "normal": (0.1 * rng.standard_normal(N)).astype(np.float32),
                  "spikes": spikes, "sunk": sunk}
        for name, bias in biases.items():
            want_D, want_I = bm.topk_model(S, bias, max(KS))                 # one model per bias: its prefixes serve all
            bt = _bias_dev(bias)
            assert bt.shape == (N,)                                          # exactly ntotal entries: the tail block's end
            for B in BATCHES:
                for k in KS:
                    what = f"d={d} {dtype} bias={name} B={B} k={k}"
                    got = ix.search_biased(q[:B], k, bt)
                    bm.same(got, (want_D[:B, :k], want_I[:B, :k]), what)
                    info = ix.last_bias_info()
                    assert info["passes"] == (B + 63) // 64, (what, info)
                    if k <= 100:
                        _fused_only(ix, what)
                    else:
                        assert info["fused_passes"] >= 1, (what, info)
            I0 = want_I[0]
            if name == "zeros":      # the plain search's ids, and its scores as floats (-0.0 + 0.0 is +0.0)
                for B, k in ((64, 100), (100, 10)):
                    pd, pi = ix.search(q[:B], k)
                    bm.same(ix.search_biased(q[:B], k, bt), (pd.cpu().numpy() + np.float32(0.0), pi.cpu().numpy()), "zero bias")
            if name == "normal":
                plain = ix.search(q[:1], 100)[1].cpu().numpy()[0]
                assert (I0[:100] != plain).mean() > 0.5                      # the bias reorders most of the top 100
            if name == "spikes":     # rows no fetch-then-rerank shortlist would hold: all 50 lead query 0's list
                assert set(I0[:50].tolist()) == set(spike_rows.tolist())
                got10 = ix.search_biased(q[:1], 10, bt)[1].cpu().numpy()[0]
                assert set(got10.tolist()) <= set(spike_rows.tolist())
                fetched = ix.search(q[:1], 2048)[1].cpu().numpy()[0]
                assert not set(fetched.tolist()) & set(spike_rows.tolist())
            if name == "sunk":
                assert not set(I0[:1000].tolist()) & set(sunk_rows.tolist())
        # numpy in -> numpy out, through host pointers
        D, I = ix.search_biased(q[:7].float().cpu().numpy(), 10, biases["normal"])
        assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
        bm.same((D, I), bm.topk_model(S[:7], biases["normal"], 10), "host pointers")
    finally:
        ix.close()


# ---------------------------------------------------------------------------------------------------- exact ties
@pytest.mark.parametrize("dtype,cls", [("f16", "ints"), ("bf16", "neg")])
def test_exact_ties_come_out_in_id_order(dtype, cls):
    """Exactly summable rows and queries (integer scores below 2^24) and integer biases: every boosted score is exact,
    and a bias that rounds query 0's scores down to multiples of 4096 makes distinct (score, bias) pairs collide."""
    n, d, B, k = ei.N_FILTER, 128, 64, 100
    c, q, unit = ei.case(cls, n, d, B)
    assert unit == 1.0
    ix = _index(c, dtype)
    try:
        qt = _dev(q, dtype)
        S = ix.scores(qt).cpu().numpy()
        exact = ei.exact_scores(c, q)
        assert np.array_equal(S.astype(np.float64), exact)                   # the inputs are what they claim to be
        bias = -np.mod(exact[0], 4096.0).astype(np.float32)
        assert np.array_equal(bias.astype(np.float64) + exact[0], np.floor(exact[0] / 4096.0) * 4096.0)
        want = bm.topk_model(S, bias, k)
        assert np.unique(want[0][0]).size <= k // 4                          # ties, many, within query 0's top k
        tied = want[0][0][:-1] == want[0][0][1:]
        assert (np.diff(want[1][0])[tied] > 0).all()                         # (the model's own order: ids ascend in a tie)
        got = ix.search_biased(qt, k, _bias_dev(bias))
        bm.same(got, want, f"{cls} {dtype}")
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))     # bit for bit
        _fused_only(ix, "ties")
        bm.same(ix.search_biased(qt, k, _bias_dev(bias), exact_dense=True), want, "dense path")
    finally:
        ix.close()


# ------------------------------------------------------------------------------- masks, tombstones and mutation
def test_masks_tombstones_and_mutation():
    dtype, d, B, k = "f16", 128, 33, 10
    rng = np.random.default_rng(7)
    rows = make_corpus(N, d, seed=71, dtype=dtype)
    q = _dev(make_corpus(B, d, seed=72, dtype=dtype), dtype)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    ix = _index(rows, dtype)
    try:
        S = ix.scores(q).cpu().numpy()
        tenth = rng.random(N) < 0.1
        span = np.zeros(N, bool)
        span[20_000:20_400] = True                                           # a contiguous 1 % range
        few = np.zeros(N, bool)
        few[[5, 31, 32, 17_777, N - 1]] = True                               # fewer than k eligible rows: padding
        per_query = [(tenth, span, None, few)[i % 4] for i in range(B)]      # masked and unmasked queries in one pass
        bt = _bias_dev(bias)
        for name, allowed in (("shared", tenth), ("per query", per_query), ("range", span), ("few", few)):
            bm.same(ix.search_biased(q, k, bt, allowed=allowed), bm.topk_model(S, bias, k, allowed=allowed), name)
            _fused_only(ix, name)
        D, I = (x.cpu().numpy() for x in ix.search_biased(q, k, bt, allowed=few))
        assert (I[:, 5:] == -1).all() and (D[:, 5:] == -bm.FLT_MAX).all() and (I[:, :5] >= 0).all()
        # an id offset: the bias stays indexed by local row
        ix.set_id_offset(1_000_000)
        bm.same(ix.search_biased(q, k, bt, allowed=per_query),
                bm.topk_model(S, bias, k, allowed=per_query, id_offset=1_000_000), "id offset")
        ix.set_id_offset(0)
        # 5 % of the rows removed, the best boosted rows of query 0 among them
        live = np.ones(N, bool)
        gone = np.unique(np.concatenate([rng.choice(N, size=N // 20, replace=False), bm.topk_model(S[:1], bias, 20)[1][0]]))
        assert ix.remove_ids(gone) == gone.size
        live[gone] = False
        for name, allowed in (("removed", None), ("removed, per query", per_query)):
            got = ix.search_biased(q, k, bt, allowed=allowed)
            bm.same(got, bm.topk_model(S, bias, k, live=live, allowed=allowed), name)
            assert not np.isin(got[1].cpu().numpy(), gone).any()
            _fused_only(ix, name)
        # update_rows: new content under old ids, the bias belongs to the id
        upd = np.flatnonzero(live)[rng.choice(int(live.sum()), size=300, replace=False)]
        new_rows = make_corpus(upd.size, d, seed=73, dtype=dtype)
        new_rows[:3] = q[:3].float().cpu().numpy()                           # three of them become some query's best match
        ix.update_rows(upd, new_rows)
        S2 = ix.scores(q).cpu().numpy()
        assert not np.array_equal(S2[:, upd], S[:, upd])
        bm.same(ix.search_biased(q, k, bt), bm.topk_model(S2, bias, k, live=live), "updated")
        assert upd[0] in ix.search_biased(q[:1], k, bt)[1].cpu().numpy()[0]   # (its score is ~1, its bias ~0.1)
        # compact: rows move down, the bias array is re-indexed through the map
        old2new = ix.compact()
        n2 = int(live.sum())
        assert ix.ntotal == n2
        bias2 = np.empty(n2, np.float32)
        bias2[old2new[live]] = bias[live]
        S3 = ix.scores(q).cpu().numpy()
        assert np.array_equal(S3, S2[:, live])
        bm.same(ix.search_biased(q, k, _bias_dev(bias2)), bm.topk_model(S3, bias2, k), "compacted")
        _fused_only(ix, "compacted")
        from tristage_rag_amd.index import pack_allowed
        bm.same(ix.search_biased(q, k, _bias_dev(bias2), allowed=tenth[live]),
                bm.topk_model(S3, bias2, k, allowed=tenth[live]), "compacted, masked")
        assert pack_allowed(tenth[live], n2).shape == ((n2 + 31) // 32,)
        with pytest.raises(ValueError, match="one entry per row"):
            ix.search_biased(q, k, bt)                                       # the old array no longer fits
    finally:
        ix.close()


def test_unchecked_nan_rows_are_never_returned_and_checked_ones_raise():
    dtype, d, B, k = "f16", 128, 5, 10
    rows = make_corpus(N, d, seed=75, dtype=dtype)
    q = _dev(make_corpus(B, d, seed=76, dtype=dtype), dtype)
    ix = _index(rows, dtype)
    try:
        S = ix.scores(q).cpu().numpy()
        bias = np.zeros(N, np.float32)
        best = bm.topk_model(S, bias, 3)[1].reshape(-1)
        bias[best] = np.nan                                                  # every query's three best rows
        bt = _bias_dev(bias)
        with pytest.raises(ValueError, match="finite"):
            ix.search_biased(q, k, bt)
        for cf in (True, False):                                             # a bias that goes through the host: always
            with pytest.raises(ValueError, match="finite"):
                ix.search_biased(q.float().cpu().numpy(), k, bias, check_finite=cf)
        for dense in (False, True):
            got = ix.search_biased(q, k, bt, check_finite=False, exact_dense=dense)
            bm.same(got, bm.topk_model(S, bias, k), f"NaN rows, dense={dense}")
            assert not np.isin(got[1].cpu().numpy(), best).any()
    finally:
        ix.close()


def test_no_mask_at_all_never_reads_the_callers_allow_bits():
    """A boosted pass takes the masked scan also when no query has a mask, and that scan reads word 0 of "mask 0" for
    its unmasked queries: with n_masks == 0 it must not be the caller's allow_bits, which is then not staged and may
    point anywhere.  Through the binding (an all-None list, numpy and CUDA queries) and through the library itself
    with a non-null allow_bits beside n_masks == 0, host pointers and device pointers."""
    import ctypes
    from tristage_rag_amd import _lib
    dtype, d, B, k = "f16", 128, 33, 10
    rng = np.random.default_rng(17)
    rows = make_corpus(N, d, seed=77, dtype=dtype)
    qn = make_corpus(B, d, seed=78, dtype=dtype)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    ix = _index(rows, dtype)
    try:
        qt, bt = _dev(qn, dtype), _bias_dev(bias)
        want = bm.topk_model(ix.scores(qt).cpu().numpy(), bias, k)
        bm.same(ix.search_biased(qn, k, bias, allowed=[None] * B), want, "numpy queries, all-None list")
        _fused_only(ix, "numpy queries, all-None list")
        bm.same(ix.search_biased(qt, k, bt, allowed=[None] * B), want, "CUDA queries, all-None list")
        _fused_only(ix, "CUDA queries, all-None list")
        addr = lambda a: ctypes.c_void_p(a.ctypes.data)
        words = np.zeros((N + 31) // 32, np.uint32)                    # host memory: not readable by the scan
        moq = np.full(B, -1, np.int32)
        D, I = np.empty((B, k), np.float32), np.empty((B, k), np.int64)
        st = ix._lib.ts_index_search_biased(ix._h, addr(qn), B, _lib.TS_F32, k, addr(bias), N, addr(words), words.size, 0,
                                            addr(moq), addr(D), addr(I), _lib.TS_FLAG_HOST_PTR, None)
        assert st == _lib.TS_OK, _lib.last_error()
        bm.same((D, I), want, "library, host pointers, n_masks = 0 with allow_bits set")
        torch = _torch()
        q32 = torch.from_numpy(qn).cuda()
        Dt = torch.empty((B, k), dtype=torch.float32, device="cuda")
        It = torch.empty((B, k), dtype=torch.int64, device="cuda")
        st = ix._lib.ts_index_search_biased(ix._h, ctypes.c_void_p(q32.data_ptr()), B, _lib.TS_F32, k,
                                            ctypes.c_void_p(bt.data_ptr()), N, addr(words), words.size, 0, None,
                                            ctypes.c_void_p(Dt.data_ptr()), ctypes.c_void_p(It.data_ptr()), 0, None)
        assert st == _lib.TS_OK, _lib.last_error()
        bm.same((Dt, It), want, "library, device pointers, n_masks = 0 with allow_bits set")
        _fused_only(ix, "library, device pointers")
    finally:
        ix.close()


def test_the_library_checks_that_need_a_handle():
    """What the binding refuses first and the library has to refuse on its own: bias_rows < ntotal, a host bias that is
    not finite, a misaligned device bias, fp32 storage; and a call without queries resets the counters."""
    import ctypes
    from tristage_rag_amd import _lib
    from tristage_rag_amd.index import FlatIPIndex
    d, n, B, k = 128, 2_000, 3, 5
    rows = make_corpus(n, d, seed=79, dtype="f16")
    qn = make_corpus(B, d, seed=80, dtype="f16")
    addr = lambda a: ctypes.c_void_p(a.ctypes.data)
    D, I = np.empty((B, k), np.float32), np.empty((B, k), np.int64)
    ix = _index(rows, "f16")
    try:
        def call(bias_ptr, bias_rows, flags=_lib.TS_FLAG_HOST_PTR, nq=B):
            return ix._lib.ts_index_search_biased(ix._h, addr(qn), nq, _lib.TS_F32, k, bias_ptr, bias_rows, None, 0, 0, None,
                                                  addr(D), addr(I), flags, None)
        bias = np.zeros(n, np.float32)
        assert call(addr(bias), n) == _lib.TS_OK
        assert ix.last_bias_info()["passes"] == 1
        assert call(addr(bias), n, nq=0) == _lib.TS_OK and ix.last_bias_info()["passes"] == 0
        assert call(addr(bias), n - 1) == _lib.TS_ERR_INVALID and "bias_rows" in _lib.last_error()
        for v in (np.nan, np.inf, -np.inf):
            bad = bias.copy()
            bad[n - 1] = v
            assert call(addr(bad), n) == _lib.TS_ERR_INVALID and "not finite" in _lib.last_error()
        bad = bias.copy()
        bad[n - 1] = np.nan
        assert call(addr(bad), n + 5) == _lib.TS_ERR_INVALID          # (entries beyond ntotal are not looked at ...
        longer = np.concatenate([bias, np.full(5, np.nan, np.float32)])
        assert call(addr(longer), n + 5) == _lib.TS_OK                 # ... so a NaN there is nobody's business)
        bt = _bias_dev(np.zeros(n + 1, np.float32))
        assert call(ctypes.c_void_p(bt.data_ptr() + 4), n, flags=0) == _lib.TS_ERR_INVALID and "aligned" in _lib.last_error()
    finally:
        ix.close()
    f32 = FlatIPIndex(d, dtype="f32")
    f32.add(rows)
    try:
        st = f32._lib.ts_index_search_biased(f32._h, addr(qn), B, _lib.TS_F32, k, addr(np.zeros(n, np.float32)), n, None, 0,
                                             0, None, addr(D), addr(I), _lib.TS_FLAG_HOST_PTR, None)
        assert st == _lib.TS_ERR_UNSUPPORTED and "f16 / bf16" in _lib.last_error()
    finally:
        f32.close()


# ------------------------------------------------------------------------------------------------------- the redo
def test_candidate_overflow_is_redone_exactly():
    """20 000 identical rows with one bias: 20 000 equal boosted scores, more than the 16 384 candidate slots."""
    d, k = 128, 10
    rng = np.random.default_rng(10)
    axis = np.zeros(d, np.float32)
    axis[0] = 1.0
    other = rng.standard_normal((20_000, d)).astype(np.float32) * 0.05
    other[:, 2] += 1.0
    x = np.concatenate([np.repeat(axis[None], 20_000, axis=0), other / np.linalg.norm(other, axis=1, keepdims=True)])
    x = x[rng.permutation(len(x))]
    same_rows = x[:, 0] == 1.0
    bias = np.where(same_rows, np.float32(0.25), (0.01 * rng.standard_normal(len(x))).astype(np.float32)).astype(np.float32)
    ix = _index(x, "f16")
    try:
        q = _dev(np.stack([axis, np.roll(axis, 1)]), "f16")
        S = ix.scores(q).cpu().numpy()
        for kk in (k, 1000):
            got = ix.search_biased(q, kk, _bias_dev(bias))
            info = ix.last_bias_info()
            assert info == {"passes": 1, "fused_passes": 1, "redone": 1, "blocks_read": info["blocks_read"]}, info
            bm.same(got, bm.topk_model(S, bias, kk), f"k={kk}")
        assert (got[0].cpu().numpy()[0] == np.float32(1.25)).all()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------- the dense path
def test_dense_path_equals_the_model():
    dtype, d = "bf16", 384
    rng = np.random.default_rng(11)
    q = _dev(make_corpus(65, d, seed=91, dtype=dtype), dtype)
    for n, ks, kw in ((2_000, (1, 10, 2_003), {}), (N, (4_096,), {}), (N, (10, 100), {"exact_dense": True})):
        rows = make_corpus(n, d, seed=90 + n % 7, dtype=dtype)
        bias = (0.1 * rng.standard_normal(n)).astype(np.float32)
        mask = rng.random(n) < 0.3
        ix = _index(rows, dtype)
        try:
            S = ix.scores(q).cpu().numpy()
            bt = _bias_dev(bias)
            for k in ks:
                for allowed in (None, mask):
                    got = ix.search_biased(q, k, bt, allowed=allowed, **kw)
                    bm.same(got, bm.topk_model(S, bias, k, allowed=allowed), f"n={n} k={k} masked={allowed is not None}")
                    info = ix.last_bias_info()
                    assert info["passes"] == 2 and info["fused_passes"] == 0 and info["redone"] == 0, info
        finally:
            ix.close()


# ------------------------------------------------------------------------------------- retriever and pipeline
DOCS = [f"passage {i}: " + " ".join(f"w{(i * 7 + j * 13) % 97}" for j in range(12)) for i in range(300)]
DOC_META = [{"ts": 1_000.0 + i, "pop": float(i % 11)} if i % 10 else {"pop": 1.0} for i in range(300)]
QUERIES = ["w3 w16 w29", "w50 w63", "passage 17"]


def _retriever(tmp_path, **kw):
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    cfg = Stage1Config(model_name="random:tiny", device="cuda", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
                       index_dtype="f16", enable_bm25=kw.pop("enable_bm25", False), **kw)
    s1 = Stage1Retriever(cfg)
    s1.add_documents(DOCS, DOC_META)
    return s1


def test_retriever_boosts_change_the_list_as_search_biased_does(tmp_path):
    from tristage_rag_amd import boost
    s1 = _retriever(tmp_path)
    assert s1._device_path()
    ix = s1.faiss_index
    decay = {"field": "ts", "decay": "gauss", "origin": 1_299.0, "scale": 40.0, "weight": 0.3, "missing": -0.5}
    arr = (0.05 * np.random.default_rng(3).standard_normal(300)).astype(np.float32)
    qt = s1._normalized_query_tensor(QUERIES)
    plain = s1.search_many(QUERIES, top_k=10)
    for spec in (arr, decay):
        bias = boost.bias_array(spec, DOC_META)
        D, I = (x.cpu().numpy() for x in ix.search_biased(qt, 10, _bias_dev(bias)))
        bm.same((D, I), bm.topk_model(ix.scores(qt).cpu().numpy(), bias, 10), "the index call")
        got = s1.search_many(QUERIES, top_k=10, boost=spec)
        assert [[r["doc_id"] for r in rs] for rs in got] == I.tolist()
        assert [[np.float32(r["score"]) for r in rs] for rs in got] == D.tolist()
        assert [r["doc_id"] for r in s1.search(QUERIES[0], top_k=10, boost=spec)] == I[0].tolist()
        ids, sc = s1.search_many_arrays(QUERIES, top_k=10, boost=spec)
        assert ids.cpu().numpy().tolist() == I.tolist() and np.array_equal(sc.cpu().numpy(), D)
        assert [[r["doc_id"] for r in rs] for rs in got] != [[r["doc_id"] for r in rs] for rs in plain]
        # filter= composes
        flt = {"pop": 1.0}
        allow = s1.filter_mask(flt)
        got = s1.search_many(QUERIES, top_k=10, filter=flt, boost=spec)
        want = ix.search_biased(qt, 10, _bias_dev(bias), allowed=allow)[1].cpu().numpy()
        assert [[r["doc_id"] for r in rs] for rs in got] == [[i for i in row if i >= 0] for row in want.tolist()]
    assert s1.search_many(QUERIES, top_k=10) == plain                      # boost=None: the parent behaviour
    assert s1.search_many(QUERIES, top_k=10, boost=None) == plain
    with pytest.raises(ValueError, match="boost"):
        s1.search(QUERIES[0], top_k=5, boost=decay, funnel_dims=128)
    with pytest.raises(ValueError, match="boost"):
        s1.search(QUERIES[0], top_k=5, boost=decay, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="boost"):
        s1.search(QUERIES[0], top_k=5, boost=decay, group_by="pop")
    # the device arrays are cached per spec and dropped by a mutation
    s1.search(QUERIES[0], top_k=5, boost=decay)
    dev = s1._boost_lru[boost.spec_key(decay)[0]]["dev"]
    s1.search(QUERIES[1], top_k=5, boost=dict(decay))
    assert s1._boost_lru[boost.spec_key(decay)[0]]["dev"] is dev and dev.is_cuda
    s1.remove_documents([299])
    assert len(s1._boost_lru) == 0
    assert 299 not in [r["doc_id"] for r in s1.search(QUERIES[0], top_k=300, boost=decay)]
    # BM25 + RRF runs on the boosted list
    s2 = _retriever(tmp_path, enable_bm25=True, boost=decay)
    fused = s2.search_many(QUERIES, top_k=10)
    assert all(len(rs) == 10 for rs in fused)
    assert s2.faiss_index.last_bias_info()["passes"] == 1                  # the config's boost reached the index


def test_unsupported_retrievers_refuse(tmp_path):
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    spec = {"field": "pop", "weight": 0.1}
    for dt in ("f32", "fp8"):
        s1 = Stage1Retriever(Stage1Config(model_name="random:tiny", device="cuda", cache_dir=str(tmp_path / "m"),
                                          index_dir=str(tmp_path / "i"), index_dtype=dt, enable_bm25=False))
        s1.add_documents(DOCS[:64], DOC_META[:64])
        with pytest.raises(NotImplementedError, match=dt):
            s1.search(QUERIES[0], top_k=5, boost=spec)
        with pytest.raises(NotImplementedError, match=dt):
            s1.faiss_index.search_biased(s1._normalized_query_tensor(QUERIES), 5, np.zeros(64, np.float32))
    ivf = Stage1Retriever(Stage1Config(model_name="random:tiny", device="cuda", cache_dir=str(tmp_path / "m"),
                                       index_dir=str(tmp_path / "i"), index_dtype="f16", enable_bm25=False,
                                       index_type="ivf", nlist=4))
    ivf.add_documents(DOCS, DOC_META)
    assert ivf.index_type_used == "ivf"
    with pytest.raises(NotImplementedError, match="IVF"):
        ivf.search(QUERIES[0], top_k=5, boost=spec)
    with pytest.raises(NotImplementedError, match="search_biased"):
        ivf.faiss_index.search_biased(ivf._normalized_query_tensor(QUERIES), 5, np.zeros(300, np.float32))


def test_pipeline_boost_reaches_stage1_and_none_is_the_parent_behaviour(tmp_path):
    from pipeline_pairs import gpu_pipeline, synth_docs
    from tristage_rag_amd import boost
    docs = synth_docs(200)
    meta = [{"ts": float(i)} for i in range(len(docs))]
    p = gpu_pipeline(tmp_path, stage1_index_dtype="f16", stage1_enable_bm25=False)
    p.add_documents(docs, meta)
    spec = {"field": "ts", "decay": "linear", "origin": 199.0, "scale": 50.0, "weight": 0.5}
    queries = [docs[3][:40], docs[150][:40]]
    plain = p.search_many(queries)
    boosted_ = p.search_many(queries, boost=spec)
    s1 = p.stage1
    bias = boost.bias_array(spec, s1.doc_metadata)
    want = s1.faiss_index.search_biased(s1._normalized_query_tensor(queries), p.config.stage1_top_k, _bias_dev(bias))[1]
    for out, row in zip(boosted_, want.cpu().numpy().tolist()):
        assert [r["doc_id"] for r in out["stage1_results"]] == row          # (save_intermediate_results is on)
    assert [[r["doc_id"] for r in o["stage1_results"]] for o in boosted_] != \
           [[r["doc_id"] for r in o["stage1_results"]] for o in plain]
    assert [[r["doc_id"] for r in o["results"]] for o in p.search_many(queries)] == \
           [[r["doc_id"] for r in o["results"]] for o in plain]                                     # off is off
    one = p.search(queries[0], boost=spec)
    assert [r["doc_id"] for r in one["results"]] == [r["doc_id"] for r in boosted_[0]["results"]]
    assert [r["doc_id"] for r in p.batch_search(queries[:1], boost=spec)[0]["results"]] == [r["doc_id"] for r in one["results"]]
    with pytest.raises(ValueError, match="boost"):
        p.search(queries[0], boost=spec, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="boost"):
        p.search_many(queries, boost=spec, group_by="ts")
    with pytest.raises(ValueError, match="boost"):
        p.search(queries[0], boost=spec, funnel_dims=128)
