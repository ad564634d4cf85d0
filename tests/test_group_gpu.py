"""Grouped search on the GPU (ts_group_topk, search_grouped, group_by) against the host model of
tests/group_model.py.  The collapse never compares a score: it is a function of the list order and the group table
alone, so every output must EQUAL the model's (``array_equal``; scores by their bits).

Where a ranking is needed it is the one ``search`` returns for the whole index (``search(q, ntotal)``), which the exact
search tests hold to their own reference; the code under test is never its own reference.  One reading of the contract
is spelled out here: with ``group_size > 1`` a group's rows are its best rows within the first ``fetched`` places, so
the result equals the model over ``search(q, fetched)`` by definition and the model over ``search(q, ntotal)`` when
everything is fetched; its GROUPS and each group's first row equal the whole ranking's for every complete query."""
import numpy as np
import pytest

import exact_inputs as xi
import group_model as gm

pytestmark = pytest.mark.gpu

# the kernel's paths: n = C rounded up to a power of two, at least 8, is the sorted length (8 / 9 and 63 / 64 / 65 cross
# one; at 8 the whole sort is one pass in registers), 256 threads up to n = 1024 and 1024 above, the 64 KiB LDS attribute
# above n = 4096, and the limit
SIZES = (1, 8, 9, 63, 64, 65, 1024, 1025, 4096, 4097, 16384)
GROUP_SIZES = (1, 2, 5)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def tables():
    return gm.tables()


def _ix():
    from tristage_rag_amd import index
    return index


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _same(got, want, what):
    names = ("D", "I", "G", "n_groups", "n_valid")
    for name, g, w in zip(names, got, want):
        g = _np(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        if name == "D":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, name)


def _ks(C, gs):
    return sorted({1, 7, min(C, 16384 // gs)})


# ------------------------------------------------------------------------------------------------ group_topk
@pytest.mark.parametrize("C", SIZES)
def test_group_topk_equals_the_model(torch_mod, tables, C):
    torch = torch_mod
    dev = torch.device("cuda", 0)
    for B in (1, 33):
        ids, scores = gm.lists(B, C, out_of_range=True)
        ids_t, sc_t = torch.from_numpy(ids).to(dev), torch.from_numpy(scores).to(dev)
        for name, tab in tables.items():
            tab_t = torch.from_numpy(tab).to(dev)
            walked = [gm.group_rank_occ(ids[b], tab) for b in range(B)]
            for gs in GROUP_SIZES:
                for k in _ks(C, gs):
                    got = _ix().group_topk(ids_t, sc_t, tab_t, k, gs)
                    assert all(torch.is_tensor(t) and t.is_cuda for t in got)
                    _same(got, gm.group_topk_from(ids, scores, tab, walked, k, gs), (C, B, name, k, gs))


@pytest.mark.parametrize("C", (1, 65, 1025, 16384))
def test_host_arrays_and_device_tensors_give_the_same_bits_and_so_do_two_runs(torch_mod, tables, C):
    torch = torch_mod
    dev = torch.device("cuda", 0)
    ids, scores = gm.lists(33, C)                       # (no out-of-range ids: host pointers refuse them)
    for name in ("heavy", "fives"):
        tab = tables[name]
        walked = [gm.group_rank_occ(ids[b], tab) for b in range(33)]
        for k, gs in ((7, 2), (min(C, 3000), 5)):
            want = gm.group_topk_from(ids, scores, tab, walked, k, gs)
            args = [torch.from_numpy(a).to(dev) for a in (ids, scores, tab)]
            first = _ix().group_topk(*args, k, gs)
            second = _ix().group_topk(*args, k, gs)
            host = _ix().group_topk(ids, scores, tab, k, gs)
            assert all(isinstance(a, np.ndarray) for a in host)
            for got in (first, second, host):
                _same(got, want, (C, name, k, gs))


def test_rows_of_a_batch_equal_single_query_calls_and_the_id_base_is_taken_off(torch_mod, tables):
    torch = torch_mod
    dev = torch.device("cuda", 0)
    tab = tables["heavy"]
    tab_t = torch.from_numpy(tab).to(dev)
    for C in (65, 1025):
        ids, scores = gm.lists(33, C, out_of_range=True)
        ids_t, sc_t = torch.from_numpy(ids).to(dev), torch.from_numpy(scores).to(dev)
        whole = [_np(t) for t in _ix().group_topk(ids_t, sc_t, tab_t, 7, 2)]
        for b in range(33):
            one = _ix().group_topk(ids_t[b: b + 1], sc_t[b: b + 1], tab_t, 7, 2)
            _same(one, [w[b: b + 1] for w in whole], (C, b))
        base = 1000
        ids_o, _ = gm.lists(33, C, id_base=base, out_of_range=True)
        got = _ix().group_topk(torch.from_numpy(ids_o).to(dev), sc_t, tab_t, 7, 2, id_base=base)
        walked = [gm.group_rank_occ(ids_o[b], tab, base) for b in range(33)]
        _same(got, gm.group_topk_from(ids_o, scores, tab, walked, 7, 2, base), (C, "id_base"))
        assert (_np(got[1])[_np(got[1]) >= 0] >= base).all()


def test_refused_host_ids_leave_the_outputs_alone(torch_mod, tables):
    ids, scores = gm.lists(2, 65)
    ids[0, 9] = gm.N_ROWS
    with pytest.raises(ValueError, match="candidate id"):
        _ix().group_topk(ids, scores, tables["three"], 3)


# ------------------------------------------------------------------------------------------------ search_grouped
N, D_, NQ = 2000, 64, 6


def _tables_for(n):
    rng = np.random.default_rng(11)
    some = rng.integers(0, 37, size=n).astype(np.int32)
    some[rng.random(n) < 0.1] = -1
    return {"fives": (np.arange(n) // 5).astype(np.int32), "some": some, "three": rng.integers(0, 3, size=n).astype(np.int32)}


def _model_over(D, I, tab, k, gs, id_base=0):
    D, I = _np(D), _np(I)
    return gm.group_topk(I, D, tab, k, gs, id_base)


def _check_grouped(idx, q, tab, k, gs, search_kw=None, grouped_kw=None, id_base=0, what=None):
    """search_grouped against the model over the whole ranking (group_size 1, or everything fetched) and over the
    fetched places; returns the info."""
    search_kw, grouped_kw = search_kw or {}, grouped_kw or {}
    got = idx.search_grouped(q, k, tab, group_size=gs, **search_kw, **grouped_kw)
    info = idx.last_group_info()
    full = idx.search(q, idx.ntotal, **search_kw)
    want_full = _model_over(*full, tab, k, gs, id_base)
    want_fetched = _model_over(*idx.search(q, info["fetched"], **search_kw), tab, k, gs, id_base)
    _same(got, want_fetched[:3], (what, "fetched"))
    assert np.array_equal(info["n_groups"], want_fetched[3])
    nv_full = want_full[4]
    exhaustive = info["fetched"] > nv_full            # (a list that came back full counts as not exhaustive)
    assert np.array_equal(info["complete"], (want_fetched[3] >= k) | exhaustive), what
    if gs == 1 or exhaustive.all():
        rows = np.nonzero(info["complete"])[0]
        for g, w in zip(got, want_full[:3]):
            assert np.array_equal(_np(g)[rows], w[rows]), (what, "whole ranking")
    else:   # the groups and their first rows are the whole ranking's
        first_full = _model_over(*full, tab, k, 1, id_base)[1]
        for b in np.nonzero(info["complete"])[0]:
            I_b, G_b = _np(got[1])[b], _np(got[2])[b]
            seen, firsts = set(), []
            for i, g in zip(I_b.tolist(), G_b.tolist()):
                key = g if g >= 0 else ("single", i)
                if i >= 0 and key not in seen:
                    seen.add(key)
                    firsts.append(i)
            assert firsts == [i for i in first_full[b].tolist() if i >= 0], (what, b)
    return info


@pytest.fixture(scope="module")
def flat_f16(torch_mod):
    c, q, _ = xi.case("ints", N, D_, NQ)
    idx = _ix().FlatIPIndex(D_, dtype="f16")
    idx.add(c)
    qt = torch_mod.from_numpy(q.copy()).cuda()
    D, I = idx.search(qt, N)
    wD, wI = xi.expected_topk(c, q, N)                   # the reference ranking is itself exact here
    assert np.array_equal(_np(I), wI) and np.array_equal(_np(D), wD)
    return idx, c, qt


@pytest.mark.parametrize("gs", GROUP_SIZES)
def test_search_grouped_equals_the_model_over_the_ranking(flat_f16, gs):
    idx, c, qt = flat_f16
    for name, tab in _tables_for(N).items():
        for k in (1, 10, 50):
            info = _check_grouped(idx, qt, tab, k, gs, what=(name, k, gs))
            if name == "three" and k > 3:                      # more groups asked for than exist: exhaustion, padding
                assert info["complete"].all() and info["fetched"] > N and info["rounds"] > 1
                assert (info["n_groups"] == 3).all()
                assert (_np(idx.search_grouped(qt, k, tab, group_size=gs)[1])[:, 3 * gs:] == -1).all()
        info = _check_grouped(idx, qt, tab, 10, gs, grouped_kw={"fetch_k": N + 1}, what=(name, "everything fetched"))
        assert info["rounds"] == 1 and info["complete"].all()
        info = _check_grouped(idx, qt, tab, 10, gs, grouped_kw={"fetch_k": 300}, what=(name, "fetch_k = 300"))
        assert info["fetched"] >= 300 and (info["rounds"] == 1) == (info["fetched"] == 300)


def test_search_grouped_numpy_queries_come_back_as_numpy(flat_f16):
    idx, c, qt = flat_f16
    tab = _tables_for(N)["some"]
    got = idx.search_grouped(_np(qt), 10, tab, group_size=2)
    assert all(isinstance(a, np.ndarray) for a in got)
    _same(got, [_np(t) for t in idx.search_grouped(qt, 10, tab, group_size=2)], "numpy")


def test_search_grouped_fp8_rows(torch_mod):
    rng = np.random.default_rng(5)
    c = rng.integers(-15, 16, size=(N, D_)).astype(np.float32)    # what e4m3 holds exactly at scale exponent 0
    q = rng.integers(-15, 16, size=(NQ, D_)).astype(np.float32)
    idx = _ix().FlatIPIndex(D_, dtype="fp8", fp8_scale_log2=0)
    idx.add(c)
    qt = torch_mod.from_numpy(q).cuda()
    wD, wI = xi.expected_topk(c, q, N)
    D, I = idx.search(qt, N)
    assert np.array_equal(_np(I), wI) and np.array_equal(_np(D), wD)
    for gs in (1, 2):
        _check_grouped(idx, qt, _tables_for(N)["fives"], 10, gs, what=("fp8", gs))


def test_a_crowded_head_makes_the_fetch_grow(torch_mod):
    c, q, _ = xi.case("ints", N, D_, NQ)
    c, q = c.copy(), q.copy()
    c[100:400] = c[100]                                            # 300 copies of one row ...
    q[0] = c[100]                                                  # ... that lead query 0's ranking
    tab = np.arange(1, N + 1, dtype=np.int32)
    tab[100:400] = 0                                               # ... in one group
    idx = _ix().FlatIPIndex(D_, dtype="f16")
    idx.add(c)
    qt = torch_mod.from_numpy(q).cuda()
    D, I = idx.search(qt, 300)
    assert np.array_equal(_np(I)[0], np.arange(100, 400))
    assert _ix().group_default_fetch_k(10) == 64
    for gs in (1, 2):
        info = _check_grouped(idx, qt, tab, 10, gs, what=("crowded", gs))
        # 64 -> 256 -> 1024 places for ten groups behind 300 copies; with two rows each, 80 -> 320
        assert (info["rounds"], info["fetched"]) == {1: (3, 1024), 2: (2, 320)}[gs] and info["complete"].all()
        got = idx.search_grouped(qt, 10, tab, group_size=gs)
        assert _np(got[1])[0, :gs].tolist() == list(range(100, 100 + gs)) and (_np(got[2])[0, gs:] != 0).all()


def test_allowed_rows_removed_rows_and_an_id_offset(torch_mod):
    c, q, _ = xi.case("ints", N, D_, NQ)
    tab = _tables_for(N)["some"]
    idx = _ix().FlatIPIndex(D_, dtype="f16")
    idx.add(c)
    qt = torch_mod.from_numpy(q.copy()).cuda()
    rng = np.random.default_rng(8)
    mask = np.zeros(N, dtype=bool)
    mask[rng.permutation(N)[:40]] = True
    for gs in (1, 2):
        info = _check_grouped(idx, qt, tab, 10, gs, search_kw={"allowed": mask}, what=("allowed", gs))
        assert info["complete"].all() and info["rounds"] == 1        # 40 rows in a fetch of 64: exhaustive at once
        got = idx.search_grouped(qt, 10, tab, group_size=gs, allowed=mask)
        ids = _np(got[1])
        assert mask[ids[ids >= 0]].all()
    gone = rng.permutation(N)[:700]
    assert idx.remove_ids(gone) == 700
    for gs in (1, 2):
        _check_grouped(idx, qt, tab, 10, gs, what=("removed", gs))
        ids = _np(idx.search_grouped(qt, 10, tab, group_size=gs)[1])
        assert not np.isin(ids, gone).any()
    info = _check_grouped(idx, qt, _tables_for(N)["three"], 10, 1, what="removed, exhausted")
    assert info["complete"].all()
    idx2 = _ix().FlatIPIndex(D_, dtype="f16")
    idx2.add(c)
    idx2.set_id_offset(5000)
    for gs in (1, 2):
        _check_grouped(idx2, qt, tab, 10, gs, id_base=5000, what=("offset", gs))
    ids = _np(idx2.search_grouped(qt, 10, tab)[1])
    assert (ids[ids >= 0] >= 5000).all()


def test_ivf_probing_every_list_equals_the_flat_index(flat_f16):
    idx, c, qt = flat_f16
    ivf = _ix().IVFFlatIndex(D_, 8, dtype="f16", nprobe=8)
    ivf.train(c.copy(), seed=1)
    ivf.add(c.copy())
    for name, tab in _tables_for(N).items():
        for k, gs in ((10, 1), (10, 2), (50, 5)):
            a = idx.search_grouped(qt, k, tab, group_size=gs)
            b = ivf.search_grouped(qt, k, tab, group_size=gs, nprobe=8)
            _same(b, [_np(t) for t in a], (name, k, gs))
            ia, ib = idx.last_group_info(), ivf.last_group_info()
            assert ia["fetched"] == ib["fetched"] and ia["rounds"] == ib["rounds"]
            assert np.array_equal(ia["n_groups"], ib["n_groups"]) and np.array_equal(ia["complete"], ib["complete"])


def test_an_incomplete_query_is_reported_not_raised(torch_mod):
    n = gm.N_ROWS
    c, q, _ = xi.case("ints", n, D_, 2)
    idx = _ix().FlatIPIndex(D_, dtype="f16")
    idx.add(c)
    qt = torch_mod.from_numpy(q.copy()).cuda()
    _, head = idx.search(qt[:1], 16384)
    tab = np.full(n, -1, dtype=np.int32)                           # singletons ...
    tab[_np(head)[0]] = 0                                          # ... behind 16384 places of one group (query 0)
    got = idx.search_grouped(qt, 5, tab)
    info = idx.last_group_info()
    assert info["fetched"] == 16384 and info["rounds"] == 5
    assert info["complete"].tolist() == [False, True] and info["n_groups"][0] == 1
    _same(got, _model_over(*idx.search(qt, 16384), tab, 5, 1)[:3], "incomplete")
    assert (_np(got[1])[0, 1:] == -1).all() and (_np(got[1])[1] >= 0).all()


# ------------------------------------------------------------------------------------------------ retriever and pipeline
WORDS = ("neural network attention transformer language retrieval index vector query document "
         "learning model data system search rank score token embedding gpu memory").split()
QUERIES = ["marginal relevance picks results", "gpu memory index", "language retrieval system"]
N_DOCS = 201


def _docs(n=N_DOCS):
    rng = np.random.default_rng(3)
    docs = [" ".join(rng.choice(WORDS, size=int(rng.integers(4, 30)))) for _ in range(n)]
    meta = [{"source": f"s{i // 3}", "i": i} for i in range(n)]          # three documents per source
    for i in range(0, n, 40):
        meta[i] = {"i": i}                                               # ... and a few without one
    return docs, meta


def _want_ids(plain, meta, k, gs, fetched=None):
    """The model over a plain (ungrouped) record list, the search with top_k = n_docs: the doc_ids kept.  With
    ``group_size > 1`` over its first ``fetched`` places, which is what a group's rows are chosen from (for
    ``group_size == 1`` the cut changes nothing: asserted)."""
    if gs == 1 and fetched is not None:
        assert _want_ids(plain, meta, k, 1) == _want_ids(plain[:fetched], meta, k, 1)
    ids = np.array([r["doc_id"] for r in plain[:fetched]], dtype=np.int64)
    codes, table = {}, np.full(len(meta), -1, dtype=np.int32)
    for i, md in enumerate(meta):
        if "source" in md:
            table[i] = codes.setdefault(md["source"], len(codes))
    kept, _, _ = gm.group_select(ids, table, k, gs)
    return ids[kept].tolist()


def _per_source(recs):
    count = {}
    for r in recs:
        s = r["metadata"].get("source")
        if s is not None:
            count[s] = count.get(s, 0) + 1
    return max(count.values(), default=0)


def test_retriever_returns_the_best_groups(tmp_path):
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    cfg = dict(model_name="random:tiny", device="cuda", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
               use_fp16=False)
    r = Stage1Retriever(Stage1Config(enable_bm25=False, **cfg))
    docs, meta = _docs()
    r.add_documents(docs, meta)
    top_k = 5
    plain_k = r.search(QUERIES[0], top_k)
    for q in QUERIES:
        plain = r.search(q, N_DOCS)
        assert len(plain) == N_DOCS
        by_id = {x["doc_id"]: x for x in plain}
        for gs in (1, 2, 3):
            got = r.search(q, top_k, group_by="source", group_size=gs)
            info = r.faiss_index.last_group_info()
            assert info["complete"].all() and info["fetched"] == max(64, 4 * top_k * gs)
            assert [x["doc_id"] for x in got] == _want_ids(plain, meta, top_k, gs, info["fetched"])
            assert _per_source(got) <= gs and len(got) <= top_k * gs
            assert all(x == by_id[x["doc_id"]] for x in got)                 # the records are the plain ones
        codes = np.array([i // 3 for i in range(N_DOCS)], dtype=np.int64)    # an array instead of a key
        got = r.search(q, top_k, group_by=codes, group_size=2)
        fetched = r.faiss_index.last_group_info()["fetched"]
        kept, _, _ = gm.group_select(np.array([x["doc_id"] for x in plain[:fetched]]), codes.astype(np.int32), top_k, 2)
        assert [x["doc_id"] for x in got] == [plain[i]["doc_id"] for i in kept]
    for gs in (1, 2):
        many = r.search_many(QUERIES, top_k, group_by="source", group_size=gs)
        assert r.faiss_index.last_group_info()["complete"].all()
        for q, m in zip(QUERIES, many):
            one = r.search(q, top_k, group_by="source", group_size=gs)
            assert [x["doc_id"] for x in m] == [x["doc_id"] for x in one]
        # the array form has rows of one width: it is there when no query's row is padded (with group_size 1: when
        # every query is complete), else the caller takes the record path
        arrs = r.search_many_arrays(QUERIES, top_k, group_by="source", group_size=gs)
        assert (arrs is not None) == all(len(m) == top_k * gs for m in many)
        assert arrs is not None or gs > 1
        if arrs is not None:
            assert arrs[0].shape == (len(QUERIES), top_k * gs)
            assert arrs[0].cpu().tolist() == [[x["doc_id"] for x in m] for m in many]
    # unset, nothing changes: the config's defaults are off, and group_size alone means nothing
    assert r.config.group_by is None and r.search(QUERIES[0], top_k) == plain_k
    assert r.search(QUERIES[0], top_k, group_size=3) == plain_k
    D, I = r.faiss_index.search(r._normalized_query_tensor([QUERIES[0]]), top_k)
    assert [x["doc_id"] for x in plain_k] == I[0].tolist() and [x["score"] for x in plain_k] == D[0].tolist()
    r.config.group_by, r.config.group_size = "source", 2                     # the config's values are the default
    assert r.search(QUERIES[0], top_k) == r.search(QUERIES[0], top_k, group_by="source", group_size=2)
    with pytest.raises(ValueError, match="mmr_lambda"):
        r.search(QUERIES[0], top_k, mmr_lambda=0.5)
    r.config.group_by, r.config.group_size = None, 1
    # documents added later extend the table; removal + compaction renumber it
    r.add_documents(["gpu memory index vector"] * 4, [{"source": "late"}] * 4)
    got = r.search("gpu memory index vector", 3, group_by="source")
    assert sum(x["metadata"].get("source") == "late" for x in got) == 1
    r.remove_documents(list(range(0, 90)))
    r.compact()
    meta2 = list(r.doc_metadata)
    assert len(meta2) == N_DOCS + 4 - 90 and meta2[0]["i"] == 90
    for q in QUERIES:
        plain = r.search(q, len(meta2))
        for gs in (1, 2):
            got = r.search(q, top_k, group_by="source", group_size=gs)
            fetched = r.faiss_index.last_group_info()["fetched"]
            assert [x["doc_id"] for x in got] == _want_ids(plain, meta2, top_k, gs, fetched)
            assert all(x["metadata"] is meta2[x["doc_id"]] for x in got)
    fused = Stage1Retriever(Stage1Config(enable_bm25=True, **cfg))
    fused.add_documents(docs, meta)
    with pytest.raises(ValueError, match="BM25"):
        fused.search(QUERIES[0], top_k, group_by="source")
    with pytest.raises(ValueError, match="BM25"):
        fused.search_many(QUERIES, top_k, group_by="source")
    assert len(fused.search(QUERIES[0], top_k)) == top_k


def _pipeline(tmp_path, name, **extra):
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    pc = PipelineConfig(stage1_model="random:tiny", stage2_model="random:tiny", stage3_model="random:tiny",
                        device="cuda", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
                        log_file=str(tmp_path / f"{name}.log"), stage1_top_k=40, stage2_top_k=30, stage3_top_k=20,
                        stage1_use_fp16=False, stage2_use_fp16=False, stage3_use_fp16=False,
                        stage1_enable_bm25=False, save_intermediate_results=True, **extra)
    p = RetrievalPipeline(config=pc)
    p.initialize_stages()
    p.add_documents(*_docs())
    return p


def test_pipeline_collapses_at_stage_one_on_both_paths(tmp_path):
    rec = _pipeline(tmp_path, "rec")
    arr = _pipeline(tmp_path, "arr", stage2_precompute_document_embeddings=True, stage3_cache_document_tokens=True)
    assert arr._arrays_ready() and not rec._arrays_ready()
    assert arr.stage1.search_many_arrays(QUERIES, 40, group_by="source") is not None     # (the array path is taken)
    _, meta = _docs()
    out = {}
    for name, p in (("rec", rec), ("arr", arr)):
        plain_before = [p.search(q) for q in QUERIES]
        for q in QUERIES:
            plain1 = p.stage1.search(q, N_DOCS)
            for gs in (1, 2):
                res = p.search(q, group_by="source", group_size=gs)
                s1 = [x["doc_id"] for x in res["stage1_results"]]
                fetched = p.stage1.faiss_index.last_group_info()["fetched"]
                assert s1 == _want_ids(plain1, meta, 40, gs, fetched)         # stage1_top_k counts groups
                assert len(s1) >= 40
                assert _per_source(res["stage1_results"]) <= gs and _per_source(res["stage2_results"]) <= gs
                assert _per_source(res["results"]) <= gs and 0 < len(res["results"]) <= 20
                assert {x["doc_id"] for x in res["results"]} <= set(s1)
                out[name, q, gs] = res
        many = p.search_many(QUERIES, group_by="source", group_size=2)
        batch = p.batch_search(QUERIES, group_by="source", group_size=2)
        for q, m, b in zip(QUERIES, many, batch):
            want = [x["doc_id"] for x in out[name, q, 2]["stage1_results"]]
            assert [x["doc_id"] for x in m["stage1_results"]] == want
            assert [x["doc_id"] for x in b["stage1_results"]] == want
            assert _per_source(m["results"]) <= 2
        with pytest.raises(ValueError, match="mmr_lambda"):
            p.search(QUERIES[0], group_by="source", mmr_lambda=0.5)
        # unset, the pipeline returns what it returned: bit for bit
        for q, before in zip(QUERIES, plain_before):
            again = p.search(q, group_size=3)
            assert again["results"] == before["results"] and again["stage1_results"] == before["stage1_results"]
    for q in QUERIES:                                                          # the two paths agree
        for gs in (1, 2):
            a, r = out["arr", q, gs], out["rec", q, gs]
            assert [x["doc_id"] for x in a["stage1_results"]] == [x["doc_id"] for x in r["stage1_results"]]
            assert [x["stage1_score"] for x in a["stage1_results"]] == [x["stage1_score"] for x in r["stage1_results"]]
            sa = {x["doc_id"]: x["stage2_score"] for x in a["stage2_results"]}
            sr = {x["doc_id"]: x["stage2_score"] for x in r["stage2_results"]}
            common = sorted(set(sa) & set(sr))
            assert len(common) >= 25                                           # (near-ties may swap the last places)
            np.testing.assert_allclose([sa[i] for i in common], [sr[i] for i in common], atol=1e-4)
    cfg = _pipeline(tmp_path, "cfg", group_by="source", group_size=2)          # the config's values are the default
    for q in QUERIES:
        res = cfg.search(q)
        assert [x["doc_id"] for x in res["stage1_results"]] == [x["doc_id"] for x in out["rec", q, 2]["stage1_results"]]
