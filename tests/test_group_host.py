"""CPU checks of grouped search: the host model of tests/group_model.py against a brute force written
differently and against its properties, and the boundary (argument errors of the library and of Python, the C ABI, the
retriever's key -> code tables, refusals, config defaults) as far as it can be reached without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import group_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_case(rng, C, n_rows):
    groups = rng.integers(-2, 4, size=n_rows).astype(np.int32)
    id_base = int(rng.integers(-3, 4))
    ids = rng.integers(-2, n_rows + 2, size=C).astype(np.int64) + id_base    # rows -2 .. n_rows + 1: some outside
    ids[rng.random(C) < 0.2] = -1
    return ids, groups, id_base


# ------------------------------------------------------------------ the model
def test_model_equals_brute_force_on_small_lists():
    rng = np.random.default_rng(1)
    n = 0
    for _ in range(1500):
        C = int(rng.integers(1, 13))
        ids, groups, id_base = _random_case(rng, C, int(rng.integers(1, 9)))
        for k in (1, 2, 3, C, C + 2):
            for gs in (1, 2, 3, C):
                assert gm.group_select(ids, groups, k, gs, id_base) == gm.group_brute_force(ids, groups, k, gs, id_base), \
                    (ids, groups, id_base, k, gs)
                n += 1
    assert n == 30000


def test_model_properties():
    rng = np.random.default_rng(2)
    for _ in range(400):
        C = int(rng.integers(1, 40))
        ids, groups, id_base = _random_case(rng, C, 12)
        k, gs = int(rng.integers(1, 6)), int(rng.integers(1, 4))
        kept, n_groups, n_valid = gm.group_select(ids, groups, k, gs, id_base)
        assert kept == sorted(kept) and len(set(kept)) == len(kept)                  # ascending positions
        valid = [i for i in range(C) if gm.is_valid(ids[i], id_base, len(groups))]
        assert n_valid == len(valid) and set(kept) <= set(valid)
        g_of = {i: int(groups[int(ids[i]) - id_base]) for i in valid}
        per = {}
        for i in kept:
            key = g_of[i] if g_of[i] >= 0 else ("single", i)
            per[key] = per.get(key, 0) + 1
        assert all(c <= gs for c in per.values()) and len(per) <= k                  # group_size per group, k groups
        named = {g for g in g_of.values() if g >= 0}
        assert n_groups == len(named) + sum(1 for g in g_of.values() if g < 0)       # ungrouped entries: one each
        D, I, G = gm.group_output(ids, np.arange(C, 0, -1), groups, kept, k, gs, id_base)
        assert (I[len(kept):] == -1).all() and (G[len(kept):] == -1).all() and (D[len(kept):] == -gm.FLT_MAX).all()
        assert I[: len(kept)].tolist() == [int(ids[i]) for i in kept]
        assert all(g >= -1 for g in G)
        # nothing to collapse: the list without its padding
        kept_all, _, _ = gm.group_select(ids, groups, C, C, id_base)
        assert kept_all == valid


def test_duplicated_ids_count_twice_and_ungrouped_entries_stand_alone():
    groups = np.array([7, 7, -1, 3], dtype=np.int32)
    ids = np.array([0, 0, 1, 0, 2, 2, 3], dtype=np.int64)
    assert gm.group_select(ids, groups, 5, 2) == ([0, 1, 4, 5, 6], 4, 7)   # group 7 full after 0, 0; row 2 twice: two groups
    assert gm.group_select(ids, groups, 2, 1) == ([0, 4], 4, 7)            # n_groups is not capped at k
    assert gm.group_select(ids, groups, 5, 9) == (list(range(7)), 4, 7)
    assert gm.group_select(ids + 100, groups, 2, 1, id_base=100) == ([0, 4], 4, 7)
    D, I, G, ng, nv = gm.group_topk(ids[None], np.arange(7, 0, -1)[None], groups, 3, 1)
    assert I.tolist() == [[0, 2, 2]] and G.tolist() == [[7, -1, -1]] and D.tolist() == [[7.0, 3.0, 2.0]]
    assert ng.tolist() == [4] and nv.tolist() == [7]


def test_walking_a_list_once_gives_the_selection_of_every_k_and_group_size():
    """What tests/test_group_gpu.py computes its expectations from equals the definition's loop."""
    rng = np.random.default_rng(4)
    for _ in range(200):
        B, C = 3, int(rng.integers(1, 30))
        groups = rng.integers(-2, 5, size=15).astype(np.int32)
        id_base = int(rng.integers(0, 3)) * 100
        ids = rng.integers(-1, 17, size=(B, C)).astype(np.int64)
        ids[ids >= 0] += id_base
        scores = rng.standard_normal((B, C)).astype(np.float32)
        walked = [gm.group_rank_occ(ids[b], groups, id_base) for b in range(B)]
        for k, gs in ((1, 1), (2, 3), (C, 1), (3, C), (C + 1, C + 1)):
            want = gm.group_topk(ids, scores, groups, k, gs, id_base)
            got = gm.group_topk_from(ids, scores, groups, walked, k, gs, id_base)
            for w, g in zip(want, got):
                assert w.dtype == g.dtype and np.array_equal(w, g), (ids, groups, k, gs)


def test_gpu_test_inputs_are_what_they_claim():
    tabs = gm.tables()
    assert set(tabs) == {"one", "distinct", "none", "three", "fives", "heavy"}
    assert all(t.shape == (gm.N_ROWS,) and t.dtype == np.int32 for t in tabs.values())
    assert len(set(tabs["distinct"].tolist())) == gm.N_ROWS and (tabs["none"] == -1).all()
    assert set(tabs["three"].tolist()) == {0, 1, 2} and (tabs["heavy"] == -1).any()
    counts = np.bincount(tabs["heavy"][tabs["heavy"] >= 0])
    assert counts.max() > 2000 and (counts == 1).sum() > 20                  # heavy-tailed
    ids, sc = gm.lists(33, 65, out_of_range=True)
    assert (ids[32] == -1).all() and (ids[0] >= 0).all() and len(set(ids[0].tolist())) == 65
    assert (ids[1] == -1).any() and (ids[1][-16:] == -1).all()
    assert len(set(ids[2].tolist())) < 65
    assert ((ids[3] >= gm.N_ROWS) | (ids[3] < -1)).any()
    assert (np.diff(sc, axis=1) < 0).all()
    ids2, _ = gm.lists(1, 65, id_base=1000)
    assert ids2.min() >= 1000 and np.array_equal(ids2 - 1000, gm.lists(1, 65)[0])


# ------------------------------------------------------------------ the boundary
def test_header_declares_and_library_exports_the_entry_point():
    from tristage_rag_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tristage.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bts_group_topk\s*\(", text)
    assert "ts_group_topk" in _lib.SIGNATURES and hasattr(lib, "ts_group_topk")
    assert len(_lib.SIGNATURES["ts_group_topk"][1]) == 17
    assert _lib.header_abi_version() == 4
    assert "ts_group.hip" in open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()


def _call(lib, **over):
    p = ctypes.c_void_p(4096)      # never dereferenced: the calls fail first
    a = dict(ids=p, scores=p, nq=1, ncand=10, groups=p, n_rows=100, id_base=0, k=3, group_size=1, D=p, I=p, G=p, ng=p, nv=p,
             flags=0, device=0, stream=None)
    a.update(over)
    return lib.ts_group_topk(a["ids"], a["scores"], a["nq"], a["ncand"], a["groups"], a["n_rows"], a["id_base"], a["k"],
                             a["group_size"], a["D"], a["I"], a["G"], a["ng"], a["nv"], a["flags"], a["device"], a["stream"])


def test_entry_point_validates_arguments_without_a_gpu():
    from tristage_rag_amd import _lib
    lib = _lib.load()
    for name in ("ids", "scores", "groups", "D", "I", "G", "ng", "nv"):
        assert _call(lib, **{name: None}) == _lib.TS_ERR_INVALID, name
        assert b"null pointer" in lib.ts_last_error()
    for over, word in (({"k": 0}, b"k = 0"), ({"k": -3}, b"k = -3"), ({"group_size": 0}, b"group_size = 0"),
                       ({"ncand": 0}, b"ncand"), ({"ncand": -1}, b"ncand"), ({"nq": -1}, b"nq"), ({"n_rows": -1}, b"n_rows")):
        assert _call(lib, **over) == _lib.TS_ERR_INVALID, over
        assert word in lib.ts_last_error(), (over, lib.ts_last_error())
    assert _call(lib, ncand=16385) == _lib.TS_ERR_UNSUPPORTED and b"16384" in lib.ts_last_error()
    assert _call(lib, k=8193, group_size=2) == _lib.TS_ERR_UNSUPPORTED and b"16384" in lib.ts_last_error()
    assert _call(lib, k=16385) == _lib.TS_ERR_UNSUPPORTED
    assert _call(lib, k=1 << 30, group_size=1 << 30) == _lib.TS_ERR_UNSUPPORTED    # (the product is taken in 64 bits)
    assert _call(lib, nq=0) == _lib.TS_OK
    assert _call(lib, nq=0, ids=None, D=None) == _lib.TS_OK
    # host pointers: an id that is neither padding nor a row of the table fails the call before anything is written
    ids = np.array([[3, -1, 7, 12]], dtype=np.int64)
    sc = np.zeros((1, 4), dtype=np.float32)
    tab = np.zeros(12, dtype=np.int32)
    out = np.full(8, 77, dtype=np.int64)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for bad, base in ((12, 0), (-2, 0), (2, 3), (1 << 40, 0), (-(1 << 62), 1 << 62)):
        ids[0, 3] = bad
        st = _call(lib, ids=hp(ids), scores=hp(sc), ncand=4, groups=hp(tab), n_rows=12, id_base=base, k=2,
                   D=hp(out), I=hp(out), G=hp(out), ng=hp(out), nv=hp(out), flags=_lib.TS_FLAG_HOST_PTR)
        assert st == _lib.TS_ERR_INVALID and b"candidate id" in lib.ts_last_error(), (bad, base)
        assert (out == 77).all()


def test_python_argument_errors_are_raised_before_anything_is_launched():
    from tristage_rag_amd import index
    assert index.group_default_fetch_k(1) == 64 and index.group_default_fetch_k(20) == 80
    assert index.group_default_fetch_k(20, 5) == 400 and index.group_default_fetch_k(5000, 2) == 16384
    assert index.group_check(3, 2, 10) == (3, 2, 10)
    assert index.group_check(20, 1, 5) == (20, 1, 5)                      # k > C is allowed
    for args, word in (((0, 1, 10), "k must"), ((1, 0, 10), "group_size"), ((8193, 2, 10), "16384"), ((1, 1, 0), "at least"),
                       ((1, 1, 16385), "16384")):
        with pytest.raises(ValueError, match=word):
            index.group_check(*args)
    ids = np.zeros((2, 8), dtype=np.int64)
    sc = np.zeros((2, 8), dtype=np.float32)
    tab = np.zeros(5, dtype=np.int32)
    with pytest.raises(ValueError, match="k must"):
        index.group_topk(ids, sc, tab, 0)
    with pytest.raises(ValueError, match="group_size"):
        index.group_topk(ids, sc, tab, 2, group_size=0)
    with pytest.raises(ValueError, match="shape"):
        index.group_topk(ids, sc[:, :4], tab, 2)
    with pytest.raises(ValueError, match="one-dimensional"):
        index.group_topk(ids, sc, np.zeros((5, 1), np.int32), 2)
    with pytest.raises(ValueError, match="candidate id"):               # the library's host check, through Python
        index.group_topk(ids + 5, sc, tab, 2)
    q = np.zeros((2, 16), dtype=np.float32)
    for cls in (index.FlatIPIndex, index.IVFFlatIndex):
        ix = cls.__new__(cls)          # no handle: whatever reached the library would fail differently
        ix.__class__ = type("Sized", (cls,), {"ntotal": property(lambda self: 5), "__del__": lambda self: None})
        with pytest.raises(ValueError, match="k must"):
            ix.search_grouped(q, 0, tab)
        with pytest.raises(ValueError, match="group_size"):
            ix.search_grouped(q, 2, tab, group_size=0)
        with pytest.raises(ValueError, match="16384"):
            ix.search_grouped(q, 2, tab, fetch_k=16385)
        with pytest.raises(ValueError, match="5 rows"):
            ix.search_grouped(q, 2, np.zeros(4, np.int32))
        assert ix.last_group_info() == {}


# ------------------------------------------------------------------ the retriever's group tables
def _bare_retriever(metadata, enable_bm25=False):
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    r = Stage1Retriever.__new__(Stage1Retriever)
    r.config, r.bm25_index, r.faiss_index = Stage1Config(enable_bm25=enable_bm25), None, None
    r.doc_metadata = list(metadata)
    r.documents = ["text"] * len(r.doc_metadata)
    r._kv_bitmaps, r._mask_lru = {}, {}
    r._reset_filter_caches()
    return r


def test_group_codes_first_seen_order_missing_key_extension_and_rebuild():
    md = [{"source": "b"}, {"source": "a"}, {}, {"source": "b"}, {"source": ("t", 1)}, {"other": 1}, {"source": None}]
    r = _bare_retriever(md)
    codes = r._group_codes("source")
    assert codes.dtype == np.int32 and codes.tolist() == [0, 1, -1, 0, 2, -1, 3]      # None is a value; no key: -1
    assert r._group_codes("source") is codes                                          # cached
    assert r._group_codes("other").tolist() == [-1, -1, -1, -1, -1, 0, -1]
    # add_documents appends to the same lists: the table is extended, old codes keep their meaning
    r.doc_metadata.extend([{"source": "a"}, {"source": "z"}])
    r.documents.extend(["text"] * 2)
    assert r._group_codes("source").tolist() == [0, 1, -1, 0, 2, -1, 3, 1, 4]
    assert np.array_equal(r._group_table("source", on_device=False), r._group_codes("source"))
    # compact / load_index replace the metadata list: the table is rebuilt from it
    r.doc_metadata = [md[1], md[3], {"source": "z"}]
    r.documents = ["text"] * 3
    assert r._group_codes("source").tolist() == [0, 1, 2]
    # update_documents rewrites entries of the same list and resets the caches
    r.doc_metadata[0] = {"source": "z"}
    r._reset_filter_caches()
    assert r._group_codes("source").tolist() == [0, 1, 0]
    r.doc_metadata.append({"source": ["unhashable"]})
    r.documents.append("text")
    with pytest.raises(TypeError, match="unhashable"):
        r._group_codes("source")


def test_group_by_accepts_an_integer_array_over_the_documents():
    r = _bare_retriever([{}] * 4)
    assert r._group_table([5, 5, -1, 2], on_device=False).tolist() == [5, 5, -1, 2]
    assert r._group_table(np.array([1, 2, 3, 4], dtype=np.int64), on_device=False).dtype == np.int32
    with pytest.raises(ValueError, match="one entry per document"):
        r._group_table(np.zeros(3, dtype=np.int64), on_device=False)
    with pytest.raises(ValueError, match="one entry per document"):
        r._group_table(np.zeros(4, dtype=np.float32), on_device=False)
    with pytest.raises(ValueError, match="32 bits"):
        r._group_table(np.array([0, 1, 2, 1 << 40]), on_device=False)


def test_group_args_defaults_and_refusals():
    from tristage_rag_amd.stage1_retriever import Stage1Config
    assert Stage1Config().group_by is None and Stage1Config().group_size == 1
    r = _bare_retriever([{}] * 3)
    assert r._group_args(None, 1) is None
    assert r._group_args("source", 2) == ("source", 2)
    r.config = Stage1Config(enable_bm25=False, group_by="source", group_size=3)
    assert r._group_args(None, 1) == ("source", 3)                 # the config's
    assert r._group_args("other", 1) == ("other", 1)               # the call's
    with pytest.raises(ValueError, match="group_size"):
        r._group_args("source", 0)
    with pytest.raises(ValueError, match="mmr_lambda"):
        r._group_args("source", 1, 0.5)
    r.faiss_index = object()
    with pytest.raises(NotImplementedError, match="search_grouped"):
        r._group_args("source", 1)
    r.faiss_index = None
    r.config, r.bm25_index = Stage1Config(enable_bm25=True), object()          # BM25 fusion on
    assert r._group_args(None, 1) is None
    with pytest.raises(ValueError, match="BM25"):
        r._group_args("source", 1)
    with pytest.raises(ValueError, match="BM25"):
        r.faiss_index = object()
        r.search("a query", 3, group_by="source")


def test_pipeline_config_defaults_and_mmr_conflict(tmp_path):
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    assert PipelineConfig().group_by is None and PipelineConfig().group_size == 1
    p = RetrievalPipeline(config=PipelineConfig(log_file=str(tmp_path / "p.log")))
    assert p._group_kwargs(None, 1, None) == {}
    assert p._group_kwargs("source", 2, None) == {"group_by": "source", "group_size": 2}
    with pytest.raises(ValueError, match="mmr_lambda"):
        p._group_kwargs("source", 1, 0.5)
    with pytest.raises(ValueError, match="group_size"):
        p._group_kwargs("source", 0, None)
    p2 = RetrievalPipeline(config=PipelineConfig(log_file=str(tmp_path / "p.log"), group_by="source", group_size=4))
    assert p2._group_kwargs(None, 1, None) == {"group_by": "source", "group_size": 4}


def test_sharded_classes_refuse(tmp_path):
    from tristage_rag_amd.parallel_pipeline import ShardedRetrievalPipeline
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig
    from tristage_rag_amd.sharded import ShardedFlatIPIndex
    sh = ShardedFlatIPIndex.__new__(ShardedFlatIPIndex)
    with pytest.raises(NotImplementedError):
        sh.search_grouped(np.zeros((1, 8), np.float32), 2, np.zeros(4, np.int32))
    kw = dict(stage1_model="random:tiny", stage2_model="random:tiny", stage3_model="random:tiny", device="cpu",
              cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"), log_file=str(tmp_path / "p.log"))
    p = ShardedRetrievalPipeline(config=PipelineConfig(**kw))
    with pytest.raises(NotImplementedError, match="group_by"):
        p.search("a query", group_by="source")
    with pytest.raises(NotImplementedError, match="group_by"):
        p.search_many(["a query"], group_by="source")
    with pytest.raises(NotImplementedError, match="group_by"):
        p.batch_search(["a query"], group_by="source")
    p2 = ShardedRetrievalPipeline(config=PipelineConfig(group_by="source", **kw))
    with pytest.raises(NotImplementedError, match="group_by"):
        p2.search("a query")
