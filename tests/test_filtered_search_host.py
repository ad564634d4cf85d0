"""Filtered search, host side (no GPU): filter specs -> bitmaps, mask packing, argument checks of the new C entry
points, their bindings, and the stage-1 / pipeline logic over a filter-aware CPU index double."""
import json
import os

import numpy as np
import pytest
import torch

from doubles import OracleIndex, oracle_maxsim
from oracle import oracle
from tristage_rag_amd import _lib
from tristage_rag_amd.encoders import SentenceEncoder
from tristage_rag_amd.index import pack_allowed
from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
from tristage_rag_amd.stage1_retriever import BM25Index, Stage1Config, Stage1Retriever
from tristage_rag_amd.stage2_rescorer import ColBERTScorer, Stage2Config
from tristage_rag_amd.stage3_reranker import AdaptiveCrossEncoderReranker, Stage3Config

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kat.json")))
DOCS = KAT["bm25"]["documents"]


class FilteredOracleIndex(OracleIndex):
    """OracleIndex with FlatIPIndex's ``allowed=`` contract: the oracle run on the allowed rows, ids mapped back,
    padded with -1 / -FLT_MAX."""

    def search(self, q, k, exact_dense=False, allowed=None):
        if allowed is None:
            return super().search(q, k, exact_dense)
        was_tensor = torch.is_tensor(q)
        qn = q.detach().cpu().float().numpy() if was_tensor else np.asarray(q, np.float32)
        qn = oracle.quantize(qn, self.dtype)
        B, n = qn.shape[0], self.ntotal
        items = list(allowed) if isinstance(allowed, (list, tuple)) else [allowed] * B
        D = np.full((B, k), -3.4028234663852886e38, np.float32)
        I = np.full((B, k), -1, np.int64)
        for b, a in enumerate(items):
            m = np.ones(n, bool) if a is None else unpack(pack_allowed(a, n), n)
            rows = np.flatnonzero(m)
            if rows.size == 0:
                continue
            d, i = oracle.ip_topk(self.rows[rows], qn[b:b + 1], int(k))
            ok = i[0] >= 0
            D[b, ok], I[b, ok] = d[0, ok], rows[i[0, ok]] + self.id_offset
        return (torch.from_numpy(D), torch.from_numpy(I)) if was_tensor else (D, I)


def unpack(words, n):
    return np.unpackbits(np.asarray(words, np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


@pytest.fixture(scope="module")
def encoder():
    return SentenceEncoder("random:tiny", device="cpu")


META = [{"tenant": "a" if i % 3 else "b", "lang": ("en", "de", "fr")[i % 3], "i": i} for i in range(len(DOCS))]


def _stage1(encoder, tmp_path, **kw):
    cfg = Stage1Config(model_name="random:tiny", device="cpu", cache_dir=str(tmp_path / "m"),
                       index_dir=str(tmp_path / "i"), **kw)
    return Stage1Retriever(cfg, model=encoder, index_factory=lambda d: FilteredOracleIndex(d))


# ------------------------------------------------------------------ masks
def test_pack_allowed_bit_order():
    n = 70
    m = np.zeros(n, bool)
    m[[0, 5, 31, 32, 64, 69]] = True
    w = pack_allowed(m, n)
    assert w.dtype == np.uint32 and w.shape == (3,)
    assert w[0] == (1 | (1 << 5) | (1 << 31)) and w[1] == 1 and w[2] == (1 | (1 << 5))
    np.testing.assert_array_equal(unpack(w, n), m)
    # packed input: bits at or beyond n are cleared, the words pass through otherwise
    np.testing.assert_array_equal(pack_allowed(np.full(3, 0xFFFFFFFF, np.uint32), n), [0xFFFFFFFF, 0xFFFFFFFF, 0x3F])
    np.testing.assert_array_equal(pack_allowed(torch.from_numpy(m), n), w)
    with pytest.raises(ValueError):
        pack_allowed(np.ones(n - 1, bool), n)
    with pytest.raises(ValueError):
        pack_allowed(np.ones(2, np.uint32), n)


def test_filter_specs_to_bitmaps(encoder, tmp_path):
    s1 = _stage1(encoder, tmp_path)
    s1.add_documents(DOCS, META)
    n = len(DOCS)
    tenant_a = np.array([md["tenant"] == "a" for md in META])
    np.testing.assert_array_equal(s1.filter_mask({"tenant": "a"}), tenant_a)
    np.testing.assert_array_equal(s1.filter_mask({"tenant": "a", "lang": "de"}),
                                  tenant_a & np.array([md["lang"] == "de" for md in META]))
    np.testing.assert_array_equal(s1.filter_mask({"lang": ["en", "fr"]}), np.array([md["lang"] != "de" for md in META]))
    np.testing.assert_array_equal(s1.filter_mask({"lang": {"en"}}), np.array([md["lang"] == "en" for md in META]))
    np.testing.assert_array_equal(s1.filter_mask({"missing": 1}), np.zeros(n, bool))
    np.testing.assert_array_equal(s1.filter_mask(lambda md: md["i"] >= 4), np.arange(n) >= 4)
    np.testing.assert_array_equal(s1.filter_mask([0, 2]), np.isin(np.arange(n), [0, 2]))
    np.testing.assert_array_equal(s1.filter_mask(np.arange(n) % 2 == 0), np.arange(n) % 2 == 0)
    assert s1.filter_mask(None) is None
    with pytest.raises(ValueError):
        s1.filter_mask([n])
    with pytest.raises(ValueError):
        s1.filter_mask(np.ones(n + 1, bool))
    # (key, value) bitmaps are built once and extended by add_documents
    assert s1._kv_bitmaps[("tenant", "a")].shape == (n,)
    s1.add_documents(["an extra document about tenants"], [{"tenant": "a", "lang": "en", "i": n}])
    m = s1.filter_mask({"tenant": "a"})
    assert m.shape == (n + 1,) and m[-1] and s1._kv_bitmaps[("tenant", "a")].shape == (n + 1,)
    np.testing.assert_array_equal(m[:n], tenant_a)


def test_per_query_filter_lists(encoder, tmp_path):
    s1 = _stage1(encoder, tmp_path)
    s1.add_documents(DOCS, META)
    n = len(DOCS)
    ms = s1._filter_masks([{"tenant": "b"}, None], 2)
    assert ms[1] is None and ms[0].sum() == sum(md["tenant"] == "b" for md in META)
    ms = s1._filter_masks([1, 3], 2)          # a list of ints is ONE filter (document indices)
    np.testing.assert_array_equal(ms[0], np.isin(np.arange(n), [1, 3]))
    assert ms[1] is ms[0]
    assert s1._filter_masks(None, 3) is None


# ------------------------------------------------------------------ C ABI
def test_signatures_bind_new_entry_points():
    for name in ("ts_index_search_filtered", "ts_index_last_filter_info", "ts_bm25_search_batch_filtered"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.ts_abi_version() == _lib.header_abi_version() == 4
    assert lib.ts_index_search_filtered.argtypes == _lib.SIGNATURES["ts_index_search_filtered"][1]


def test_filtered_argument_errors_without_gpu():
    lib = _lib.load()
    q = np.zeros((2, 32), np.float32)
    D = np.empty((2, 5), np.float32)
    I = np.empty((2, 5), np.int64)
    bits = np.zeros((2, 4), np.uint32)

    def call(bits_ptr, words, n_masks, moq, k=5, h=None):
        return lib.ts_index_search_filtered(h, q.ctypes.data, 2, _lib.TS_F32, k, bits_ptr, words, n_masks,
                                            None if moq is None else moq.ctypes.data, D.ctypes.data, I.ctypes.data,
                                            _lib.TS_FLAG_HOST_PTR, None)

    ok_moq = np.array([0, -1], np.int32)
    assert call(None, 4, 2, ok_moq) == _lib.TS_ERR_INVALID and "allow_bits is null" in _lib.last_error()
    assert call(bits.ctypes.data, 4, 1, np.array([0, 1], np.int32)) == _lib.TS_ERR_INVALID
    assert "mask_of_query[1]" in _lib.last_error()
    assert call(bits.ctypes.data, 4, 2, np.array([-2, 0], np.int32)) == _lib.TS_ERR_INVALID
    assert "mask_of_query[0]" in _lib.last_error()
    assert call(bits.ctypes.data, 4, 2, None) == _lib.TS_ERR_INVALID and "mask_of_query is null" in _lib.last_error()
    assert call(bits.ctypes.data, -1, 2, ok_moq) == _lib.TS_ERR_INVALID
    assert call(bits.ctypes.data, 4, 2, ok_moq, k=0) == _lib.TS_ERR_INVALID
    assert call(bits.ctypes.data, 4, 2, ok_moq) == _lib.TS_ERR_INVALID and "null handle" in _lib.last_error()
    info = (_lib.c_int64 * 4)()
    assert lib.ts_index_last_filter_info(None, info) == _lib.TS_ERR_INVALID
    terms = np.zeros(1, np.int32)
    off = np.array([0, 1, 1], np.int64)
    sc = np.zeros((2, 5), np.float64)
    ids = np.zeros((2, 5), np.int64)
    n_out = np.zeros(2, np.int32)
    st = lib.ts_bm25_search_batch_filtered(None, terms.ctypes.data, off.ctypes.data, 2, 5, bits.ctypes.data, 4, 1,
                                           np.array([0, 3], np.int32).ctypes.data, _lib.TS_FLAG_HOST_PTR,
                                           sc.ctypes.data, ids.ctypes.data, n_out.ctypes.data, None)
    assert st == _lib.TS_ERR_INVALID and "mask_of_query[1]" in _lib.last_error()


# ------------------------------------------------------------------ BM25 (host scoring)
def test_bm25_host_filter_ranks_allowed_only():
    bm = BM25Index()
    bm.fit(DOCS)
    n = len(DOCS)
    allowed = np.arange(n) % 2 == 1
    q = "neural networks attention"
    s = bm.scores(q)
    got = bm.search(q, 4, allowed=allowed)
    cand = np.flatnonzero(allowed)
    want = cand[np.argsort(-s[cand], kind="stable")[:4]]
    assert [i for i, _ in got] == want.tolist()
    assert all(allowed[i] for i, _ in got)
    assert bm.search(q, 4, allowed=np.zeros(n, bool)) == []
    # zero-score padding takes allowed documents only (ascending id)
    pad = bm._pad_with_zero_scores([], 3, allowed)
    assert [i for i, _ in pad] == cand[:3].tolist()


# ------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("bm25", [False, True])
def test_stage1_filtered_equals_subcorpus(encoder, tmp_path, bm25):
    """Stage 1 with a filter over the full corpus == stage 1 over the allowed sub-corpus, ids mapped back."""
    full = _stage1(encoder, tmp_path / "full", enable_bm25=bm25)
    full.add_documents(DOCS, META)
    keep = [i for i, md in enumerate(META) if md["tenant"] == "a"]
    sub = _stage1(encoder, tmp_path / "sub", enable_bm25=bm25)
    sub.add_documents([DOCS[i] for i in keep], [META[i] for i in keep])
    for q in ("neural networks attention", "language models", "zzz unknown"):
        got = full.search(q, 3, filter={"tenant": "a"})
        want = sub.search(q, 3)
        assert [r["doc_id"] for r in got] == [keep[r["doc_id"]] for r in want]
        assert all(META[r["doc_id"]]["tenant"] == "a" for r in got)
        if not bm25:   # (the sub-corpus is encoded in other batches: its embeddings may differ in the last bit)
            np.testing.assert_allclose([r["score"] for r in got], [r["score"] for r in want], atol=1e-6, rtol=0)
    assert full.search("language models", 3, filter={"tenant": "nobody"}) == []
    many = full.search_many(["neural networks attention", "language models"], 3,
                            filter=[{"tenant": "a"}, lambda md: md["lang"] == "de"])
    assert all(META[r["doc_id"]]["tenant"] == "a" for r in many[0])
    assert all(META[r["doc_id"]]["lang"] == "de" for r in many[1])
    one = full.search_many(["neural networks attention"], 3, filter=[0, 1])   # document indices
    assert {r["doc_id"] for r in one[0]} <= {0, 1}


def test_stage1_search_many_arrays_filtered(encoder, tmp_path):
    s1 = _stage1(encoder, tmp_path, enable_bm25=True)
    s1.add_documents(DOCS, META)
    qs = ["neural networks attention", "language models"]
    flt = {"tenant": "a"}
    arr = s1.search_many_arrays(qs, 2, filter=flt)
    rec = s1.search_many(qs, 2, filter=flt)
    assert arr is not None
    ids, _ = arr
    for q in range(2):
        assert ids[q].tolist() == [r["doc_id"] for r in rec[q]]
    assert s1.search_many_arrays(qs, 2, filter=[0]) is None   # fewer allowed documents than top_k: records path


def test_stage1_search_many_arrays_filtered_types_match_unfiltered(encoder, tmp_path):
    """The pure dense search returns torch tensors (ids, scores) with and without a filter (with BM25 fusion both
    return numpy arrays)."""
    s1 = _stage1(encoder, tmp_path, enable_bm25=False)
    s1.add_documents(DOCS, META)
    qs = ["neural networks attention", "language models"]
    plain = s1.search_many_arrays(qs, 2)
    filt = s1.search_many_arrays(qs, 2, filter={"tenant": "a"})
    assert all(torch.is_tensor(x) for x in plain) and all(torch.is_tensor(x) for x in filt)
    assert [x.dtype for x in filt] == [x.dtype for x in plain]
    rec = s1.search_many(qs, 2, filter={"tenant": "a"})
    for q in range(2):
        assert filt[0][q].tolist() == [r["doc_id"] for r in rec[q]]


def test_filter_caches_follow_load_index(encoder, tmp_path):
    """A dict filter used before load_index must not serve the previous corpus's bitmaps afterwards."""
    a = _stage1(encoder, tmp_path / "a")
    a.add_documents(DOCS, [{"tenant": "a" if i % 2 == 0 else "b"} for i in range(len(DOCS))])
    assert a.filter_mask({"tenant": "a"}).sum() == (len(DOCS) + 1) // 2
    assert a.search("neural networks attention", 3, filter={"tenant": "a"})
    other = _stage1(encoder, tmp_path / "other")
    other.add_documents(DOCS, [{"tenant": "x"} for _ in DOCS])          # same size, different metadata
    path = str(tmp_path / "other_index.pkl")
    other.save_index(path)
    a.load_index(path)
    assert not a.filter_mask({"tenant": "a"}).any()
    assert a.search("neural networks attention", 3, filter={"tenant": "a"}) == []
    assert len(a.search("neural networks attention", 3, filter={"tenant": "x"})) == 3
    # a larger corpus, and a metadata list replaced by assignment (as the sharded pipeline does)
    big = _stage1(encoder, tmp_path / "big")
    big.add_documents(DOCS + DOCS, [{"tenant": "a" if i >= len(DOCS) else "x"} for i in range(2 * len(DOCS))])
    big.save_index(path)
    a.load_index(path)
    np.testing.assert_array_equal(a.filter_mask({"tenant": "a"}), np.arange(2 * len(DOCS)) >= len(DOCS))
    a.doc_metadata = [{"tenant": "a"}] * len(a.documents)
    assert a.filter_mask({"tenant": "a"}).all()


# ------------------------------------------------------------------ pipeline
def _pipeline(encoder, tmp_path, **cfg):
    pc = PipelineConfig(stage1_model="random:tiny", stage2_model="random:tiny", stage3_model="random:tiny",
                        device="cpu", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
                        log_file=str(tmp_path / "p.log"), stage1_top_k=4, stage2_top_k=3, stage3_top_k=2, **cfg)
    p = RetrievalPipeline(config=pc)
    p.stage1 = Stage1Retriever(Stage1Config(model_name="random:tiny", device="cpu", cache_dir=pc.cache_dir,
                                            index_dir=pc.index_dir, top_k_candidates=pc.stage1_top_k,
                                            enable_bm25=pc.stage1_enable_bm25),
                               model=encoder, index_factory=lambda d: FilteredOracleIndex(d))
    p.stage2 = ColBERTScorer(Stage2Config(model_name="random:tiny", device="cpu", top_k_candidates=pc.stage2_top_k),
                             maxsim_fn=oracle_maxsim)
    p.stage3 = AdaptiveCrossEncoderReranker(Stage3Config(model_name="random:tiny", device="cpu",
                                                         top_k_final=pc.stage3_top_k))
    return p


@pytest.mark.parametrize("bm25", [False, True])
def test_pipeline_filter(encoder, tmp_path, bm25):
    p = _pipeline(encoder, tmp_path, save_intermediate_results=True, stage1_enable_bm25=bm25)
    p.add_documents(DOCS, META)
    r = p.search("neural networks attention", filter={"lang": "de"})
    allowed = {i for i, md in enumerate(META) if md["lang"] == "de"}
    for key in ("results", "stage1_results", "stage2_results"):
        assert {x["doc_id"] for x in r[key]} <= allowed
    assert len(r["stage1_results"]) == min(4, len(allowed))
    assert p.search("neural networks attention", filter={"lang": "xx"})["results"] == []
    single = p.search("language models", filter=[3])
    assert [x["doc_id"] for x in single["results"]] == [3]
    many = p.search_many(["neural networks attention", "language models"], filter=[{"lang": "de"}, {"lang": "xx"}])
    assert {x["doc_id"] for x in many[0]["results"]} <= allowed and many[1]["results"] == []
    seq = p.batch_search(["neural networks attention", "language models"], filter=[{"lang": "de"}, {"lang": "xx"}])
    assert [x["doc_id"] for x in seq[0]["results"]] == [x["doc_id"] for x in many[0]["results"]]
    assert seq[1]["results"] == []


def test_sharded_paths_refuse_filters():
    from tristage_rag_amd.parallel_pipeline import ShardedBM25, ShardedRetrievalPipeline
    from tristage_rag_amd.sharded import ShardedFlatIPIndex
    with pytest.raises(NotImplementedError):
        ShardedFlatIPIndex.search(object.__new__(ShardedFlatIPIndex), np.zeros((1, 4), np.float32), 1,
                                  allowed=np.ones(1, bool))
    with pytest.raises(NotImplementedError):
        ShardedBM25.search(object.__new__(ShardedBM25), "q", 1, allowed=np.ones(1, bool))
    with pytest.raises(NotImplementedError):
        ShardedRetrievalPipeline.search(object.__new__(ShardedRetrievalPipeline), "q", filter={"a": 1})
    with pytest.raises(NotImplementedError):
        ShardedRetrievalPipeline.search_many(object.__new__(ShardedRetrievalPipeline), ["q"], filter={"a": 1})
