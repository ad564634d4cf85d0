"""Update in place, host side (no GPU): the two entry points are declared, bound and exported within ABI version 4 and
check their arguments before touching a device, the new kernels use no scratch, and the Python layers (stage 1 with
BM25, the token store, the token-id cache, the pipeline on its CPU doubles) keep their books."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tristage_rag_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")
NEW = ("ts_index_update", "ts_update_ivf")
STAGES = (("stage1_results", "stage1_score"), ("stage2_results", "stage2_score"), ("results", "stage3_score"))
PQ = ["neural networks attention", "language retrieval system", "gpu memory index", "token embedding search"]


def assert_close_results(a, b):
    """The criterion of test_pipeline_gpu_matches_cpu_doubles for two pipelines that encoded the same texts in
    different batches: scores within 1e-3, and a position may differ only where the two scores differ by < 1e-4."""
    for stage, key in STAGES:
        ia, ib = [r["doc_id"] for r in a[stage]], [r["doc_id"] for r in b[stage]]
        sa, sb = np.array([r[key] for r in a[stage]]), np.array([r[key] for r in b[stage]])
        assert len(ia) == len(ib), stage
        np.testing.assert_allclose(sa, sb, atol=1e-3)
        if ia != ib:
            assert sorted(ia) == sorted(ib) or np.abs(sa - sb).max() < 1e-4, stage
            for x, y, u, v in zip(ia, ib, sa, sb):
                assert x == y or abs(u - v) < 1e-4, stage


def updated_texts(docs, ids, tag="zzupdated"):
    """New texts for the documents `ids`: every one carries a token no other document has, the first is much longer
    than what it replaces and the second much shorter."""
    out = []
    for j, i in enumerate(ids):
        words = docs[(i * 7 + 3) % len(docs)].split()
        if j == 0:
            words = words + docs[(i + 1) % len(docs)].split() + docs[(i + 2) % len(docs)].split() + ["memory"] * 30
        elif j == 1:
            words = words[:2]
        out.append(" ".join([f"{tag}{i}"] + words))
    return out


# ------------------------------------------------------------------ the C boundary
def _header_symbols():
    text = open(os.path.join(ROOT, "include", "tristage.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", text))


def test_update_symbols_are_declared_bound_and_exported_within_version_4():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_symbols()
    for name in NEW:
        assert name in hdr
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
        assert not name.startswith("ts_ivf_")
    assert _lib.header_abi_version() == 4
    assert _lib.load().ts_abi_version() == 4


def test_update_arguments_are_checked_without_a_gpu():
    lib = _lib.load()
    ids = (ctypes.c_int64 * 2)(0, 1)
    p = ctypes.c_void_p(4096)   # never dereferenced: the calls fail first
    for fn in (lib.ts_index_update, lib.ts_update_ivf):
        assert fn(None, ids, 2, p, _lib.TS_F16, 0, None) == _lib.TS_ERR_INVALID
        assert "bad arguments" in _lib.last_error()
        assert fn(None, ids, -1, p, _lib.TS_F16, 0, None) == _lib.TS_ERR_INVALID
        assert fn(None, None, 0, None, _lib.TS_F16, 0, None) == _lib.TS_ERR_INVALID
    # a handle is not needed to see that the other arguments are refused first
    h = ctypes.c_void_p(4096)
    for fn in (lib.ts_index_update, lib.ts_update_ivf):
        assert fn(h, ids, -3, p, _lib.TS_F16, 0, None) == _lib.TS_ERR_INVALID      # bad count
        assert fn(h, None, 2, p, _lib.TS_F16, 0, None) == _lib.TS_ERR_INVALID      # no ids
        assert fn(h, ids, 2, None, _lib.TS_F16, 0, None) == _lib.TS_ERR_INVALID    # no rows
        assert fn(h, ids, 2, p, 9, 0, None) == _lib.TS_ERR_INVALID                 # bad dtype
    assert lib.ts_update_ivf(h, ids, 2, p, _lib.TS_F16, _lib.TS_FLAG_HOST_PTR, None) == _lib.TS_ERR_INVALID   # device rows only


def test_update_kernels_use_no_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                          "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "-c", "ts_update.hip",
                          "-o", os.devnull], cwd=CSRC, capture_output=True, text=True, check=True).stderr
    found, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and re.search(r"upd_\w+_kernel", name):
            found[name] = int(m.group(1))
    assert len(found) == 5, found   # live check, whole blocks, single rows, IVF check, IVF placement
    assert all(v == 0 for v in found.values()), found
    # and none of them is counted among the removal kernels (tests/test_remove_host.py fixes that set)
    removal = r"(live_set|live_clear|and_live|word_count|tile_scan|word_scan|compact_map|compact_gather|ivf_remove)_kernel"
    assert not [n for n in found if re.search(removal, n)]


def test_new_source_is_listed_and_python_surface_exists():
    from tristage_rag_amd.index import FlatIPIndex, IVFFlatIndex
    from tristage_rag_amd.retrieval_pipeline import RetrievalPipeline
    from tristage_rag_amd.stage1_retriever import Stage1Retriever
    from tristage_rag_amd.stage2_rescorer import ColBERTScorer
    from tristage_rag_amd.stage3_reranker import CrossEncoderReranker
    assert "ts_update.hip" in open(os.path.join(CSRC, "Makefile")).read()
    for cls in (FlatIPIndex, IVFFlatIndex):
        assert hasattr(cls, "update_rows")
    for cls in (RetrievalPipeline, Stage1Retriever, ColBERTScorer, CrossEncoderReranker):
        assert hasattr(cls, "update_documents")


def test_sharded_pipeline_refuses_updates():
    from tristage_rag_amd.parallel_pipeline import ShardedRetrievalPipeline
    p = ShardedRetrievalPipeline.__new__(ShardedRetrievalPipeline)
    with pytest.raises(NotImplementedError):
        p.update_documents([0], ["text"])


# ------------------------------------------------------------------ stage 1 / BM25 (CPU doubles)
def _stage1(tmp_path, name="s"):
    from test_remove_host import _stage1 as make
    return make(tmp_path, name)


def test_stage1_update_refits_bm25_and_replaces_texts_and_metadata(tmp_path):
    from test_filtered_search_host import DOCS, META
    from tristage_rag_amd.stage1_retriever import BM25Index
    s1 = _stage1(tmp_path)
    n = len(DOCS)
    ids = [1, n - 1, 2]
    new = updated_texts(DOCS, ids)
    meta = [dict(META[i], tenant="zz") for i in ids]
    before = s1.faiss_index.reconstruct_n(0, n).copy()
    assert s1.filter_mask({"tenant": "zz"}).sum() == 0   # (builds the cache that has to start over)
    assert s1.update_documents(ids, new, meta) == 3
    final = list(DOCS)
    for i, t in zip(ids, new):
        final[i] = t
    assert s1.documents == final and len(s1.doc_metadata) == n
    assert np.flatnonzero(s1.filter_mask({"tenant": "zz"})).tolist() == sorted(ids)
    fresh = BM25Index()
    fresh.fit(final)
    for q in ["machine learning models", "zzupdated1", new[1]]:
        assert np.array_equal(s1.bm25_index.scores(q), fresh.scores(q))
    # the rebuild fallback (the double has no update_rows): other rows as they were, updated rows changed
    after = s1.faiss_index.reconstruct_n(0, n)
    keep = np.ones(n, bool)
    keep[ids] = False
    assert np.array_equal(after[keep], before[keep]) and not np.array_equal(after[ids], before[ids])
    s1.config.enable_bm25 = False
    for i, t in zip(ids, new):
        top = s1.search(t, top_k=3)[0]
        assert top["doc_id"] == i and abs(top["score"] - 1.0) < 1e-3 and top["document"] == t
    assert s1.update_documents([], []) == 0


def test_stage1_update_under_bm25_refit_compat_scores_the_new_text(tmp_path):
    """BM25Index(refit_compat=True).fit() appends to the entries of earlier fits, so a refit in place would keep
    scoring document i with the old text's term frequencies: update_documents fits a fresh index, as compact() does."""
    from test_filtered_search_host import DOCS
    from tristage_rag_amd.stage1_retriever import BM25Index
    s1 = _stage1(tmp_path)
    s1.bm25_index.close()
    s1.bm25_index = BM25Index(refit_compat=True)
    s1.bm25_index.fit(s1.documents)
    assert s1.update_documents([1], ["zzupdated1 entirely new words"]) == 1
    final = list(DOCS)
    final[1] = "zzupdated1 entirely new words"
    fresh = BM25Index(refit_compat=True)
    fresh.fit(final)
    assert s1.bm25_index.refit_compat and s1.bm25_index.corpus_size == len(final)
    for q in ["zzupdated1", "machine learning models", DOCS[1]]:
        assert np.array_equal(s1.bm25_index.scores(q), fresh.scores(q))
    assert s1.bm25_index.search("zzupdated1", 1)[0][0] == 1


def test_stage1_update_is_all_or_nothing(tmp_path):
    from test_filtered_search_host import DOCS
    s1 = _stage1(tmp_path)
    n = len(DOCS)
    s1.remove_documents([2])
    docs, rows = list(s1.documents), s1.faiss_index.reconstruct_n(0, n).copy()
    for bad in ([0, 2], [0, n], [0, -1], [0, 3, 0]):
        with pytest.raises(ValueError) as e:
            s1.update_documents(bad, ["new text"] * len(bad))
        assert str(bad[-1]) in str(e.value)
    with pytest.raises(ValueError):
        s1.update_documents([0, 1], ["one text"])
    with pytest.raises(ValueError):
        s1.update_documents([0], ["one text"], [{}, {}])
    assert s1.documents == docs and np.array_equal(s1.faiss_index.reconstruct_n(0, n), rows)
    # a live document next to a removed one is updated, and the removed one stays removed
    assert s1.update_documents([3], ["zzonly new words"]) == 1
    assert s1.n_removed == 1
    got = [r["doc_id"] for r in s1.search("zzonly new words", top_k=n)]
    assert got[0] == 3 and 2 not in got


# ------------------------------------------------------------------ token store and slots (CPU tensors)
@pytest.mark.parametrize("dt", ["bf16", "fp8"])
def test_token_store_overwrite_append_and_compact(dt):
    import torch
    from tristage_rag_amd.stage2_rescorer import ColBERTScorer, TokenStore, _as_bytes
    rng = np.random.default_rng(2)

    def mat(L):
        m = torch.from_numpy(rng.standard_normal((L, 32)).astype(np.float32)).to(torch.bfloat16)
        return m.float().to(torch.float8_e4m3fn) if dt == "fp8" else m

    lens = [5, 9, 3, 12, 7, 4]
    mats = [mat(L) for L in lens]
    sc = ColBERTScorer.__new__(ColBERTScorer)   # the bookkeeping alone: no model
    sc.token_store, sc._store_slot, sc._slot_version, sc._doc_cache = TokenStore(), {}, 0, {}
    sc.token_store.append(mats)
    sc._store_slot = {10 + i: i for i in range(6)}   # doc ids 10..15
    new = {11: mat(9), 12: mat(2), 13: mat(20), 15: mat(5)}   # same length, shrunk, grown, grown

    def batches(documents):   # what _store_batches yields, from ready-made matrices
        yield list(range(len(documents))), torch.cat([_as_bytes(m) for m in documents]).view(mats[0].dtype), \
            [int(m.shape[0]) for m in documents]
    sc._store_batches = batches
    v0 = sc._slot_version
    sc.update_documents(list(new), list(new.values()))
    st = sc.token_store
    assert sc._slot_version > v0
    assert sc._store_slot[11] == 1 and sc._store_slot[12] == 2          # in place
    assert st.lens[1] == 9 and st.lens[2] == 2 and st.starts[2] == 14   # shortened where it was
    assert sc._store_slot[13] == 6 and sc._store_slot[15] == 7          # appended and repointed
    assert len(st) == 8 and st.rows == sum(lens) + 20 + 5
    final = {10 + i: m for i, m in enumerate(mats)}
    final.update(new)

    def rows_of(d):
        s = sc._store_slot[d]
        return _as_bytes(st.data[st.starts[s]: st.starts[s] + st.lens[s]])
    for d, m in final.items():
        assert torch.equal(rows_of(d), _as_bytes(m)), d
    # compaction reclaims the tails and the abandoned slots; doc 14 is removed on the way
    old2new = np.full(16, -1, dtype=np.int64)
    old2new[[10, 11, 12, 13, 15]] = np.arange(5)
    sc.compact_documents(old2new)
    st = sc.token_store
    live = [10, 11, 12, 13, 15]
    assert st.rows == sum(int(final[d].shape[0]) for d in live) and len(st) == 5
    assert sorted(sc._store_slot) == [0, 1, 2, 3, 4] and sorted(sc._store_slot.values()) == [0, 1, 2, 3, 4]
    for d in live:
        assert torch.equal(rows_of(int(old2new[d])), _as_bytes(final[d])), d
    # shortened documents alone (nothing dropped) are packed too
    st.overwrite(sc._store_slot[0], final[10][:2])
    rows_before = st.rows
    sc.compact_documents(np.arange(5))
    assert sc.token_store.rows == rows_before - (int(final[10].shape[0]) - 2)
    with pytest.raises(ValueError):
        st.overwrite(0, mat(50))


def test_pair_assembler_replaces_token_ids():
    from tristage_rag_amd.encoders import HashTokenizer, PairAssembler
    tok = HashTokenizer()
    pa = PairAssembler(tok, 64)
    if not pa.ok:
        pytest.fail(f"the hash tokenizer is not restated: {pa.why}")
    texts = ["alpha bravo charlie", "delta echo", "foxtrot golf hotel india"]
    pa.add_documents(texts)
    pa.table("cpu")
    pa.replace_documents([1, 2], ["one two three four five", "six"])
    assert pa._table is None and len(pa) == 3
    ref = PairAssembler(tok, 64)
    ref.add_documents([texts[0], "one two three four five", "six"])
    assert pa._doc_ids == ref._doc_ids and pa._doc_len == ref._doc_len


# ------------------------------------------------------------------ the pipeline on its CPU doubles
@pytest.mark.parametrize("bm25", [False, True])
def test_cpu_doubles_pipeline_equals_a_rebuilt_pipeline(tmp_path, bm25):
    from test_pipeline_gpu import _build, _corpus
    docs = _corpus(150)
    ids = [3, 40, 77, len(docs) - 1]
    new = updated_texts(docs, ids)
    p = _build("cpu", tmp_path, doubles=True, stage1_enable_bm25=bm25)
    p.add_documents(docs)
    info = p.get_pipeline_info()["documents"]
    assert p.update_documents(ids, new) == len(ids)
    assert p.get_pipeline_info()["documents"] == info
    final = list(docs)
    for i, t in zip(ids, new):
        final[i] = t
    ref = _build("cpu", tmp_path, doubles=True, stage1_enable_bm25=bm25)
    ref.add_documents(final)
    queries = PQ + [new[0], new[2]]
    for q in queries:
        assert_close_results(p.search(q), ref.search(q))
    for a, b in zip(p.search_many(queries), ref.search_many(queries)):
        assert_close_results(a, b)
    if not bm25:
        for i, t, old in zip(ids, new, [docs[i] for i in ids]):
            top = p.search(t)["stage1_results"][0]
            assert top["doc_id"] == i and abs(top["stage1_score"] - 1.0) < 1e-3
            assert not [r for r in p.search(old)["stage1_results"]
                        if r["doc_id"] == i and abs(r["stage1_score"] - 1.0) < 1e-3]
    with pytest.raises(ValueError):
        p.update_documents([0, 0], ["a", "b"])
    with pytest.raises(ValueError):
        p.update_documents([len(docs)], ["a"])
