"""Removal (tombstones), host side (no GPU): the new entry points are declared, bound and exported within ABI
version 4, they check their arguments before touching a device, the new kernels use no scratch (the tombstone
forms of the coalesced scans: tests/test_wide_prefetch_build.py), and the Python surface exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tristage_rag_amd import _lib
from tristage_rag_amd.index import FlatIPIndex, pack_allowed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")
NEW = ("ts_index_remove", "ts_index_live_count", "ts_index_live_words", "ts_index_compact", "ts_remove_ivf")


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "tristage.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", text))


def test_new_symbols_are_declared_bound_and_exported_within_version_4():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_symbols()
    for name in NEW:
        assert name in hdr
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert _lib.header_abi_version() == 4
    assert _lib.load().ts_abi_version() == 4


def test_arguments_are_checked_without_a_gpu():
    lib = _lib.load()
    n = ctypes.c_int64(7)
    ids = (ctypes.c_int64 * 2)(0, 1)
    assert lib.ts_index_remove(None, ids, 2, ctypes.byref(n), None) == _lib.TS_ERR_INVALID
    assert "bad arguments" in _lib.last_error()
    assert lib.ts_index_compact(None, None, None) == _lib.TS_ERR_INVALID
    assert lib.ts_index_live_count(None) == -1
    assert lib.ts_index_live_words(None, None, None) == _lib.TS_ERR_INVALID
    assert lib.ts_remove_ivf(None, ids, 2, ctypes.byref(n), None) == _lib.TS_ERR_INVALID


def test_removal_kernels_use_no_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    found = {}
    for src in ("ts_remove.hip", "ts_ivf.hip"):
        out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                              "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                              "-o", os.devnull], cwd=CSRC, capture_output=True, text=True, check=True).stderr
        name = None
        for line in out.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and name and re.search(r"(live_set|live_clear|and_live|word_count|tile_scan|word_scan|compact_map|"
                                        r"compact_gather|ivf_remove)_kernel", name):
                found[name] = int(m.group(1))
    assert len(found) == 9, found
    assert all(v == 0 for v in found.values()), found


def test_python_surface():
    for attr in ("remove_ids", "nlive", "compact", "live_words", "live_mask"):
        assert hasattr(FlatIPIndex, attr)


def test_live_mask_unpacks_the_live_words():
    """FlatIPIndex.live_mask: the library's live words (the filter-mask layout) -> one bool per row."""
    rng = np.random.default_rng(3)
    for n in (1, 31, 32, 33, 1000):
        live = rng.random(n) < 0.7

        class Words:
            ntotal = n

            def live_words(self):
                return pack_allowed(live, n)

        got = FlatIPIndex.live_mask(Words())
        assert got.dtype == np.bool_ and got.shape == (n,) and (got == live).all()


# ------------------------------------------------------------------ stage 1 / BM25 / token store (CPU doubles)
def _stage1(tmp_path, name="s"):
    from test_filtered_search_host import DOCS, META, FilteredOracleIndex
    from tristage_rag_amd.encoders import SentenceEncoder
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    cfg = Stage1Config(model_name="random:tiny", device="cpu", cache_dir=str(tmp_path / "m"),
                       index_dir=str(tmp_path / name))
    s1 = Stage1Retriever(cfg, model=SentenceEncoder("random:tiny", device="cpu"),
                         index_factory=lambda d: FilteredOracleIndex(d))
    s1.add_documents(DOCS, META)
    return s1


QUERIES = ["machine learning models", "vector search on gpus", "the quick brown fox", "retrieval augmented generation"]


def test_stage1_never_returns_removed_documents(tmp_path):
    s1 = _stage1(tmp_path)
    n = len(s1.documents)
    gone = [0, 2, 3, n - 1]
    df_before = dict(s1.bm25_index.idf)
    assert s1.remove_documents(gone + [2, -1, n + 5]) == len(gone)
    assert s1.remove_documents([2]) == 0 and s1.n_removed == len(gone)
    assert s1.bm25_index.idf == df_before and s1.bm25_index.corpus_size == n   # statistics of everything added
    for fusion in (True, False):
        s1.config.enable_bm25 = fusion
        for res in s1.search_many(QUERIES, top_k=n):
            ids = [r["doc_id"] for r in res]
            assert not set(ids) & set(gone) and len(ids) == n - len(gone)
        res = s1.search(QUERIES[0], top_k=n)
        assert not {r["doc_id"] for r in res} & set(gone)
        got = s1.search_many_arrays(QUERIES, top_k=3)
        if got is not None:
            ids = np.asarray(got[0].cpu() if hasattr(got[0], "cpu") else got[0])
            assert not np.isin(ids, gone).any()
        filt = s1.search_many(QUERIES, top_k=n, filter={"tenant": "a"})
        for res in filt:
            assert all(r["metadata"]["tenant"] == "a" and r["doc_id"] not in gone for r in res)
    s1.config.enable_bm25 = True
    # the BM25 host path alone: removed documents are neither ranked nor used as zero-score padding
    live = s1.live_mask()
    for q in QUERIES:
        bm = s1.bm25_index.search(q, n, allowed=live)
        assert not {i for i, _ in bm} & set(gone) and len(bm) == n - len(gone)


def test_stage1_compact_refits_bm25_and_matches_a_fresh_index(tmp_path):
    from tristage_rag_amd.stage1_retriever import BM25Index
    s1 = _stage1(tmp_path)
    n = len(s1.documents)
    gone = [1, 3]
    s1.remove_documents(gone)
    before = s1.search_many(QUERIES, top_k=n)
    docs_live = [d for i, d in enumerate(s1.documents) if i not in gone]
    old2new = s1.compact()
    assert np.array_equal(old2new[old2new >= 0], np.arange(n - len(gone))) and (old2new[gone] == -1).all()
    assert s1.documents == docs_live and len(s1.doc_metadata) == len(docs_live)
    assert s1.n_removed == 0 and s1.live_mask() is None
    fresh = BM25Index()
    fresh.fit(docs_live)
    for q in QUERIES:
        assert np.array_equal(s1.bm25_index.scores(q), fresh.scores(q))
    s1.config.enable_bm25 = False   # dense only: the pre-compaction lists, renumbered
    s_before = _stage1(tmp_path, "t")
    s_before.config.enable_bm25 = False
    s_before.remove_documents(gone)
    pre = s_before.search_many(QUERIES, top_k=n)
    post = s1.search_many(QUERIES, top_k=n)
    for a, b in zip(pre, post):
        assert [old2new[r["doc_id"]] for r in a] == [r["doc_id"] for r in b]
        assert [r["score"] for r in a] == [r["score"] for r in b]
    assert before   # (the fused lists before compaction were produced)


def test_manifest_round_trip_keeps_tombstones(tmp_path):
    import json
    s1 = _stage1(tmp_path)
    s1.remove_documents([3, 6])
    path = str(tmp_path / "idx" / "stage1.json")
    s1.save_index(path)
    man = json.load(open(path))
    assert man["removed"].endswith(".removed.npy")
    s2 = _stage1(tmp_path, "u")
    s2.load_index(path)
    assert np.array_equal(s2.live_mask(), s1.live_mask())
    assert [r["doc_id"] for r in s2.search(QUERIES[0], top_k=50)] == [r["doc_id"] for r in s1.search(QUERIES[0], top_k=50)]
    del man["removed"]   # an older manifest: every document live
    json.dump(man, open(path, "w"))
    s3 = _stage1(tmp_path, "v")
    s3.load_index(path)
    assert s3.live_mask() is None and s3.n_removed == 0


@pytest.mark.parametrize("dt", ["bf16", "fp8"])
def test_token_store_compact_in_place(dt):
    import torch
    from tristage_rag_amd.stage2_rescorer import TokenStore, _as_bytes
    rng = np.random.default_rng(1)
    lens = rng.integers(1, 40, size=60).tolist()
    mats = [torch.from_numpy(rng.standard_normal((L, 32)).astype(np.float32)).to(torch.bfloat16) for L in lens]
    if dt == "fp8":
        mats = [m.float().to(torch.float8_e4m3fn) for m in mats]
    st = TokenStore()
    st.append(mats[:30])
    st.append(mats[30:])
    keep = rng.random(60) < 0.6
    keep[0] = False
    old_data = st.data
    TokenStore.COMPACT_CHUNK_BYTES = 32 * 2 * 7   # many chunks of 7 rows (bf16 rows; more for fp8)
    try:
        st.compact(keep)
    finally:
        TokenStore.COMPACT_CHUNK_BYTES = 64 << 20
    assert st.data is old_data   # in place
    ref = TokenStore()
    ref.append([m for m, k in zip(mats, keep) if k])
    assert st.starts == ref.starts and st.lens == ref.lens and st.rows == ref.rows
    assert torch.equal(_as_bytes(st.data[: st.rows]), _as_bytes(ref.data[: ref.rows]))
