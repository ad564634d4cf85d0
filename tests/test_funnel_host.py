"""Funnel search, the parts that need no GPU: signatures and defaults, the argument checks that are
made before anything is launched, the refusals, the numpy model of ``rescore``, and the three places an entry point
has to be listed in."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import funnel_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ts_index_search_prefix", "ts_index_rescore")


def _bare(cls, **attrs):
    ix = cls.__new__(cls)          # no handle: whatever reached the library would fail differently
    for k, v in attrs.items():
        setattr(ix, k, v)
    return ix


def test_signatures_and_config_defaults():
    from tristage_rag_amd import index
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(index.FlatIPIndex.search_prefix)[:5] == ["self", "q", "k", "dims", "allowed"]
    assert inspect.signature(index.FlatIPIndex.search_prefix).parameters["allowed"].default is None
    assert sig(index.FlatIPIndex.rescore) == ["self", "q", "ids", "k"]
    assert inspect.signature(index.FlatIPIndex.rescore).parameters["k"].default is None
    assert sig(index.FlatIPIndex.search_funnel) == ["self", "q", "k", "dims", "fetch_k", "allowed"]
    p = inspect.signature(index.FlatIPIndex.search_funnel).parameters
    assert p["fetch_k"].default is None and p["allowed"].default is None
    assert index.FlatIPIndex.last_funnel_info(_bare(index.FlatIPIndex, _h=None)) == {}
    assert Stage1Config().funnel_dims is None and Stage1Config().funnel_fetch_k is None
    assert PipelineConfig().stage1_funnel_dims is None and PipelineConfig().stage1_funnel_fetch_k is None
    for f in (Stage1Retriever.search, Stage1Retriever.search_many, Stage1Retriever.search_many_arrays,
              RetrievalPipeline.search, RetrievalPipeline.batch_search, RetrievalPipeline.search_many):
        assert inspect.signature(f).parameters["funnel_dims"].default is None, f.__qualname__
    # fetch_k defaults to min(2048, max(8 k, 128)): the filter path of the prefix pass
    assert [index.funnel_default_fetch_k(k) for k in (1, 10, 16, 17, 100, 256, 1000)] == [128, 128, 128, 136, 800, 2048, 2048]


def test_bad_dims_k_and_fetch_k_raise_before_anything_is_launched():
    from tristage_rag_amd import index
    ix = _bare(index.FlatIPIndex, d=768, storage_dtype="f16")
    q = np.zeros((2, 768), dtype=np.float32)
    for dims in (0, 64, 100, 192, 768, 896, -128, 256.5):
        with pytest.raises(ValueError, match="dims"):
            ix.search_prefix(q, 10, dims)
        with pytest.raises(ValueError, match="dims"):
            ix.search_funnel(q, 10, dims)
    for k in (0, -1, 16385):
        with pytest.raises(ValueError, match="k"):
            ix.search_prefix(q, k, 256)
    with pytest.raises(ValueError, match="fetch_k"):
        ix.search_funnel(q, 10, 256, fetch_k=9)                 # fetch_k < k
    with pytest.raises(ValueError, match="fetch_k"):
        ix.search_funnel(q, 10, 256, fetch_k=16385)
    with pytest.raises(ValueError, match="fetch_k"):
        ix.search_funnel(q, 4096, 256)                          # the default shortlist (2048) is below k
    ids = np.zeros((2, 8), dtype=np.int64)
    with pytest.raises(ValueError, match="k="):
        ix.rescore(q, ids, 9)                                   # k > C
    with pytest.raises(ValueError, match="k="):
        ix.rescore(q, ids, 0)
    with pytest.raises(ValueError, match="candidates"):
        ix.rescore(q, np.zeros((2, 16385), dtype=np.int64))
    with pytest.raises(ValueError, match="ids"):
        ix.rescore(q, np.zeros((3, 8), dtype=np.int64))
    with pytest.raises(ValueError, match="queries"):
        ix.rescore(q[:, :100], ids)
    assert index.funnel_check(768, 512, 7) == (7, 512) and index.funnel_check(384, 256, 3, 3) == (3, 256, 3)
    ix._h = None                   # (__del__ then has nothing to close)
    for dt in ("f32", "fp8"):      # storage the prefix scans do not take
        other = _bare(index.FlatIPIndex, d=768, storage_dtype=dt, _h=None)
        for call in (lambda: other.search_prefix(q, 10, 256), lambda: other.rescore(q, ids),
                     lambda: other.search_funnel(q, 10, 256)):
            with pytest.raises(NotImplementedError, match=dt):
                call()


def test_the_library_refuses_bad_arguments_without_a_gpu():
    """TS_ERR_INVALID before any HIP call: a null handle never reaches the device."""
    from tristage_rag_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    assert lib.ts_index_search_prefix(None, buf, 1, _lib.TS_F32, 128, 1, None, 0, 0, None, buf, buf, 0, None) == _lib.TS_ERR_INVALID
    assert "null handle" in _lib.last_error()
    assert lib.ts_index_rescore(None, buf, 1, _lib.TS_F32, buf, 1, 1, buf, buf, None) == _lib.TS_ERR_INVALID
    assert "null handle" in _lib.last_error()


def test_funnel_with_mmr_or_grouping_is_a_value_error():
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    r = _bare(Stage1Retriever, config=Stage1Config(enable_bm25=False), bm25_index=None, faiss_index=None)
    assert r._funnel_args(None) is None
    assert r._funnel_args(256) == (256, None)
    r.config = Stage1Config(enable_bm25=False, funnel_dims=128, funnel_fetch_k=300)     # the config's value is the default
    assert r._funnel_args(None) == (128, 300) and r._funnel_args(256) == (256, 300)
    with pytest.raises(ValueError, match="funnel_dims"):
        r._funnel_args(256, lam=0.5)
    with pytest.raises(ValueError, match="funnel_dims"):
        r._funnel_args(None, grp=("topic", 1))
    r.faiss_index = object()                                                            # an index without the method
    with pytest.raises(NotImplementedError, match="search_funnel"):
        r._funnel_args(256)
    r.index_type_used = "ivf"
    with pytest.raises(NotImplementedError, match="IVF"):
        r._funnel_args(256)
    p = _bare(RetrievalPipeline, config=PipelineConfig())
    assert p._funnel_kwargs(None, None, {}) == {} and p._funnel_kwargs(256, None, {}) == {"funnel_dims": 256}
    with pytest.raises(ValueError, match="funnel_dims"):
        p._funnel_kwargs(256, 0.5, {})
    with pytest.raises(ValueError, match="funnel_dims"):
        p._funnel_kwargs(256, None, {"group_by": "topic", "group_size": 1})
    p.config = PipelineConfig(stage1_funnel_dims=128)
    assert p._funnel_kwargs(None, None, {}) == {"funnel_dims": 128}
    with pytest.raises(ValueError, match="funnel_dims"):
        p._funnel_kwargs(None, 0.5, {})


def test_sharded_and_ivf_classes_refuse(tmp_path):
    from tristage_rag_amd.index import IVFFlatIndex
    from tristage_rag_amd.parallel_pipeline import ShardedRetrievalPipeline
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig
    from tristage_rag_amd.sharded import ShardedFlatIPIndex
    q, ids = np.zeros((1, 256), np.float32), np.zeros((1, 4), np.int64)
    for ix in (_bare(ShardedFlatIPIndex), _bare(IVFFlatIndex, _h=None)):
        with pytest.raises(NotImplementedError, match="funnel"):
            ix.search_prefix(q, 2, 128)
        with pytest.raises(NotImplementedError, match="funnel"):
            ix.rescore(q, ids)
        with pytest.raises(NotImplementedError, match="funnel"):
            ix.search_funnel(q, 2, 128)
    kw = dict(stage1_model="random:tiny", stage2_model="random:tiny", stage3_model="random:tiny", device="cpu",
              cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"), log_file=str(tmp_path / "p.log"))
    p = ShardedRetrievalPipeline(config=PipelineConfig(**kw))
    with pytest.raises(NotImplementedError, match="funnel_dims"):
        p.search("a query", funnel_dims=128)
    with pytest.raises(NotImplementedError, match="funnel_dims"):
        p.search_many(["a query"], funnel_dims=128)
    with pytest.raises(NotImplementedError, match="funnel_dims"):
        p.batch_search(["a query"], funnel_dims=128)
    p2 = ShardedRetrievalPipeline(config=PipelineConfig(stage1_funnel_dims=128, **kw))
    with pytest.raises(NotImplementedError, match="funnel_dims"):
        p2.search("a query")


def test_rescore_model_on_a_hand_made_case():
    """Ties, -1 entries, an out-of-range id, a removed row and duplicates, worked out by hand."""
    S = np.array([[0.5, 2.0, 2.0, -1.0, 2.0, 0.25],
                  [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]], dtype=np.float32)
    ids = np.array([[4, -1, 0, 2, 1, 4, 9, 3],          # 4 twice, a padding entry, 9 is out of range
                    [5, 3, -1, -1, 3, 0, -7, 6]], dtype=np.int64)
    D, I = fm.rescore_model(S, ids)
    assert I[0].tolist() == [1, 2, 4, 4, 0, 3, -1, -1]                     # 2.0 three ways: ids ascending, 4 stays twice
    assert D[0].tolist() == [2.0, 2.0, 2.0, 2.0, 0.5, -1.0, -fm.FLT_MAX, -fm.FLT_MAX]
    assert I[1].tolist() == [0, 3, 3, 5, -1, -1, -1, -1]                   # all scores equal: ids ascending
    assert D[1].tolist() == [1.0] * 4 + [-fm.FLT_MAX] * 4
    D, I = fm.rescore_model(S, ids, k=3)
    assert I.tolist() == [[1, 2, 4], [0, 3, 3]] and D.tolist() == [[2.0, 2.0, 2.0], [1.0, 1.0, 1.0]]
    live = np.array([True, True, False, True, True, True])                 # row 2 removed
    D, I = fm.rescore_model(S, ids, live=live)
    assert I[0].tolist() == [1, 4, 4, 0, 3, -1, -1, -1] and D[0, 3] == 0.5
    D, I = fm.rescore_model(S, ids + np.where(ids >= 0, 100, 0), id_offset=100)   # ids carry the index's offset
    assert I[0].tolist() == [101, 102, 104, 104, 100, 103, -1, -1]
    neg0 = np.array([[-0.0, 0.0, -0.0]], dtype=np.float32)                 # -0 and +0 are one score
    D, I = fm.rescore_model(neg0, np.array([[2, 1, 0]], dtype=np.int64))
    assert I[0].tolist() == [0, 1, 2] and not np.signbit(D).any()


def test_header_binding_and_library_list_both_entries():
    from tristage_rag_amd import _lib
    header = open(os.path.join(ROOT, "include", "tristage.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/tristage.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), f"{name}: header and binding differ in arity"
        assert hasattr(lib, name), f"{name} is not exported by libtristage.so"
    assert len(_lib.SIGNATURES["ts_index_search_prefix"][1]) == 14 and len(_lib.SIGNATURES["ts_index_rescore"][1]) == 10
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in ENTRIES)


def test_the_new_kernels_use_no_scratch():
    """The twelve prefix scans and the two rescore kernels: scratch 0 under -Rpass-analysis=kernel-resource-usage."""
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(ROOT, "tristage-rag_amd", "csrc")
    found = {}
    for src in ("ts_scan_prefix.hip", "ts_rescore.hip"):
        out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                              "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                              "-o", os.devnull], cwd=csrc, capture_output=True, text=True, check=True).stderr
        name = None
        for line in out.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and name and re.search(r"Walk(Strided|Live)Prefix|rescore_kernel", name):
                found[name] = int(m.group(1))
    assert len(found) == 14, found
    assert all(v == 0 for v in found.values()), found
