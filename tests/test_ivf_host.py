"""CPU checks of the IVF-Flat boundary: the ts_ivf_* entry points are declared, bound and exported, reject bad
arguments before any HIP call, and the retriever's index_type plumbing (default, the 1000-row rule, manifest)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tristage_rag_amd import _lib
from tristage_rag_amd.encoders import SentenceEncoder
from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever

from doubles import OracleIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IVF_SYMBOLS = ("ts_ivf_create", "ts_ivf_destroy", "ts_ivf_reset", "ts_ivf_train", "ts_ivf_set_centroids",
               "ts_ivf_get_centroids", "ts_ivf_is_trained", "ts_ivf_add", "ts_ivf_search", "ts_ivf_probe",
               "ts_ivf_list_sizes", "ts_ivf_reconstruct", "ts_ivf_ntotal", "ts_ivf_set_id_offset",
               "ts_ivf_last_search_info")


def test_ivf_symbols_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tristage.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ts_ivf_[a-z0-9_]+)\s*\(", text))
    assert declared == set(IVF_SYMBOLS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in IVF_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _lib.header_abi_version() == 4


def test_ivf_argument_errors_without_a_gpu():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.ts_ivf_create(64, 16, _lib.TS_F16, 0, None) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_create(64, 16, _lib.TS_F32, 0, ctypes.byref(h)) == _lib.TS_ERR_INVALID   # f16 / bf16 only
    assert "f16 or bf16" in _lib.last_error()
    assert lib.ts_ivf_create(0, 16, _lib.TS_F16, 0, ctypes.byref(h)) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_create(64, 0, _lib.TS_F16, 0, ctypes.byref(h)) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_create(64, 16385, _lib.TS_BF16, 0, ctypes.byref(h)) == _lib.TS_ERR_INVALID
    assert "nlist" in _lib.last_error()
    assert not h.value
    assert lib.ts_ivf_destroy(None) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_reset(None) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_ntotal(None) == -1
    assert lib.ts_ivf_is_trained(None) == -1
    assert lib.ts_ivf_set_id_offset(None, 5) == _lib.TS_ERR_INVALID
    buf = (ctypes.c_int64 * 16)()
    assert lib.ts_ivf_list_sizes(None, buf) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_last_search_info(None, buf) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_train(None, None, 10, _lib.TS_F16, 0, 25, None, None) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_add(None, None, 10, _lib.TS_F16, 0, None) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_search(None, None, 1, _lib.TS_F16, 10, 1, None, None, None) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_probe(None, None, 1, _lib.TS_F16, 1, None, None, None) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_reconstruct(None, 0, 1, None, None) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_set_centroids(None, None, None) == _lib.TS_ERR_INVALID
    assert lib.ts_ivf_get_centroids(None, None, None) == _lib.TS_ERR_INVALID


@pytest.fixture(scope="module")
def encoder():
    return SentenceEncoder("random:tiny", device="cpu")


def _stage1(encoder, tmp_path, **kw):
    cfg = Stage1Config(model_name="random:tiny", device="cpu", cache_dir=str(tmp_path / "m"),
                       index_dir=str(tmp_path / "i"), enable_bm25=False, **kw)
    return Stage1Retriever(cfg, model=encoder, index_factory=lambda d: OracleIndex(d))


def test_stage1_config_defaults_to_flat():
    c = Stage1Config()
    assert c.index_type == "flat" and c.nlist == 100 and c.nprobe == 10


def test_index_kind_follows_the_reference_rule(encoder, tmp_path):
    s = _stage1(encoder, tmp_path)
    assert s._index_kind(5000) == "flat"
    s.config.index_type = "auto"
    assert s._index_kind(1000) == "flat" and s._index_kind(1001) == "ivf"
    s.config.index_type = "ivf"
    assert s._index_kind(3) == "ivf"
    s.config.index_type = "hnsw"
    with pytest.raises(ValueError):
        s._index_kind(10)


def test_manifest_round_trip_of_the_index_type(encoder, tmp_path):
    docs = ["alpha beta", "gamma delta", "epsilon zeta", "eta theta"]
    a = _stage1(encoder, tmp_path)
    a.add_documents(docs)
    path = str(tmp_path / "i" / "stage1_index.pkl")
    a.save_index(path)
    man = json.load(open(path))
    assert man["index_type"] == "flat" and man["centroids"] is None
    assert man["config"]["index_type"] == "flat"
    b = _stage1(encoder, tmp_path)
    b.load_index(path)
    assert b.index_type_used == "flat" and b.get_stats()["index_type"] == "flat"
    assert np.array_equal(b.faiss_index.reconstruct_n(), a.faiss_index.reconstruct_n())
    # an IVF retriever refuses filters instead of ignoring them
    b.index_type_used = "ivf"
    with pytest.raises(NotImplementedError):
        b.search("alpha", top_k=2, filter={"x": 1})
