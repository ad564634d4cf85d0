"""Boosted search, the parts that need no GPU: the three places an entry point has to be listed in,
the argument checks made before anything is launched, signatures and defaults, the boost formulae against a written-out
float64 model, the option conflicts and refusals, and the retriever's bias cache over a host double of the index."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import bias_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ts_index_search_biased", "ts_index_last_bias_info")


def _bare(cls, **attrs):
    ix = cls.__new__(cls)          # no handle: whatever reached the library would fail differently
    for k, v in attrs.items():
        setattr(ix, k, v)
    return ix


# ------------------------------------------------------------------------------------------------------- the ABI
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
        assert not name.startswith("ts_ivf_")
    assert len(_lib.SIGNATURES["ts_index_search_biased"][1]) == 15 and len(_lib.SIGNATURES["ts_index_last_bias_info"][1]) == 2
    assert _lib.header_abi_version() == 4 and _lib.load().ts_abi_version() == 4
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in ENTRIES)


def test_the_library_refuses_bad_arguments_without_a_gpu():
    """TS_ERR_INVALID before any HIP call.  The checks that need no handle come first, so each is reached with a null
    handle; a call whose other arguments are fine then fails on the handle itself."""
    from tristage_rag_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    moq = (ctypes.c_int32 * 1)(0)
    F32, HOST, NOF = _lib.TS_F32, _lib.TS_FLAG_HOST_PTR, _lib.TS_FLAG_NO_FILTER

    def call(queries=buf, nq=1, q_dtype=F32, k=1, bias=buf, bias_rows=64, bits=None, words=0, n_masks=0, moq=None,
             out_s=buf, out_i=buf, flags=0):
        return lib.ts_index_search_biased(None, queries, nq, q_dtype, k, bias, bias_rows, bits, words, n_masks, moq,
                                          out_s, out_i, flags, None)

    for kw, word in (({"flags": _lib.TS_FLAG_ASYNC}, "flags"), ({"flags": HOST | 0x4000}, "flags"),
                     ({"k": 0}, "k ="), ({"k": 16385}, "k ="), ({"nq": -1}, "nq ="), ({"q_dtype": 99}, "dtype"),
                     ({"bias": None}, "null"), ({"queries": None}, "null"), ({"out_s": None}, "null"),
                     ({"out_i": None}, "null"), ({"n_masks": -1}, "n_masks"), ({"n_masks": 1, "words": -1}, "n_masks"),
                     ({"n_masks": 1, "words": 2, "bits": None}, "allow_bits"),
                     ({"n_masks": 1, "words": 2, "bits": buf, "moq": (ctypes.c_int32 * 1)(1)}, "mask_of_query"),
                     ({"n_masks": 1, "words": 2, "bits": buf, "moq": (ctypes.c_int32 * 1)(-2)}, "mask_of_query")):
        assert call(**kw) == _lib.TS_ERR_INVALID, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    for flags in (0, HOST, NOF, HOST | NOF):                      # the two accepted flags get as far as the handle
        assert call(flags=flags, n_masks=1, words=2, bits=buf, moq=moq) == _lib.TS_ERR_INVALID
        assert "null handle" in _lib.last_error()
    info = (ctypes.c_int64 * 4)()
    assert lib.ts_index_last_bias_info(None, info) == _lib.TS_ERR_INVALID
    assert lib.ts_index_last_bias_info(None, None) == _lib.TS_ERR_INVALID


def test_the_new_kernels_use_no_scratch():
    """The four biased scans, the threshold kernel and the dense path's kernel: scratch 0 under
    -Rpass-analysis=kernel-resource-usage, and the scans fit the 256 VGPRs of their occupancy (DESIGN.md 4.22 records
    164 / 210)."""
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(ROOT, "tristage-rag_amd", "csrc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "ts_scan_bias.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True, check=True).stderr
    scratch, vgprs, name = {}, {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r" VGPRs: (\d+)", line)
        if m and name:
            vgprs[name] = int(m.group(1))
    scans = [n for n in scratch if "WalkLiveBias" in n]
    assert len(scans) == 4 and len(scratch) == 6, scratch
    assert all(v == 0 for v in scratch.values()), scratch
    assert all(vgprs[n] <= 256 for n in scans), vgprs                 # two waves per SIMD, as the masked scans run


# --------------------------------------------------------------------------------------- signatures and defaults
def test_signatures_and_config_defaults():
    from tristage_rag_amd import index
    from tristage_rag_amd.parallel_pipeline import ShardedRetrievalPipeline
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    from tristage_rag_amd.sharded import ShardedFlatIPIndex
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    want = ["self", "q", "k", "bias", "allowed", "exact_dense", "check_finite"]
    for cls in (index.FlatIPIndex, index.IVFFlatIndex, ShardedFlatIPIndex):
        p = inspect.signature(cls.search_biased).parameters
        assert list(p) == want, cls.__name__
        assert p["allowed"].default is None and p["exact_dense"].default is False and p["check_finite"].default is True
    assert Stage1Config().boost is None and PipelineConfig().stage1_boost is None
    for f in (Stage1Retriever.search, Stage1Retriever.search_many, Stage1Retriever.search_many_arrays,
              RetrievalPipeline.search, RetrievalPipeline.batch_search, RetrievalPipeline.search_many,
              ShardedRetrievalPipeline.search, ShardedRetrievalPipeline.batch_search, ShardedRetrievalPipeline.search_many):
        assert inspect.signature(f).parameters["boost"].default is None, f.__qualname__
    assert hasattr(index.FlatIPIndex, "last_bias_info")


def test_bad_k_bias_and_storage_raise_before_anything_is_launched():
    from tristage_rag_amd import index
    ix = _bare(index.FlatIPIndex, d=8, storage_dtype="f16")
    q = np.zeros((2, 8), dtype=np.float32)
    for k in (0, -1, 16385):
        with pytest.raises(ValueError, match="k="):
            ix.search_biased(q, k, np.zeros(4, np.float32))
    assert index.bias_check_k(16384) == 16384 and index.bias_check_k(1) == 1
    for bad in (np.zeros(5, np.float32), np.zeros((4, 1), np.float32), np.zeros(3, np.float32)):
        with pytest.raises(ValueError, match="one entry per row"):
            index._marshal_bias(bad, 4, None, True)
    for v in (np.nan, np.inf, -np.inf):
        b = np.zeros(4, np.float32)
        b[2] = v
        with pytest.raises(ValueError, match="finite"):
            index._marshal_bias(b, 4, None, True)
        with pytest.raises(ValueError, match="CUDA tensors only"):              # a host bias is always checked
            index._marshal_bias(b, 4, None, False)
    got = index._marshal_bias(np.arange(4, dtype=np.float64)[::-1], 4, None, True)
    assert got.dtype == np.float32 and got.flags.c_contiguous and got.tolist() == [3.0, 2.0, 1.0, 0.0]
    ix._h = None                   # (__del__ then has nothing to close)
    for dt in ("f32", "fp8"):      # storage the biased scan does not take: the message names it
        other = _bare(index.FlatIPIndex, d=8, storage_dtype=dt, _h=None)
        with pytest.raises(NotImplementedError, match=dt):
            other.search_biased(q, 1, np.zeros(4, np.float32))


# ------------------------------------------------------------------------------------------------- boost formulae
META = [{"ts": 100.0, "pop": 3}, {"ts": 90.0}, {"pop": 7, "ts": None}, {"ts": 130.0, "pop": 0.5}, {}, {"ts": 100.5, "pop": -2}]


def _ulp_equal(a, b):
    """Equal to within one float32 ulp: the model and the product may spell a float64 formula differently (exp(x * ln v
    / s) against exp(ln v / s * x)), which moves the float64 value by parts in 10^16 and the rounded float32 by at most
    one place, and only where the value sits on a rounding boundary."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all((a == b) | (np.nextafter(a, b) == b)))


def test_field_and_decay_specs_follow_the_float64_model():
    from tristage_rag_amd import boost
    spec = {"field": "pop", "weight": 0.125, "missing": -1.5}
    got = boost.bias_array(spec, META)
    assert got.dtype == np.float32 and got.tolist() == [0.375, -1.5, 0.875, 0.0625, -1.5, -0.25]     # exact in binary
    assert np.array_equal(got, bm.spec_bias64(spec, META))
    assert boost.bias_array({"field": "pop"}, META).tolist() == [3.0, 0.0, 7.0, 0.5, 0.0, -2.0]       # weight 1, missing 0
    for kind in boost.DECAYS:
        for offset in (0.0, 5.0):
            spec = {"field": "ts", "decay": kind, "origin": 100.0, "scale": 10.0, "offset": offset, "decay_value": 0.25,
                    "weight": 0.3, "missing": 0.01}
            got = boost.bias_array(spec, META)
            assert _ulp_equal(got, bm.spec_bias64(spec, META)), (kind, offset, got)
            assert got[0] == np.float32(0.3)                                   # at the origin: the weight
            assert got[2] == got[4] == np.float32(0.01)                        # None and absent: `missing`, as it is
            if offset:
                assert got[5] == np.float32(0.3)                               # inside the offset: still the weight
            else:
                assert got[1] == np.float32(0.3 * 0.25)                        # |x - o| = scale: weight * decay_value
        # |x - o| - offset = scale, on either side of the origin
        spec = {"field": "ts", "decay": kind, "origin": 100.0, "scale": 25.0, "offset": 5.0, "weight": 2.0}
        got = boost.bias_array(spec, [{"ts": 130.0}, {"ts": 70.0}])
        assert got.tolist() == [1.0, 1.0], kind                               # decay_value defaults to 0.5
    # linear reaches zero at scale / (1 - decay_value) and stays there; exp and gauss never do
    far = [{"ts": 110.0}, {"ts": 1000.0}]                                      # 7.5 / (1 - 0.25) = 10, exact in binary
    assert boost.bias_array({"field": "ts", "decay": "linear", "origin": 100.0, "scale": 7.5, "decay_value": 0.25}, far).tolist() == [0.0, 0.0]
    assert bm.decay64("gauss", 20.0, 10.0, 0.5) == pytest.approx(0.5 ** 4, rel=1e-15)
    assert bm.decay64("exp", 20.0, 10.0, 0.5) == pytest.approx(0.5 ** 2, rel=1e-15)


def test_array_and_callable_specs_and_the_refusals():
    from tristage_rag_amd import boost
    arr = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    got = boost.bias_array(arr, META)
    assert got.dtype == np.float32 and np.array_equal(got, arr.astype(np.float32))
    fn = lambda m: 2.0 * len(m)
    assert boost.bias_array(fn, META).tolist() == [4.0, 2.0, 4.0, 4.0, 0.0, 4.0]
    with pytest.raises(ValueError, match="one entry per document"):
        boost.bias_array(arr[:5], META)
    for bad in ({"weight": 1.0}, {"field": "ts", "decay": "cubic", "origin": 0, "scale": 1},
                {"field": "ts", "decay": "exp", "origin": 0}, {"field": "ts", "decay": "exp", "origin": 0, "scale": 0.0},
                {"field": "ts", "decay": "exp", "origin": 0, "scale": 1, "decay_value": 1.0},
                {"field": "ts", "decay": "exp", "origin": 0, "scale": 1, "offset": -1.0},
                {"field": "ts", "wieght": 2.0}, {"field": "ts", "origin": 3.0}, {"field": "ts", "weight": float("inf")}):
        with pytest.raises(ValueError):
            boost.check_spec(bad)
    with pytest.raises(TypeError):
        boost.check_spec("ts")
    with pytest.raises(ValueError, match="finite"):
        boost.bias_array({"field": "ts", "weight": 1e38}, [{"ts": 100.0}])       # overflows float32
    with pytest.raises(ValueError, match="finite"):
        boost.bias_array(lambda m: float("nan"), [{}])
    # a dict is one spec by value, an array or a callable by identity
    assert boost.spec_key({"field": "a", "weight": 1.0})[0] == boost.spec_key({"weight": 1.0, "field": "a"})[0]
    assert boost.spec_key({"field": "a", "weight": 1.0})[0] != boost.spec_key({"field": "a", "weight": 2.0})[0]
    assert boost.spec_key(arr)[0] == boost.spec_key(arr)[0] != boost.spec_key(arr.copy())[0] and boost.spec_key(arr)[1] is arr


# ------------------------------------------------------------------------------------------ conflicts and refusals
def test_boost_with_mmr_grouping_or_funnel_is_a_value_error():
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    spec = {"field": "pop", "weight": 0.1}
    r = _bare(Stage1Retriever, config=Stage1Config(enable_bm25=False), bm25_index=None, faiss_index=None)
    assert r._boost_args(None) is None
    assert r._boost_args(spec) is spec
    r.config = Stage1Config(enable_bm25=False, boost=spec)                   # the config's value is the default
    assert r._boost_args(None) is spec
    arr = np.zeros(3, np.float32)
    assert r._boost_args(arr) is arr                                     # the argument wins
    for kw in ({"lam": 0.5}, {"grp": ("topic", 1)}, {"fun": (256, None)}):
        with pytest.raises(ValueError, match="boost"):
            r._boost_args(spec, **kw)
    with pytest.raises(ValueError):
        r._boost_args({"field": "pop", "decay": "cubic", "origin": 0, "scale": 1})
    r.faiss_index = object()                                                  # an index without the method
    with pytest.raises(NotImplementedError, match="search_biased"):
        r._boost_args(spec)
    for dt in ("f32", "fp8"):
        r.faiss_index = type("Ix", (), {"search_biased": None, "storage_dtype": dt})()
        with pytest.raises(NotImplementedError, match=dt):
            r._boost_args(spec)
    r.index_type_used = "ivf"
    with pytest.raises(NotImplementedError, match="IVF"):
        r._boost_args(spec)
    p = _bare(RetrievalPipeline, config=PipelineConfig())
    assert p._boost_kwargs(None, None, {}) == {} and p._boost_kwargs(spec, None, {}) == {"boost": spec}
    for lam, gkw in ((0.5, {}), (None, {"group_by": "topic", "group_size": 1}), (None, {"funnel_dims": 256})):
        with pytest.raises(ValueError, match="boost"):
            p._boost_kwargs(spec, lam, gkw)
    p.config = PipelineConfig(stage1_boost=spec)
    assert p._boost_kwargs(None, None, {}) == {"boost": spec}
    # the new field is the last one (the positional order of the others is the parent's), and an export names an
    # array or a callable instead of dumping it
    from dataclasses import fields
    assert [f.name for f in fields(PipelineConfig)][-1] == "stage1_boost"
    assert p._config_dict()["stage1_boost"] == spec
    p.config = PipelineConfig(stage1_boost=np.zeros(7, np.float32))
    assert p._config_dict()["stage1_boost"] == "<array of 7 biases>"
    p.config = PipelineConfig(stage1_boost=len)
    assert p._config_dict()["stage1_boost"] == "<callable len>"
    import yaml
    assert "callable len" in yaml.safe_dump({"pipeline": p._config_dict()})
    with pytest.raises(ValueError, match="boost"):
        p._boost_kwargs(None, 0.5, {})


def test_sharded_and_ivf_classes_refuse(tmp_path):
    from tristage_rag_amd.index import IVFFlatIndex
    from tristage_rag_amd.parallel_pipeline import ShardedRetrievalPipeline
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig
    from tristage_rag_amd.sharded import ShardedFlatIPIndex
    q, b = np.zeros((1, 256), np.float32), np.zeros(4, np.float32)
    for ix in (_bare(ShardedFlatIPIndex), _bare(IVFFlatIndex, _h=None)):
        with pytest.raises(NotImplementedError, match="search_biased"):
            ix.search_biased(q, 2, b)
    kw = dict(stage1_model="random:tiny", stage2_model="random:tiny", stage3_model="random:tiny", device="cpu",
              cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"), log_file=str(tmp_path / "p.log"))
    p = ShardedRetrievalPipeline(config=PipelineConfig(**kw))
    spec = {"field": "pop"}
    with pytest.raises(NotImplementedError, match="boost"):
        p.search("a query", boost=spec)
    with pytest.raises(NotImplementedError, match="boost"):
        p.search_many(["a query"], boost=spec)
    with pytest.raises(NotImplementedError, match="boost"):
        p.batch_search(["a query"], boost=spec)
    p2 = ShardedRetrievalPipeline(config=PipelineConfig(stage1_boost=spec, **kw))
    with pytest.raises(NotImplementedError, match="boost"):
        p2.search("a query")


# --------------------------------------------------------------------------- the retriever over a host double
class BiasDoubleIndex:
    """A FlatIPIndex-shaped host double: float32 rows, tombstones, ``search_biased`` by the model of bias_model.py.  It
    records every bias object it is handed."""
    storage_dtype = "f16"
    mmr = search_grouped = None      # (named, so that the retriever's option checks get as far as the boost's)

    def __init__(self, d):
        self.d = d
        self.rows = np.zeros((0, d), np.float32)
        self.live = np.zeros(0, bool)
        self.biases = []

    @property
    def ntotal(self):
        return self.rows.shape[0]

    def add(self, x, normalize=False):
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)], 0)
        self.live = np.concatenate([self.live, np.ones(len(x), bool)])

    def _allowed(self, allowed, B):
        if allowed is None:
            return None
        from tristage_rag_amd.index import pack_allowed
        items = list(allowed) if isinstance(allowed, (list, tuple)) else [allowed] * B
        unpack = lambda a: np.unpackbits(pack_allowed(a, self.ntotal).view(np.uint8), bitorder="little")[: self.ntotal].astype(bool)
        return [None if a is None else unpack(a) for a in items]

    def search_biased(self, q, k, bias, allowed=None, exact_dense=False, check_finite=True):
        self.biases.append(bias)
        q = np.asarray(q, np.float32)
        S = (q @ self.rows.T).astype(np.float32)
        return bm.topk_model(S, np.asarray(bias, np.float32), int(k), live=self.live, allowed=self._allowed(allowed, len(q)))

    def search(self, q, k, exact_dense=False, allowed=None):
        q = np.asarray(q, np.float32)
        S = (q @ self.rows.T).astype(np.float32)
        return bm.topk_model(S, np.zeros(self.ntotal, np.float32), int(k), live=self.live, allowed=self._allowed(allowed, len(q)))

    def remove_ids(self, ids):
        ids = np.asarray(ids, np.int64)
        n = int(self.live[ids].sum())
        self.live[ids] = False
        return n

    def update_rows(self, ids, x, normalize=False):
        self.rows[np.asarray(ids, np.int64)] = np.asarray(x, np.float32)

    def compact(self):
        old2new = np.full(self.ntotal, -1, np.int64)
        old2new[self.live] = np.arange(int(self.live.sum()))
        self.rows, self.live = self.rows[self.live], np.ones(int(self.live.sum()), bool)
        return old2new

    def reconstruct_n(self, i0=0, n=None):
        return self.rows[i0: self.ntotal if n is None else i0 + n].copy()


DOCS = [f"document number {i} about topic {i % 5} with some words" for i in range(40)]
DOC_META = [{"pop": float(i % 7), "ts": 1000.0 + i} if i % 9 else {} for i in range(40)]


@pytest.fixture(scope="module")
def encoder():
    from tristage_rag_amd.encoders import SentenceEncoder
    return SentenceEncoder("random:tiny", device="cpu")


def _stage1(encoder, tmp_path, **kw):
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    cfg = Stage1Config(model_name="random:tiny", device="cpu", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
                       enable_bm25=kw.pop("enable_bm25", False), **kw)
    s1 = Stage1Retriever(cfg, model=encoder, index_factory=lambda d: BiasDoubleIndex(d))
    s1.add_documents(DOCS, DOC_META)
    return s1


def test_boost_changes_the_stage1_list_as_search_biased_does(encoder, tmp_path):
    from tristage_rag_amd import boost
    s1 = _stage1(encoder, tmp_path)
    ix = s1.faiss_index
    q = s1._normalize_embeddings(s1._encode_batch(["topic 3 words"]))
    spec = {"field": "ts", "decay": "exp", "origin": 1039.0, "scale": 5.0, "weight": 0.5, "missing": -1.0}
    bias = boost.bias_array(spec, DOC_META)
    plain = s1.search("topic 3 words", top_k=8)
    for given in (spec, bias, lambda m: float(bias[DOC_META.index(m)]) if m else -1.0):
        got = s1.search("topic 3 words", top_k=8, boost=given)
        D, I = ix.search_biased(q, 8, bias)
        assert [r["doc_id"] for r in got] == I[0].tolist()
        assert [np.float32(r["score"]) for r in got] == D[0].tolist()
    assert [r["doc_id"] for r in got] != [r["doc_id"] for r in plain]                      # the boost reorders
    assert s1.search("topic 3 words", top_k=8) == plain                                    # and off is off
    many = s1.search_many(["topic 3 words", "number 7"], top_k=5, boost=spec)
    assert [r["doc_id"] for r in many[0]] == ix.search_biased(q, 5, bias)[1][0].tolist()
    # filter= composes: the allowed documents, ranked by boosted score
    allow = np.arange(40) % 2 == 0
    got = s1.search("topic 3 words", top_k=6, filter=allow, boost=spec)
    assert [r["doc_id"] for r in got] == ix.search_biased(q, 6, bias, allowed=allow)[1][0].tolist()
    assert all(r["doc_id"] % 2 == 0 for r in got)
    with pytest.raises(ValueError, match="boost"):
        s1.search("topic 3 words", top_k=4, boost=spec, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="boost"):
        s1.search_many(["topic 3 words"], top_k=4, boost=spec, group_by="pop")
    with pytest.raises(ValueError, match="one entry per document"):
        s1.search("topic 3 words", top_k=4, boost=np.zeros(39, np.float32))
    s2 = _stage1(encoder, tmp_path, enable_bm25=True, boost=spec)                          # BM25 + RRF runs on its output
    fused = s2.search("topic 3 words", top_k=8)
    assert len(fused) == 8 and s2.faiss_index.biases, "the config's boost reached the index"


def test_the_bias_cache_is_an_lru_of_four_dropped_by_every_mutation(encoder, tmp_path):
    s1 = _stage1(encoder, tmp_path)
    ix = s1.faiss_index
    spec = {"field": "pop", "weight": 0.25}
    s1.search("topic 1", top_k=3, boost=spec)
    s1.search("topic 2", top_k=3, boost=dict(spec))                  # an equal dict is the same spec
    assert ix.biases[0] is ix.biases[1] and len(s1._boost_lru) == 1
    arrs = [np.full(40, i, np.float32) for i in range(4)]
    for a in arrs:
        s1.search("topic 1", top_k=3, boost=a)
    assert len(s1._boost_lru) == 4                                   # the dict spec, the oldest, fell out
    s1.search("topic 1", top_k=3, boost=spec)
    assert ix.biases[-1] is not ix.biases[0] and np.array_equal(ix.biases[-1], ix.biases[0])

    def cached():
        s1.search("topic 1", top_k=3, boost=spec)
        first = ix.biases[-1]
        s1.search("topic 1", top_k=3, boost=spec)
        assert ix.biases[-1] is first
        return first

    before = cached()
    s1.add_documents(["one more document"], [{"pop": 100.0}])
    assert len(s1._boost_lru) == 0
    after = cached()
    assert after is not before and after.shape == (41,) and after[40] == 25.0
    s1.update_documents([3], ["a new text"], [{"pop": 8.0}])
    assert len(s1._boost_lru) == 0
    assert cached()[3] == 2.0
    s1.update_documents([4], ["another new text"])                   # texts only: dropped all the same
    assert len(s1._boost_lru) == 0
    cached()
    assert s1.remove_documents([0, 5]) == 2
    assert len(s1._boost_lru) == 0
    got = s1.search("topic 1", top_k=41, boost=spec)
    assert len(got) == 39 and not {0, 5} & {r["doc_id"] for r in got}
    old2new = s1.compact()
    assert len(s1._boost_lru) == 0 and old2new[1] == 0
    b = cached()
    assert b.shape == (39,) and b[old2new[3]] == 2.0 and b[old2new[40]] == 25.0
    s1.doc_metadata = [dict(m, pop=1.0) for m in s1.doc_metadata]    # the metadata list is replaced
    assert np.array_equal(cached(), np.full(39, 0.25, np.float32))
