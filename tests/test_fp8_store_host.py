"""The e4m3 stage-2 token store without a GPU: the stored format (index.quantize_rows_fp8_reference), the C ABI's
argument checks, the fp8 kernels' resource usage, and the pipeline with an fp8 store on CPU doubles."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tristage_rag_amd import _lib
from tristage_rag_amd.index import quantize_rows_fp8, quantize_rows_fp8_reference
from tests.doubles import oracle_maxsim_indexed, oracle_maxsim_indexed_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")


def _scale_exponent(x: torch.Tensor) -> torch.Tensor:
    """k of every row, recovered from the stored bytes: decode(q) = round(x * 2^k), and the largest |x_i| is rounded by
    less than 1/16 of itself, so k is the nearest integer to log2(largest decoded / largest input)."""
    q = quantize_rows_fp8_reference(x).float()
    ratio = q.abs().amax(dim=1).double() / x.abs().amax(dim=1).double()
    return torch.round(torch.log2(ratio))


# -- 1. the reference quantiser ---------------------------------------------------------------------------------
def test_scale_rule_every_row():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2000, 96, generator=g) * torch.exp(torch.randn(2000, 1, generator=g) * 8)
    q = quantize_rows_fp8_reference(x)
    assert q.dtype == torch.float8_e4m3fn and q.shape == x.shape
    m = x.abs().amax(dim=1).double()
    mant, e = torch.frexp(m)
    k = torch.where(mant <= 0.875, 9 - e, 8 - e).double()
    scaled = m * torch.pow(2.0, k)
    assert bool(((scaled > 224) & (scaled <= 448)).all())
    # the largest element decodes to the scaled maximum rounded: within (224, 448]
    dec_max = q.float().abs().amax(dim=1)
    assert bool(((dec_max >= 224) & (dec_max <= 448)).all())


@pytest.mark.parametrize("m", [2.0 ** e for e in range(-30, 31, 3)] + [448.0, 224.0, 0.875, 1.75, 2.0 ** -140])
def test_scale_exact_at_powers_of_two_and_448(m):
    x = torch.tensor([[m, -m / 3, m / 7, 0.0] + [0.0] * 12], dtype=torch.float32)
    q = quantize_rows_fp8_reference(x).float()
    mant, e = np.frexp(m)
    k = (9 - e) if mant <= 0.875 else (8 - e)
    assert m * 2.0 ** k <= 448 and m * 2.0 ** (k + 1) > 448
    assert float(q[0, 0]) == m * 2.0 ** k            # exact: the maximum itself is representable after scaling
    if m == 448.0:
        assert float(q[0, 0]) == 448.0 and k == 0
    if m in (1.0, 2.0 ** -3, 2.0 ** 30):              # a power of two lands on 256 exactly
        assert float(q[0, 0]) == 256.0


def test_zero_row_nan_inf_rows():
    x = torch.zeros(4, 32)
    x[1, 5] = float("nan")
    x[2, 0] = float("inf")
    x[3, 31] = float("-inf")
    x[1:, 1] = 3.0
    b = quantize_rows_fp8_reference(x).view(torch.uint8)
    assert bool((b[0] == 0).all())
    for r in (1, 2, 3):
        assert bool((b[r] == 0x7F).all()), b[r]
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(quantize_rows_fp8_reference(x.to(dt)).view(torch.uint8), b)


def test_subnormals_kept_and_ties_to_even():
    # max 448 -> k = 0, so the other elements are stored as they are: e4m3 subnormals are multiples of 2^-9
    sub = [2.0 ** -9, 3 * 2.0 ** -9, 7 * 2.0 ** -9, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 0.5 * 2.0 ** -9, 0.75 * 2.0 ** -9]
    want_sub = [1, 3, 7, 2, 2, 0, 1]           # 1.5 -> 2 (even), 2.5 -> 2 (even), 0.5 -> 0 (even), 0.75 -> 1
    # ties between normal neighbours: 1.0625 is halfway between 1.0 (mantissa 0) and 1.125 (mantissa 1) -> 1.0;
    # 1.1875 is halfway between 1.125 and 1.25 -> 1.25 (mantissa 2, even); 17 halfway 16 / 18 -> 16; 19 -> 20
    ties = [1.0625, 1.1875, 17.0, 19.0, -1.0625]
    want_ties = [1.0, 1.25, 16.0, 20.0, -1.0]
    row = torch.tensor([[448.0] + sub + ties + [0.0] * (16 - 1 - len(sub) - len(ties) + 16)], dtype=torch.float32)
    q = quantize_rows_fp8_reference(row)
    b = q.view(torch.uint8)[0]
    for i, w in enumerate(want_sub):
        assert int(b[1 + i]) == w, (i, int(b[1 + i]))
    dec = q.float()[0]
    for i, w in enumerate(want_ties):
        assert float(dec[1 + len(sub) + i]) == w


def test_decode_within_half_ulp():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(500, 128, generator=g) * torch.exp(torch.randn(500, 1, generator=g) * 4)
    q = quantize_rows_fp8_reference(x).float().double()
    k = _scale_exponent(x)
    xs = x.double() * torch.pow(2.0, k).unsqueeze(1)          # the scaled input, exact in float64
    err = (q - xs).abs()
    # half an e4m3 ulp of the scaled value: 2^(e - 3 - 1) for |v| in [2^e, 2^(e+1)), e >= -6; 2^-10 below 2^-6
    e = torch.floor(torch.log2(xs.abs().clamp(min=2.0 ** -6)))
    half_ulp = torch.pow(2.0, e - 4)
    assert bool((err <= half_ulp + 0.0).all()), float((err - half_ulp).max())
    # and back in the input's scale
    assert bool(((q * torch.pow(2.0, -k).unsqueeze(1) - x.double()).abs()
                 <= half_ulp * torch.pow(2.0, -k).unsqueeze(1)).all())


def test_cpu_quantize_is_the_reference():
    x = torch.randn(64, 48, dtype=torch.bfloat16)
    assert torch.equal(quantize_rows_fp8(x).view(torch.uint8), quantize_rows_fp8_reference(x).view(torch.uint8))


# -- 2. the C ABI without a GPU -------------------------------------------------------------------------------
def test_new_symbols_bound_and_abi_version():
    lib = _lib.load()
    for name in ("ts_quantize_rows_fp8", "ts_maxsim_indexed_fp8", "ts_maxsim_indexed_batch_fp8"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ts_abi_version() == 4
    assert _lib.TS_FP8_E4M3 == 3


def _buf(n=4096):
    return (ctypes.c_uint8 * n)()


def test_fp8_entry_points_validate_before_any_hip_call():
    lib = _lib.load()
    q, st, s64, l32, out = _buf(), _buf(), _buf(), _buf(), _buf()
    qo = (ctypes.c_int32 * 3)(0, 4, 8)
    co = (ctypes.c_int32 * 3)(0, 2, 4)
    P = ctypes.addressof
    ok = dict(q=P(q), st=P(st), s=P(s64), l=P(l32), o=P(out))

    def single(q=ok["q"], q_dtype=_lib.TS_BF16, Lq=4, store=ok["st"], starts=ok["s"], lens=ok["l"], n=2, H=64,
               mode=0, out=ok["o"]):
        return lib.ts_maxsim_indexed_fp8(q, q_dtype, Lq, store, starts, lens, n, H, mode, out, 0, None)

    def batch(q=ok["q"], q_dtype=_lib.TS_BF16, q_off=P(qo), nq=2, store=ok["st"], starts=ok["s"], lens=ok["l"],
              c_off=P(co), H=64, mode=0, out=ok["o"]):
        return lib.ts_maxsim_indexed_batch_fp8(q, q_dtype, q_off, nq, store, starts, lens, c_off, H, mode, out, 0, None)

    for kw in ({"q": None}, {"store": None}, {"starts": None}, {"lens": None}, {"out": None}, {"q_dtype": _lib.TS_F32},
               {"q_dtype": _lib.TS_FP8_E4M3}, {"q_dtype": 7}, {"mode": 2}, {"Lq": 0}, {"n": -1}, {"H": 0}):
        assert single(**kw) == _lib.TS_ERR_INVALID, kw
    for kw in ({"q": None}, {"q_off": None}, {"store": None}, {"starts": None}, {"lens": None}, {"c_off": None},
               {"out": None}, {"q_dtype": _lib.TS_F32}, {"q_dtype": _lib.TS_FP8_E4M3}, {"mode": 3}, {"nq": -1}):
        assert batch(**kw) == _lib.TS_ERR_INVALID, kw
    bad_q = (ctypes.c_int32 * 3)(0, 4, 2)
    bad_c = (ctypes.c_int32 * 3)(0, 3, 1)
    assert batch(q_off=P(bad_q)) == _lib.TS_ERR_INVALID
    assert batch(c_off=P(bad_c)) == _lib.TS_ERR_INVALID
    # H % 16 != 0: unsupported (there is no general kernel behind the e4m3 store)
    for H in (8, 104, 770):
        assert single(H=H) == _lib.TS_ERR_UNSUPPORTED
        assert batch(H=H) == _lib.TS_ERR_UNSUPPORTED
    # the quantiser
    qz = lib.ts_quantize_rows_fp8
    assert qz(None, _lib.TS_F32, 4, 64, ok["o"], 0, None) == _lib.TS_ERR_INVALID
    assert qz(ok["q"], _lib.TS_F32, 4, 64, None, 0, None) == _lib.TS_ERR_INVALID
    assert qz(ok["q"], _lib.TS_FP8_E4M3, 4, 64, ok["o"], 0, None) == _lib.TS_ERR_INVALID
    assert qz(ok["q"], _lib.TS_F32, -1, 64, ok["o"], 0, None) == _lib.TS_ERR_INVALID
    assert qz(ok["q"], _lib.TS_BF16, 4, 104, ok["o"], 0, None) == _lib.TS_ERR_UNSUPPORTED
    # the existing entry points keep rejecting the e4m3 type
    assert lib.ts_maxsim_indexed(ok["q"], 4, ok["st"], ok["s"], ok["l"], 2, 64, _lib.TS_FP8_E4M3, 0, ok["o"], 0,
                                 None) == _lib.TS_ERR_INVALID
    assert lib.ts_maxsim_indexed_batch(ok["q"], P(qo), 2, ok["st"], ok["s"], ok["l"], P(co), 64, _lib.TS_FP8_E4M3, 0,
                                       ok["o"], 0, None) == _lib.TS_ERR_INVALID
    assert lib.ts_maxsim(ok["q"], 4, ok["st"], ok["s"], 2, 64, _lib.TS_FP8_E4M3, 0, ok["o"], 0, None) == _lib.TS_ERR_INVALID
    assert lib.ts_abi_version() == 4


# -- 3. build: no scratch in any fp8 instantiation ------------------------------------------------------------
def _resource_usage(src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                          "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", os.devnull], cwd=CSRC, capture_output=True, text=True, check=True).stderr
    found, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            found[name] = int(m.group(1))
    return found


def test_fp8_kernels_use_no_scratch():
    m16 = {k: v for k, v in _resource_usage("ts_maxsim16.hip").items() if k.startswith("_Z15maxsim16_kernelILi3E")}
    # e4m3 store x {f16, bf16} query x NQT {1, 2} x single / batch x (16-deep ring full / partial, 24-deep ring)
    assert len(m16) == 24, sorted(m16)
    assert all(v == 0 for v in m16.values()), m16
    qz = {k: v for k, v in _resource_usage("ts_fp8.hip").items() if "quantize_rows_fp8_kernel" in k}
    assert len(qz) == 3 and all(v == 0 for v in qz.values()), qz


# -- 4. the pipeline with an fp8 store (CPU doubles) ---------------------------------------------------------
from tests.test_host_logic import DOCS, _pipeline  # noqa: E402
from tristage_rag_amd.encoders import SentenceEncoder  # noqa: E402


@pytest.fixture(scope="module")
def encoder():
    return SentenceEncoder("random:tiny", device="cpu")


def _build(encoder, tmp_path, sub, dtype, docs=DOCS):
    p = _pipeline(encoder, tmp_path / sub, stage1_enable_bm25=False, stage2_precompute_document_embeddings=True,
                  stage2_token_store_dtype=dtype)
    p.stage2._maxsim_indexed_fn, p.stage2._maxsim_indexed_batch_fn = oracle_maxsim_indexed, oracle_maxsim_indexed_batch
    p.stage2.config.precompute_document_embeddings = True
    p.stage2.config.token_store_dtype = dtype
    if docs is not None:
        p.add_documents(docs)
    return p


QUERIES = ["neural networks attention", "language models", "retrieval of documents", "x"]


def test_pipeline_fp8_store(encoder, tmp_path):
    a = _build(encoder, tmp_path, "f8", "fp8")
    b = _build(encoder, tmp_path, "b16", "bf16")
    sa, sb = a.stage2.token_store, b.stage2.token_store
    assert sa.data.dtype == torch.float8_e4m3fn and sb.data.dtype == torch.bfloat16
    assert sa.lens == sb.lens and sa.rows == sb.rows
    assert sa.rows * sa.data.shape[1] * sa.data.element_size() * 2 == sb.rows * sb.data.shape[1] * sb.data.element_size()
    assert a.stage2.get_model_info()["token_store_dtype"] == "fp8"
    assert a.get_pipeline_info()["stage2_token_store_dtype"] == "fp8"
    assert b.get_pipeline_info()["stage2_token_store_dtype"] == "bf16"
    many = a.search_many(QUERIES)
    for q, m in zip(QUERIES, many):
        one = a.search(q)
        assert [r["doc_id"] for r in one["results"]] == [r["doc_id"] for r in m["results"]]
        for x, y in zip(one["results"], m["results"]):
            assert x["stage2_score"] == pytest.approx(y["stage2_score"], abs=1e-6)
    # stage-2 scores against the bf16 store's, candidate by candidate
    for q in QUERIES:
        cands = [{"doc_id": i, "document": d} for i, d in enumerate(DOCS)]
        fa = a.stage2.score_candidates(q, cands)
        fb = b.stage2.score_candidates(q, cands)
        assert np.abs(np.array(fa) - np.array(fb)).max() <= 5e-3


def test_pipeline_fp8_store_persistence(encoder, tmp_path):
    a = _build(encoder, tmp_path, "a", "fp8")
    want = a.search("neural networks attention")
    path = str(tmp_path / "idx" / "pipeline_index.pkl")
    a.save_index(path)
    tok = str(tmp_path / "idx" / "pipeline_index.stage2_tokens.safetensors")
    from safetensors import safe_open
    with safe_open(tok, framework="pt") as f:
        assert f.metadata()["format"] == "tristage-rag_amd/token-store-fp8/1"
        assert f.get_tensor("tokens").dtype == torch.float8_e4m3fn
    b = _build(encoder, tmp_path, "b", "fp8", docs=None)
    b.load_index(path)
    sa, sb = a.stage2.token_store, b.stage2.token_store
    assert sb.data.dtype == torch.float8_e4m3fn and sb.lens == sa.lens
    assert torch.equal(sb.data[: sb.rows].view(torch.uint8).cpu(), sa.data[: sa.rows].view(torch.uint8).cpu())
    got = b.search("neural networks attention")
    assert [(r["doc_id"], r["stage2_score"]) for r in got["results"]] == \
        [(r["doc_id"], r["stage2_score"]) for r in want["results"]]
    # an fp8 file makes a bf16 scorer re-encode (it never reads one-byte rows as two-byte ones)
    c = _build(encoder, tmp_path, "c", "bf16", docs=None)
    calls = []
    orig = c.stage2.index_documents
    c.stage2.index_documents = lambda *a_, **k_: (calls.append(1), orig(*a_, **k_))[1]
    c.load_index(path)
    assert calls and c.stage2.token_store.data.dtype == torch.bfloat16 and len(c.stage2.token_store) == len(DOCS)


def test_bf16_file_migrates_into_fp8_scorer(encoder, tmp_path):
    a = _build(encoder, tmp_path, "a", "bf16")
    path = str(tmp_path / "idx" / "pipeline_index.pkl")
    a.save_index(path)
    b = _build(encoder, tmp_path, "b", "fp8", docs=None)
    calls = []
    orig = b.stage2.index_documents
    b.stage2.index_documents = lambda *a_, **k_: (calls.append(1), orig(*a_, **k_))[1]
    b.load_index(path)
    assert not calls                                   # quantised on load, not re-encoded
    sa, sb = a.stage2.token_store, b.stage2.token_store
    assert sb.data.dtype == torch.float8_e4m3fn and sb.lens == sa.lens
    want = quantize_rows_fp8_reference(sa.data[: sa.rows].cpu())
    assert torch.equal(sb.data[: sb.rows].cpu().view(torch.uint8), want.view(torch.uint8))


def test_unsupported_hidden_size_raises_at_index_time():
    from tristage_rag_amd.stage2_rescorer import ColBERTScorer, Stage2Config

    sc = ColBERTScorer(Stage2Config(model_name="random:tiny", device="cpu", token_store_dtype="fp8",
                                    precompute_document_embeddings=True))
    sc._forward = lambda enc: torch.randn(enc["attention_mask"].shape[0], enc["attention_mask"].shape[1], 104)
    with pytest.raises(ValueError, match="H = 104"):
        sc.index_documents(["a document", "another one"], 0)
    assert len(sc.token_store) == 0
