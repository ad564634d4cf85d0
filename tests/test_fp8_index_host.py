"""The fp8 (e4m3) stage-1 index without a GPU: the stored format against a brute-force quantiser, the error lemma,
the C ABI's new symbols, and the new kernels' resource usage."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fp8_index_model as fm
from tristage_rag_amd import _lib
from tristage_rag_amd import index as ix
from tristage_rag_amd.index import decode_rows_e4m3_fixed, quantize_rows_e4m3_fixed_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")
SCALES = [0, 8, 15]


# -- 1. the reference quantiser against brute force ---------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES)
def test_midpoints_and_their_neighbours(s):
    x = fm.midpoint_inputs(s)
    got = quantize_rows_e4m3_fixed_reference(x, s)
    want = fm.brute_force_quantize(x, s)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:8]]


@pytest.mark.parametrize("s", SCALES)
def test_subnormals_zeros_saturation_inf_nan(s):
    x = fm.special_inputs(s)
    got = quantize_rows_e4m3_fixed_reference(x, s)
    want = fm.brute_force_quantize(x, s)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    one = lambda v: int(quantize_rows_e4m3_fixed_reference(np.array([v], dtype=np.float32), s)[0])
    sc = 2.0 ** -s
    assert one(0.0) == 0x00 and one(-0.0) == 0x80
    assert one(np.inf) == 0x7E and one(-np.inf) == 0xFE and one(np.nan) == 0x7F
    assert one(1e30) == 0x7E and one(-1e30) == 0xFE and one(448 * sc) == 0x7E and one(464 * sc) == 0x7E
    assert one(2.0 ** -9 * sc) == 0x01 and one(2.0 ** -10 * sc) == 0x00 and one(1.5 * 2.0 ** -9 * sc) == 0x02
    assert one(7.5 * 2.0 ** -9 * sc) == 0x08 and one(2.0 ** -6 * sc) == 0x08


@pytest.mark.parametrize("s", SCALES)
def test_random_inputs_match_brute_force(s):
    g = np.random.default_rng(s)
    x = (g.standard_normal(4000) * np.exp(g.standard_normal(4000) * 4) * 2.0 ** -s).astype(np.float32)
    assert np.array_equal(quantize_rows_e4m3_fixed_reference(x, s), fm.brute_force_quantize(x, s))


@pytest.mark.parametrize("s", SCALES)
def test_quantise_of_decode_is_identity(s):
    b = np.array([v for v in range(256) if v & 0x7F != 0x7F], dtype=np.uint8)
    dec = decode_rows_e4m3_fixed(b, s)
    assert dec.dtype == np.float32
    assert np.array_equal(dec.astype(np.float64), fm.TABLE[b] * 2.0 ** -s)      # the decoder is exact
    assert np.array_equal(quantize_rows_e4m3_fixed_reference(dec, s), b)
    assert np.isnan(decode_rows_e4m3_fixed(np.array([0x7F, 0xFF], dtype=np.uint8), s)).all()


def test_input_dtypes_and_shapes():
    import torch
    x = torch.randn(7, 33)
    want = quantize_rows_e4m3_fixed_reference(x.numpy(), 8)
    assert want.shape == (7, 33) and want.dtype == np.uint8
    assert np.array_equal(quantize_rows_e4m3_fixed_reference(x, 8), want)
    for dt in (torch.float16, torch.bfloat16):
        assert np.array_equal(quantize_rows_e4m3_fixed_reference(x.to(dt), 8),
                              quantize_rows_e4m3_fixed_reference(x.to(dt).float().numpy(), 8))
    for s in (-1, 16):
        with pytest.raises(ValueError):
            quantize_rows_e4m3_fixed_reference(x, s)


# -- 2. the error lemma -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 384, 768])
@pytest.mark.parametrize("s", [0, 8])
def test_error_lemma(d, s):
    x = fm.unit_rows(400, d, seed=d)
    q = fm.unit_rows(16, d, seed=d + 1)
    dec = decode_rows_e4m3_fixed(quantize_rows_e4m3_fixed_reference(x, s), s).astype(np.float64)
    err = np.abs(q.astype(np.float64) @ dec.T - q.astype(np.float64) @ x.astype(np.float64).T)
    bound = fm.lemma_bound(q, x, s)
    assert (err <= bound).all(), float((err - bound).max())
    # per element, which is what the lemma sums
    xs = np.abs(x.astype(np.float64))
    assert (np.abs(dec - x) <= 2.0 ** -4 * xs + 2.0 ** -(10 + s)).all()


# -- 3. the C ABI ---------------------------------------------------------------------------------------------------
def test_new_symbols_declared_bound_and_exported():
    lib = _lib.load()
    header = open(_lib.HEADER_PATH).read()
    for name in ("ts_index_set_fp8_scale_log2", "ts_index_fp8_scale_log2"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert lib.ts_abi_version() == 4 and _lib.header_abi_version() == 4
    assert _lib.TS_FP8_E4M3 == 3
    # null handles are refused before any HIP call
    assert lib.ts_index_set_fp8_scale_log2(None, 8) == _lib.TS_ERR_INVALID
    assert lib.ts_index_fp8_scale_log2(None) == -1
    assert lib.ts_coalesce_groups(768, _lib.TS_FP8_E4M3) == 0
    assert lib.ts_coalesce_groups_wide(768, _lib.TS_FP8_E4M3) == 0


def test_name_maps_carry_fp8():
    assert ix._NAME_TO_DTYPE["fp8"] == _lib.TS_FP8_E4M3
    assert ix._DTYPE_NAME[_lib.TS_FP8_E4M3] == "fp8"
    from tristage_rag_amd.stage1_retriever import Stage1Config
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig
    assert Stage1Config(index_dtype="fp8").index_dtype == "fp8"
    assert PipelineConfig(stage1_index_dtype="fp8").stage1_index_dtype == "fp8"


def test_refusals_need_no_gpu():
    with pytest.raises(NotImplementedError):
        ix.IVFFlatIndex(64, 4, dtype="fp8")
    with pytest.raises(NotImplementedError):
        ix.FlatIPIndex(2304, dtype="fp8")
    with pytest.raises(ValueError):
        ix.FlatIPIndex(64, dtype="fp8", fp8_scale_log2=16)
    from tristage_rag_amd.sharded import ShardedFlatIPIndex
    with pytest.raises(NotImplementedError):
        ShardedFlatIPIndex(64, 100, dtype="fp8")

    class _Fp8Double:
        storage_dtype = "fp8"
    with pytest.raises(NotImplementedError):
        ShardedFlatIPIndex(64, 100, dtype="f16", local_index=_Fp8Double())


# -- 4. build: the new kernels compile for gfx950 and use no scratch -----------------------------------------------
def test_fp8_scan_kernels_use_no_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                          "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "-c", "ts_scan_fp8.hip",
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
    scans = {k: v for k, v in found.items() if "scan_kernel" in k and "OpFp8" in k and "WalkStrided" in k}
    masked = {k: v for k, v in found.items() if "scan_kernel" in k and "OpFp8" in k and "WalkLive" in k}
    assert len(scans) == 4 and len(masked) == 2, sorted(found)      # QH {1, 2} x {dense, filter}; QH {1, 2}
    others = {k: v for k, v in found.items() if any(t in k for t in ("qprep_fp8", "relayout_fp8", "reconstruct_fp8"))}
    assert len(others) == 7, sorted(found)
    assert all(v == 0 for v in found.values()), found
