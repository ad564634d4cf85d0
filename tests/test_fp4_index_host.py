"""The fp4 (OCP e2m1 elements, one E8M0 scale per 32) stage-1 index without a GPU: the stored format against a
brute-force quantiser, the fixed point of decoding, the error lemma, the planted case of the GPU test decided by the
model, the C ABI's new dtype, and the new kernels' resource usage."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fp4_index_model as fm
from tristage_rag_amd import _lib
from tristage_rag_amd import index as ix
from tristage_rag_amd.index import decode_rows_mxfp4, quantize_rows_mxfp4_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")
EXPS = [-100, -20, -3, 0, 5, 100]


def _equal(x):
    got_c, got_e = quantize_rows_mxfp4_reference(x)
    want_c, want_e = fm.brute_force_quantize(x)
    assert got_c.dtype == np.uint8 and got_e.dtype == np.int8
    assert got_c.shape == want_c.shape and got_e.shape == want_e.shape
    assert np.array_equal(got_e, want_e), np.argwhere(got_e != want_e)[:8]
    bad = np.argwhere(got_c != want_c)
    assert bad.size == 0, [(tuple(b), int(got_c[tuple(b)]), int(want_c[tuple(b)])) for b in bad[:8]]
    return got_c, got_e


# -- 1. the reference quantiser against brute force ---------------------------------------------------------------
@pytest.mark.parametrize("e", EXPS)
def test_midpoints_and_their_neighbours(e):
    x = fm.midpoint_rows(e)
    codes, exps = _equal(x)
    assert (exps[:, 0] == e).all()
    dims = fm.block_dims(64)[0]
    # the midpoint itself goes to the even index: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    assert [int(c) for c in codes[:, dims[1]]] == [0, 2, 2, 4, 4, 6, 6]
    assert [int(c) for c in codes[:, dims[4]]] == [8, 10, 10, 12, 12, 14, 14]


@pytest.mark.parametrize("e", EXPS)
def test_amax_at_six_and_its_neighbours(e):
    x = fm.amax_rows(e)
    codes, exps = _equal(x)
    assert int(exps[0, 0]) == e and int(codes[0, 0]) == 7                   # amax = 6 * 2^e: index 7, exponent e
    assert int(exps[2, 0]) == min(e + 1, 100)                               # one ulp above: the next exponent
    assert int(exps[4, 0]) == e                                             # one ulp below
    assert ((codes & 7) <= 7).all()


def test_zero_blocks_signed_zero_nan_inf_and_the_clamps():
    x = fm.special_rows()
    codes, exps = _equal(x)
    dims = fm.block_dims(64)[0]
    first = lambda r: [int(c) for c in codes[r, dims[:3]]]
    assert int(exps[0, 0]) == 0 and (codes[0] == 0).all()                    # a zero block
    assert first(1) == [8, 0, 0] and int(exps[1, 0]) == 0                     # -0 keeps its sign bit
    assert first(2) == [0, 0, 0] and int(exps[2, 0]) == 0                     # NaN counts as 0
    assert first(3)[0] == 0 and first(3)[2] == 0 and int(exps[3, 0]) == -2    # amax = 1: 4 * 2^-2
    assert int(exps[4, 0]) == 100 and first(4) == [7, 0, 0]                   # +Inf = FLT_MAX, clamped exponent: 6
    assert int(exps[5, 0]) == 100 and first(5)[0] == 15
    assert int(exps[6, 0]) == -100 and first(6) == [0, 0, 8]                  # 2^-120 under the lower clamp: 0
    assert int(exps[7, 0]) == 100 and first(7) == [7, 15, 0]                  # 2^120 over the upper clamp: 6
    dec = decode_rows_mxfp4(codes, exps, 64)
    assert np.isfinite(dec).all()


@pytest.mark.parametrize("d", [64, 100, 768])
def test_random_rows_match_brute_force(d):
    x = fm.wide_rows(24, d, seed=d)
    codes, exps = _equal(x)
    assert codes.shape == (24, -(-d // 64) * 64) and exps.shape == (24, codes.shape[1] // 32)
    dec = decode_rows_mxfp4(codes, exps, d)
    assert dec.dtype == np.float32 and dec.shape == (24, d)
    assert np.array_equal(dec.astype(np.float64), fm.decode64(codes, exps, d))      # the decoder is exact
    assert np.array_equal(fm.to_bf16_f32(dec).view(np.uint32), dec.view(np.uint32))  # and exact in bf16


# -- 2. decoding is a fixed point in values -----------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 768])
def test_decode_is_a_fixed_point_in_values(d):
    x = np.concatenate([fm.wide_rows(200, d, seed=d + 1), fm.unit_rows(200, d, seed=d + 2)])
    c1, e1 = quantize_rows_mxfp4_reference(x)
    dec1 = decode_rows_mxfp4(c1, e1, d)
    c2, e2 = quantize_rows_mxfp4_reference(dec1)
    dec2 = decode_rows_mxfp4(c2, e2, d)
    assert np.array_equal(dec1.view(np.uint32), dec2.view(np.uint32))
    assert (e2 <= e1).all()                                                   # (a block whose largest code is 3 moves down)


def test_every_code_and_exponent_is_a_fixed_point():
    g = np.random.default_rng(0)
    codes = g.integers(0, 16, size=(400, 64)).astype(np.uint8)
    codes[:16, :] = np.arange(16, dtype=np.uint8)[:, None]                    # blocks of one code, every largest code
    exps = g.integers(-100, 101, size=(400, 2)).astype(np.int8)
    dec1 = decode_rows_mxfp4(codes, exps, 64)
    c2, e2 = quantize_rows_mxfp4_reference(dec1)
    dec2 = decode_rows_mxfp4(c2, e2, 64)
    # A block whose largest magnitude index is M re-quantises with e, e - 1, e - 2 or e - 3 (M = 6..7, 4..5, 2..3, 1)
    # or, where that is below the clamp, with -100 <= e; a grid value times a power of two that stays <= 6 is a grid
    # value again, so the decoded values come back bit for bit.
    assert np.array_equal(dec1.view(np.uint32), dec2.view(np.uint32))
    assert (e2 <= np.maximum(exps, 0)).all()


def test_input_dtypes_give_the_codes_of_their_f32_values():
    import torch
    x = torch.randn(7, 100) * 3
    want = quantize_rows_mxfp4_reference(x.numpy())
    got = quantize_rows_mxfp4_reference(x)
    assert want[0].shape == (7, 128) and want[1].shape == (7, 4)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for dt in (torch.float16, torch.bfloat16):
        a = quantize_rows_mxfp4_reference(x.to(dt))
        b = quantize_rows_mxfp4_reference(x.to(dt).float().numpy())
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a = quantize_rows_mxfp4_reference(x.numpy().astype(np.float16))
    b = quantize_rows_mxfp4_reference(x.numpy().astype(np.float16).astype(np.float32))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        quantize_rows_mxfp4_reference(np.zeros(5, np.float32))


# -- 3. the error lemma -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 768])
def test_error_lemma(d):
    x = fm.unit_rows(300, d, seed=d)
    q = fm.unit_rows(16, d, seed=d + 1)
    dec = decode_rows_mxfp4(*quantize_rows_mxfp4_reference(x), d).astype(np.float64)
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    delta = fm.deltas(x)                                         # (exponents from the model, not from the code under test)
    assert np.array_equal(fm.model_exponents(x[:6]), fm.brute_force_quantize(x[:6])[1])
    assert np.array_equal(fm.model_exponents(x), quantize_rows_mxfp4_reference(x)[1])
    assert (np.abs(dec - x64) <= delta).all()                    # per element, which is what the lemma sums
    err = np.abs(q64 @ dec.T - q64 @ x64.T)
    bound = fm.lemma_bound(q, x)
    assert (err <= bound).all(), float((err - bound).max())


def test_planted_case_is_decided_by_the_model():
    q, rows, planted = fm.planted_case()
    dec = decode_rows_mxfp4(*quantize_rows_mxfp4_reference(rows), rows.shape[1]).astype(np.float64)
    S = fm.to_bf16_f32(q).astype(np.float64) @ dec.T
    for j in range(q.shape[0]):
        other = np.setdiff1d(np.arange(rows.shape[0]), planted[j])
        lo, hi = S[j, planted[j]].min(), S[j, other].max()
        print(f"query {j}: smallest planted score {lo:.3f}, largest other score {hi:.3f}")
        assert lo > hi + 1e-3, (j, lo, hi)                       # (1e-3: far above the f32 accumulation error at d = 64)


# -- 4. names, configuration, refusals --------------------------------------------------------------------------
def test_c_abi_carries_the_dtype():
    lib = _lib.load()
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"TS_MXFP4_E2M1\s*=\s*4\b", header)
    assert _lib.TS_MXFP4_E2M1 == 4
    assert lib.ts_abi_version() == 4 and _lib.header_abi_version() == 4
    assert lib.ts_coalesce_groups(768, _lib.TS_MXFP4_E2M1) == 0
    assert lib.ts_coalesce_groups_wide(768, _lib.TS_MXFP4_E2M1) == 0
    assert lib.ts_coalesce_groups_stationary(768, _lib.TS_MXFP4_E2M1) == 0
    h = ctypes.c_void_p()
    assert lib.ts_index_create(0, _lib.TS_MXFP4_E2M1, 0, 0, ctypes.byref(h)) == _lib.TS_ERR_INVALID
    assert lib.ts_index_create(64, 5, 0, 0, ctypes.byref(h)) == _lib.TS_ERR_INVALID


def test_name_maps_and_config_fields_carry_fp4():
    for name in ("fp4", "mxfp4", "e2m1"):
        assert ix._NAME_TO_DTYPE[name] == _lib.TS_MXFP4_E2M1
    assert ix._DTYPE_NAME[_lib.TS_MXFP4_E2M1] == "fp4"
    from tristage_rag_amd.stage1_retriever import Stage1Config
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig
    assert Stage1Config(index_dtype="fp4").index_dtype == "fp4"
    assert PipelineConfig(stage1_index_dtype="fp4").stage1_index_dtype == "fp4"


def test_refusals_need_no_gpu():
    with pytest.raises(NotImplementedError, match="fp4"):
        ix.IVFFlatIndex(64, 4, dtype="fp4")
    with pytest.raises(NotImplementedError, match="fp4"):
        ix.FlatIPIndex(2304, dtype="fp4")
    from tristage_rag_amd.sharded import ShardedFlatIPIndex
    with pytest.raises(NotImplementedError, match="fp4"):
        ShardedFlatIPIndex(64, 100, dtype="fp4")

    class _Fp4Double:
        storage_dtype = "fp4"
    with pytest.raises(NotImplementedError, match="fp4"):
        ShardedFlatIPIndex(64, 100, dtype="f16", local_index=_Fp4Double())


# -- 5. build: the new kernels compile for gfx950 and use no scratch -----------------------------------------------
def test_fp4_scan_kernels_use_no_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                          "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "-c", "ts_scan_fp4.hip",
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
    scans = {k: v for k, v in found.items() if "scan_kernel" in k and "OpFp4" in k and "WalkStrided" in k}
    masked = {k: v for k, v in found.items() if "scan_kernel" in k and "OpFp4" in k and "WalkLive" in k}
    assert len(scans) == 4 and len(masked) == 2, sorted(found)      # QH {1, 2} x {dense, filter}; QH {1, 2}
    others = {k: v for k, v in found.items() if any(t in k for t in ("relayout_fp4", "reconstruct_fp4", "upd_rows_fp4"))}
    assert len(others) == 5, sorted(found)                          # relayout x 3 input types, reconstruct, update
    assert len(found) == 11, sorted(found)
    assert all(v == 0 for v in found.values()), found
