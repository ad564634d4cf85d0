"""The marshalling helpers of tristage_rag_amd/index.py that need neither a GPU nor the library: the host-pointer query
normaliser, the host half of the ``allowed`` marshaller, the output helper and the error mapper.  Expected values come
from ``np.packbits`` / plain numpy here, never from the helpers or what they call."""
import numpy as np
import pytest
import torch

from tristage_rag_amd import _lib
from tristage_rag_amd import index as ix

D = 24
EMPTY_TEXT = "No documents indexed. Call add_documents() first."   # reference src/stage1_retriever.py:370-371
OUT_TEXT = "out must be contiguous (float32[B,k], int64[B,k]) CUDA tensors"


@pytest.fixture
def no_native(monkeypatch):
    """torch and the library are out of reach of index.py: a helper that asks for either fails the test."""
    def refuse(*a, **kw):
        raise AssertionError("this helper must not need torch or the library")
    monkeypatch.setattr(ix, "_torch", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def rows(B=5, d=D, seed=0):
    return np.random.default_rng(seed).standard_normal((B, d)).astype(np.float32)


# ---- query normaliser, host-pointer policy --------------------------------------------------------------------
@pytest.mark.parametrize("dtype, code", [(np.float32, _lib.TS_F32), (np.float16, _lib.TS_F16)])
def test_host_query_keeps_contiguous_f32_f16_in_place(no_native, dtype, code):
    x = rows().astype(dtype)
    y, dt, B, on_gpu = ix._host_query(x, D)
    assert np.shares_memory(y, x) and y.dtype == dtype and y.flags.c_contiguous
    assert (dt, B, on_gpu) == (code, 5, False)
    assert ix._addr(y) == x.ctypes.data


@pytest.mark.parametrize("make, want_dtype", [
    (lambda x: x.astype(np.float64), np.float32),
    (lambda x: (x * 8).astype(np.int32), np.float32),
    (lambda x: np.asfortranarray(x), np.float32),
    (lambda x: np.asfortranarray(x.astype(np.float16)), np.float16),
    (lambda x: x[::2], np.float32),
], ids=["float64", "int32", "fortran_f32", "fortran_f16", "strided"])
def test_host_query_converts_to_contiguous_f32_or_f16(no_native, make, want_dtype):
    x = make(rows(6))
    y, dt, B, on_gpu = ix._host_query(x, D)
    assert isinstance(y, np.ndarray) and y.dtype == want_dtype and y.flags.c_contiguous
    assert np.array_equal(y, x.astype(want_dtype))
    assert dt == (_lib.TS_F16 if want_dtype == np.float16 else _lib.TS_F32) and B == x.shape[0] and not on_gpu


@pytest.mark.parametrize("tdtype", [torch.bfloat16, torch.float16, torch.float32, torch.float64])
def test_host_query_cpu_tensor_becomes_f32_numpy(tdtype):
    t = torch.from_numpy(rows()).to(tdtype)
    y, dt, B, on_gpu = ix._host_query(t, D)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.flags.c_contiguous
    assert np.array_equal(y, t.float().numpy())
    assert (dt, B, on_gpu) == (_lib.TS_F32, 5, False)


def test_host_query_shape_errors(no_native):
    with pytest.raises(ValueError) as e:
        ix._host_query(np.zeros((3, D + 1), np.float32), D)
    assert str(e.value) == f"expected [B, {D}] queries, got (3, {D + 1})"
    with pytest.raises(ValueError) as e:
        ix._host_query(np.zeros(D, np.float32), D)
    assert str(e.value) == f"expected [B, {D}] queries, got ({D},)"
    with pytest.raises(ValueError) as e:
        ix._host_query(torch.zeros((3, D + 1)), D, "rows", "n")
    assert str(e.value) == f"expected [n, {D}] rows, got (3, {D + 1})"
    with pytest.raises(ValueError) as e:   # a row count the input must have (update_rows)
        ix._host_query(np.zeros((4, D), np.float32), D, "rows", 3)
    assert str(e.value) == f"expected [3, {D}] rows, got (4, {D})"
    assert ix._host_query(np.zeros((3, D), np.float32), D, "rows", 3)[2] == 3


# ---- allowed marshaller, host half ----------------------------------------------------------------------------
def packed(m, n):
    """A bool mask -> ceil(n / 32) little-endian uint32 words, bit r % 32 of word r // 32 = row r."""
    b = np.zeros((n + 31) // 32 * 4, dtype=np.uint8)
    p = np.packbits(np.asarray(m, dtype=bool), bitorder="little")
    b[: p.shape[0]] = p
    return b.view("<u4")


def two_masks(n, seed=1):
    rng = np.random.default_rng(seed)
    m, m2 = rng.random(n) < 0.5, rng.random(n) < 0.3
    m[-1] = True   # the last row, in the ragged word where there is one
    return m, m2


SIZES = [70, 64, 1]
B = 5


@pytest.mark.parametrize("n", SIZES)
def test_one_mask_serves_every_query(no_native, n):
    m, _ = two_masks(n)
    got = ix._marshal_allowed(m, B, n)
    assert got.words == (n + 31) // 32 and got.n_masks == 1
    assert got.moq.dtype == np.int32 and np.array_equal(got.moq, np.zeros(B))
    assert got.host.dtype == np.uint32 and got.host.flags.c_contiguous
    assert np.array_equal(got.host, packed(m, n)[None, :])
    assert got.keep is got.host and ix._addr(got.bits) == got.host.ctypes.data


@pytest.mark.parametrize("n", SIZES)
def test_list_shares_masks_by_identity_only(no_native, n):
    m, m2 = two_masks(n)
    got = ix._marshal_allowed([m, None, m, m2, None], B, n)
    assert got.n_masks == 2 and got.words == (n + 31) // 32
    assert np.array_equal(got.moq, [0, -1, 0, 1, -1])
    assert np.array_equal(got.host, np.stack([packed(m, n), packed(m2, n)]))
    twin = m.copy()   # equal, but another object: its own row
    got = ix._marshal_allowed((m, twin, m, None, twin), B, n)
    assert got.n_masks == 2 and np.array_equal(got.moq, [0, 1, 0, -1, 1])
    assert np.array_equal(got.host, np.stack([packed(m, n), packed(m, n)]))


@pytest.mark.parametrize("n", SIZES)
def test_2d_bool_array_is_one_row_per_query(no_native, n):
    a = np.random.default_rng(2).random((B, n)) < 0.4
    got = ix._marshal_allowed(a, B, n)
    assert got.n_masks == B and np.array_equal(got.moq, np.arange(B))
    assert np.array_equal(got.host, np.stack([packed(r, n) for r in a]))


@pytest.mark.parametrize("n", SIZES)
def test_packed_input_loses_bits_at_and_beyond_n(no_native, n):
    m, _ = two_masks(n)
    words = (n + 31) // 32
    dirty = np.concatenate([packed(m, n), np.full(2, 0xFFFFFFFF, np.uint32)])   # more words than needed
    if n % 32:
        dirty[words - 1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32)
    for given in (dirty, dirty.view(np.int32)):
        got = ix._marshal_allowed(given, B, n)
        assert got.n_masks == 1 and got.host.shape == (1, words)
        assert np.array_equal(got.host[0], packed(m, n))


@pytest.mark.parametrize("n", SIZES)
def test_wrong_mask_count_raises(no_native, n):
    m, m2 = two_masks(n)
    with pytest.raises(ValueError) as e:
        ix._marshal_allowed([m, m2, None, m], B, n)
    assert str(e.value) == "allowed: 4 masks for 5 queries"
    with pytest.raises(ValueError) as e:
        ix._marshal_allowed(np.zeros((4, n), bool), B, n)
    assert str(e.value) == "allowed: 4 masks for 5 queries"


@pytest.mark.parametrize("n", SIZES)
def test_no_mask_at_all_is_a_null_pointer(no_native, n):
    got = ix._marshal_allowed([None] * B, B, n)
    assert got.n_masks == 0 and got.bits is None and ix._addr(got.bits) is None
    assert got.words == (n + 31) // 32 and np.array_equal(got.moq, np.full(B, -1))
    assert ix._NO_MASKS.n_masks == 0 and ix._addr(ix._NO_MASKS.bits) is None and ix._addr(ix._NO_MASKS.moq) is None


def test_cpu_tensor_masks_are_packed_like_arrays():
    n = 70
    m, m2 = two_masks(n)
    got = ix._marshal_allowed([torch.from_numpy(m), None, torch.from_numpy(m2), None, None], B, n)
    assert np.array_equal(got.moq, [0, -1, 1, -1, -1])
    assert np.array_equal(got.host, np.stack([packed(m, n), packed(m2, n)]))
    rows2d = torch.from_numpy(np.stack([m, m2, m, m2, m]))
    got = ix._marshal_allowed(rows2d, B, n)
    assert got.n_masks == B and np.array_equal(got.host, np.stack([packed(r, n) for r in rows2d.numpy()]))


# ---- outputs --------------------------------------------------------------------------------------------------
def test_outputs_allocates_where_the_query_lives(no_native):
    Dn, In = ix._outputs(None, 3, 7, np.zeros((3, D), np.float32))
    assert isinstance(Dn, np.ndarray) and Dn.shape == (3, 7) and Dn.dtype == np.float32 and Dn.flags.c_contiguous
    assert isinstance(In, np.ndarray) and In.shape == (3, 7) and In.dtype == np.int64 and In.flags.c_contiguous


def test_outputs_on_tensors():
    Dt, It = ix._outputs(None, 3, 7, torch.zeros((3, D)))
    assert Dt.shape == (3, 7) and Dt.dtype == torch.float32 and Dt.device.type == "cpu" and Dt.is_contiguous()
    assert It.shape == (3, 7) and It.dtype == torch.int64 and It.device.type == "cpu" and It.is_contiguous()
    good = (torch.empty((3, 7)), torch.empty((3, 7), dtype=torch.int64))
    got = ix._outputs(good, 3, 7, torch.zeros((3, D)))
    assert got[0] is good[0] and got[1] is good[1]
    wide = (torch.empty((3, 14)), torch.empty((3, 14), dtype=torch.int64))
    bad = {"shape_D": (torch.empty((2, 7)), good[1]),
           "shape_I": (good[0], torch.empty((3, 8), dtype=torch.int64)),
           "dtype_D": (torch.empty((3, 7), dtype=torch.float16), good[1]),
           "dtype_I": (good[0], torch.empty((3, 7), dtype=torch.int32)),
           "view_D": (wide[0][:, ::2], good[1]),
           "view_I": (good[0], wide[1][:, ::2])}
    for name, out in bad.items():
        with pytest.raises(ValueError) as e:
            ix._outputs(out, 3, 7, torch.zeros((3, D)))
        assert str(e.value) == OUT_TEXT, name


# ---- error mapper ---------------------------------------------------------------------------------------------
def test_check_maps_ok_and_empty(no_native):
    assert ix._check(_lib.TS_OK) is None
    assert ix._check(_lib.TS_OK, invalid=True) is None
    for invalid in (False, True):
        with pytest.raises(ValueError) as e:
            ix._check(_lib.TS_ERR_EMPTY, invalid=invalid)
        assert str(e.value) == EMPTY_TEXT


def test_addr():
    a = np.zeros(4, np.int64)
    t = torch.zeros(4)
    assert ix._addr(None) is None and ix._addr(a) == a.ctypes.data and ix._addr(t) == t.data_ptr()
    assert np.array_equal(ix._id_array(torch.tensor([[3, 1], [2, 0]])), [3, 1, 2, 0])
    assert ix._id_array([5, 7]).dtype == np.int64 and ix._id_array(np.arange(6)[::2]).flags.c_contiguous
