"""Rows and queries going in, held to the bit-level model of tests/ingest_model.py.

Rows: ``row_den_kernel``, ``relayout_kernel`` and ``reconstruct_kernel`` with the host and device drivers of
``ts_index_add`` / ``ts_index_reconstruct``, read back through ``reconstruct_n``.  Queries: ``qprep_kernel``,
``qprep_f32s_kernel`` and ``q_unit`` / ``build_qimage`` of the one-launch scan, read back through ``scores()`` and
``search()`` on probe corpora whose row i holds one power of two at k = i mod d.  Everything is compared by bits (NaN
as NaN); only the normalisation of general rows is bracketed (``ingest_model.stored_bracket``)."""
import ctypes
import functools

import numpy as np
import pytest

import exact_inputs as ex
import ingest_model as im
from helpers import make_corpus

pytestmark = pytest.mark.gpu

F32 = np.float32
STORE_D = (8, 40, 99, 100, 768, 1536)       # 40: a half group past dim in the vector branch; 99: k0 < dim <= k1; 100: scalar
F32_MAX_D = 1024                            # fp32 storage: 32 queries of d = 1536 do not fit the LDS; the index refuses it
PIECES = (45, 1000, 7, 1)                   # rows per add: row0 falls inside a row block
HOWS = ("host", "dev", "dev+1")             # a host array, an aligned CUDA tensor, one offset by one element
PAIRS = [(i, T) for i in im.INPUTS for T in im.STORAGE]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dims(T, dims=STORE_D):
    """The dimensions of a storage test: d = 1536 becomes 1024, the largest the suite uses, for fp32 storage."""
    return tuple(min(d, F32_MAX_D) if T == "f32" else d for d in dims)


def _ix():
    from tristage_rag_amd import index
    return index


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _bits16(v, dtype):
    v = np.ascontiguousarray(v, dtype=F32)
    if dtype == "f16":
        return v.astype(np.float16).view(np.uint16)
    return (v.view(np.uint32) >> 16).astype(np.uint16)


def _host(v, dtype):
    """float32 values that are numbers of ``dtype`` as a host array of that type (bf16: its bit patterns)."""
    v = np.ascontiguousarray(v, dtype=F32)
    assert im.representable(v, dtype).all()
    if dtype == "f32":
        return v if v.flags.writeable else v.copy()          # (torch.from_numpy wants a writable array)
    return v.astype(np.float16) if dtype == "f16" else _bits16(v, "bf16")


def _dev(v, dtype, offset=False):
    """The same values as a CUDA tensor of ``dtype``, moved by bits; ``offset``: contiguous, but one element into a
    larger buffer, so its address is no multiple of 16."""
    import torch
    h = _host(v, dtype)
    t = torch.from_numpy(h.view(np.int16)).view(torch.bfloat16) if dtype == "bf16" else torch.from_numpy(h)
    if not offset:
        t = t.cuda()
        assert t.data_ptr() % 32 == 0
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    flat = buf[1:]
    flat.copy_(t.reshape(-1))
    out = flat.view(t.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def _give(v, dtype, how):
    return _host(v, dtype) if how == "host" else _dev(v, dtype, offset=how == "dev+1")


def _add_one(idx, x, dtype, normalize):
    if isinstance(x, np.ndarray) and dtype == "bf16":         # numpy has no bfloat16: the library call itself
        from tristage_rag_amd import _lib
        flags = _lib.TS_FLAG_HOST_PTR | (_lib.TS_FLAG_NORMALIZE if normalize else 0)
        _lib.check(idx._lib.ts_index_add(idx._h, x.ctypes.data_as(ctypes.c_void_p), x.shape[0], _lib.TS_BF16, flags, None))
    else:
        idx.add(x, normalize=normalize)


def _add(idx, rows, dtype, how, normalize=False, pieces=PIECES):
    x = _give(rows, dtype, how)
    r, i = 0, 0
    while r < rows.shape[0]:
        c = min(pieces[i % len(pieces)], rows.shape[0] - r)
        _add_one(idx, x[r: r + c], dtype, normalize)
        r, i = r + c, i + 1
    assert idx.ntotal == rows.shape[0]


def _partial_block(rows):
    """The rows, one zero row more where they would end on a row block."""
    return rows if rows.shape[0] % 32 else np.concatenate([rows, np.zeros((1, rows.shape[1]), dtype=F32)])


# ------------------------------------------------------------------------------------------------------- rounding
@pytest.mark.parametrize("in_dtype,T", PAIRS)
def test_rows_are_rounded_once_to_nearest_even(torch_mod, in_dtype, T):
    """Every (input type, storage type) on its catalogue -- every finite pattern, every tie with both float32
    neighbours, the overflow threshold, subnormals, inf and NaN; all patterns of a 16-bit input -- at every d of
    STORE_D, from a host array, an aligned CUDA tensor (the vector branch where d % 8 == 0) and an offset one (the
    scalar branch), added in pieces of 45, 1000, 7 and 1 rows."""
    values = im.rounding_input(in_dtype, T)
    for d in _dims(T):
        rows = _partial_block(im.pack_rows(values, d))
        with np.errstate(over="ignore"):
            want = im.stored(rows, in_dtype, T)
        first = None
        for how in HOWS:
            idx = _ix().FlatIPIndex(d, dtype=T)
            _add(idx, rows, in_dtype, how)
            got = idx.reconstruct_n()
            idx.close()
            im.assert_same_bits(got, want, f"{in_dtype} -> {T} d={d} {how}")
            first = got if first is None else first
            assert im.mismatches(got, first).size == 0


@pytest.mark.parametrize("T", im.STORAGE)
def test_reconstruct_n_returns_the_models_slice(torch_mod, T):
    """Sub-ranges that start and end inside a row block, single rows, the last row, the whole index."""
    for d in (40, 99):
        rows = _partial_block(im.pack_rows(im.catalogue_values("f16" if T == "f32" else T)[:: 7], d))[:1061]
        n = rows.shape[0]
        assert n > 200 and n % 32
        with np.errstate(over="ignore"):
            want = im.stored(rows, "f32", T)
        idx = _ix().FlatIPIndex(d, dtype=T)
        _add(idx, rows, "f32", "dev")
        for i0, c in ((0, n), (0, 1), (45, 100), (33, 1), (31, 2), (63, 66), (n - 1, 1), (n - 40, 40), (n // 2, n - n // 2),
                      (5, 0)):
            got = idx.reconstruct_n(i0, c)
            assert got.shape == (c, d)
            im.assert_same_bits(got, want[i0: i0 + c], f"{T} d={d} reconstruct_n({i0}, {c})")
        im.assert_same_bits(idx.reconstruct_n(17), want[17:], "to the end")
        idx.close()


# ------------------------------------------------------------------------------------------------- normalisation
@functools.lru_cache(maxsize=None)
def _exact_case(d, in_dtype):
    """Class 1 rows and the degenerate rows of one (d, input type), with their exact denominators."""
    rows, N, e = im.exact_norm_rows(150, d, in_dtype, seed=2)
    deg, dden = im.degenerate_rows(d, in_dtype)
    rows, den = np.concatenate([rows[:100], deg, rows[100:]]), np.concatenate([im.exact_den(N[:100], e[:100]), dden,
                                                                              im.exact_den(N[100:], e[100:])])
    rows.setflags(write=False)
    return rows, den


@pytest.mark.parametrize("in_dtype,T", PAIRS)
def test_exact_rows_are_normalised_bit_for_bit(torch_mod, in_dtype, T):
    """Class 1 (integer rows with a perfect-square sum of squares, times 2^e) and the degenerate rows: the stored
    value is round_to(fl32(v / fl32(N 2^e + 1e-8)), T) exactly.  f16 and bf16 input launch row_den_kernel<_Float16>
    and row_den_kernel<__bf16>."""
    for d in _dims(T):
        rows, den = _exact_case(d, in_dtype)
        want = im.stored_exact_norm(rows, den, T)
        assert np.isfinite(want).all()
        for how in HOWS:
            idx = _ix().FlatIPIndex(d, dtype=T)
            _add(idx, rows, in_dtype, how, normalize=True, pieces=(45, 7, 1, 1000))
            got = idx.reconstruct_n()
            idx.close()
            im.assert_same_bits(got, want, f"{in_dtype} -> {T} d={d} {how}")


@pytest.mark.parametrize("in_dtype,T", PAIRS)
def test_general_rows_are_normalised_inside_the_bracket(torch_mod, in_dtype, T):
    """Class 2 (standard normal times 3): each stored element lies between round_to(fl32(v / den_lo), T) and
    round_to(fl32(v / den_hi), T), den_lo / den_hi bracketing the float64 denominator by beta(d); at most 1 % of the
    elements of 16-bit storage have two different ends (test_ingest_model_host.py).  Host and device rows agree."""
    for d in _dims(T, (40, 100, 768, 1536)):
        rows = im.general_rows(300, d, in_dtype)
        first = None
        for how in ("host", "dev"):
            idx = _ix().FlatIPIndex(d, dtype=T)
            _add(idx, rows, in_dtype, how, normalize=True)
            got = idx.reconstruct_n()
            idx.close()
            im.assert_in_bracket(got, rows, T, f"{in_dtype} -> {T} d={d} {how}")
            first = got if first is None else first
            assert im.mismatches(got, first).size == 0
        emu = im.stored_exact_norm(rows, im.emulated_den(rows), T)
        print(f"\n{in_dtype} -> {T} d={d}: {100 * im.undecided_share(rows, T):.2f} % undecided, "
              f"{100 * float((got != emu).mean()):.3f} % differ from the emulation of the kernel's order")


@pytest.mark.parametrize("T", im.STORAGE)
@pytest.mark.parametrize("how", ["host", "dev"])
def test_update_rows_normalises_as_add_does(torch_mod, T, how):
    d = 100
    rows, den = _exact_case(d, "f32")
    base = im.pack_rows(im.catalogue_values("bf16")[:: 5], d)[:400]
    assert base.shape[0] == 400
    base = np.where(np.isfinite(base), base, F32(1))
    ids = np.random.default_rng(4).permutation(400)[: rows.shape[0]]
    idx = _ix().FlatIPIndex(d, dtype=T)
    idx.add(base)
    idx.update_rows(ids, _give(rows, "f32", how), normalize=True)
    with np.errstate(over="ignore"):
        want = im.stored(base, "f32", T)
    want[ids] = im.stored_exact_norm(rows, den, T)
    im.assert_same_bits(idx.reconstruct_n(), want, f"{T} update_rows {how}")
    idx.close()


@pytest.mark.parametrize("T", ["f16", "bf16"])
@pytest.mark.parametrize("in_dtype", im.INPUTS)
def test_ivf_add_normalises_as_the_flat_index_does(torch_mod, T, in_dtype):
    d = 96
    rows, den = _exact_case(d, in_dtype)
    ivf = _ix().IVFFlatIndex(d, 8, dtype=T, nprobe=8)
    ivf.set_centroids(make_corpus(8, d, seed=3, dtype=T))
    ivf.add(_dev(rows, in_dtype), normalize=True)
    im.assert_same_bits(ivf.reconstruct_n(), im.stored_exact_norm(rows, den, T), f"IVF {in_dtype} -> {T}")
    ivf.close()


@pytest.mark.parametrize("in_dtype", im.INPUTS)
@pytest.mark.parametrize("how", ["host", "dev"])
def test_fp8_index_quantises_the_exact_quotient(torch_mod, in_dtype, how):
    """The e4m3 index normalises with the same row_den_kernel: its bytes are the reference quantiser's of fl32(v / den)."""
    ix = _ix()
    for d in (40, 100, 768):
        rows, den = _exact_case(d, in_dtype)
        with np.errstate(all="ignore"):
            quot = (rows / den.reshape(-1, 1)).astype(F32)
        want = ix.decode_rows_e4m3_fixed(ix.quantize_rows_e4m3_fixed_reference(quot, 8), 8)
        idx = ix.FlatIPIndex(d, dtype="fp8", fp8_scale_log2=8)
        _add(idx, rows, in_dtype, how, normalize=True)
        im.assert_same_bits(idx.reconstruct_n(), want, f"fp8 {in_dtype} d={d} {how}")
        idx.close()


# ------------------------------------------------------------------------------------------------ host chunk loops
def _chunk_dim(T):
    """The first of ingest_model.CHUNK_D the flat index takes; only its refusal of a dimension counts as "not taken"."""
    from tristage_rag_amd import _lib
    for d in im.CHUNK_D:
        try:
            _ix().FlatIPIndex(d, dtype=T).close()
            return d
        except _lib.TriStageNativeError as e:
            if e.code != _lib.TS_ERR_UNSUPPORTED:
                raise
    pytest.skip(f"the flat index refuses d = {im.CHUNK_D} for {T} storage: {_lib.last_error()}")


def test_host_chunk_loops_advance_through_the_rows(torch_mod):
    """float32 host rows at d = 4096, or at 2176 where 4096 is refused (ingest_model.CHUNK_D), chunk + 33 of them by the drivers' rule (64 MiB of
    staging): ts_index_add and ts_index_reconstruct both run a second, partial chunk.  The stored rows are read back
    in one launch too (a device destination), so a fault is pinned to one loop."""
    torch = torch_mod
    from tristage_rag_amd import _lib
    T = "f16"
    d = _chunk_dim(T)
    chunk = im.chunk_rows(d)
    n = chunk + 33
    assert len(range(0, n, chunk)) == 2
    print(f"\nchunk loops: d={d}, {n} rows of {4 * d} bytes, chunks of {chunk}")
    rows = np.random.default_rng(9).standard_normal((n, d), dtype=F32)
    want = im.round_to(rows, T)
    idx = _ix().FlatIPIndex(d, dtype=T)
    idx.add(rows)
    out = torch.empty((n, d), dtype=torch.float32, device="cuda")
    _lib.check(idx._lib.ts_index_reconstruct(idx._h, 0, n, ctypes.c_void_p(out.data_ptr()), 0, None))
    torch.cuda.synchronize()
    im.assert_same_bits(out.cpu().numpy(), want, f"d={d}: rows stored by the chunked add")
    del out
    im.assert_same_bits(idx.reconstruct_n(), want, f"d={d}: chunked reconstruct")
    im.assert_same_bits(idx.reconstruct_n(chunk - 5, 38), want[chunk - 5:], "a range across the chunk boundary")
    idx.close()


# ---------------------------------------------------------------------------------- query images through scores()
SCORE_B = (1, 31, 33, 64, 65)
SCORE_CASES = [(T, d) for T in im.STORAGE for d in (40, 99, 100, 768)] + [("f32", 600)]


@pytest.mark.parametrize("T,d", SCORE_CASES)
def test_scores_read_back_the_rounded_queries(torch_mod, T, d):
    """scores() on a probe corpus is round_to(q, T) times the row's power of two, bit for bit: float32, float16 and
    bfloat16 queries from the edge catalogue (finite, in range), as aligned and as offset CUDA tensors; scores() turns
    every host array into float32, so a host array is given for the float32 queries only.  f32 storage at d = 600 and
    768 is the bf16x3 split (qprep_f32s_kernel, its __bf16 instantiation included)."""
    n = d + 37
    corpus, k, scale = im.probe_corpus(n, d)
    idx = _ix().FlatIPIndex(d, dtype=T)
    idx.add(_dev(corpus, T))
    for in_dtype in im.INPUTS:
        q = im.probe_queries(max(SCORE_B), d, in_dtype, T)
        want = im.probe_scores(q, T, k, scale).astype(F32)
        assert np.array_equal(want.astype(np.float64), im.probe_scores(q, T, k, scale))
        for B in SCORE_B:
            for how in (HOWS if in_dtype == "f32" else HOWS[1:]):
                x = q[:B].copy() if how == "host" else _dev(q[:B], in_dtype, offset=how == "dev+1")
                got = _np(idx.scores(x))
                im.assert_same_bits(got, want[:B], f"{in_dtype} queries -> {T} d={d} B={B} {how}")
    idx.close()


# ------------------------------------------------------------------------- query images on every path that builds one
PATH_CASES = [("f16", 128), ("f16", 99), ("bf16", 128), ("bf16", 99), ("f32", 128), ("f32", 99)]
PATH_K = (1, 100)


@functools.lru_cache(maxsize=2)
def _probe(n, d):
    c, k, scale = im.probe_corpus(n, d)
    c.setflags(write=False)
    return c, k, scale


def _queries(B, d, T):
    """float32 queries from T's catalogue and the same queries already rounded to T."""
    q = im.probe_queries(B, d, "f32", T, seed=7)
    return q, im.round_to(q, T)


def _check(got, want, what):
    D, I = _np(got[0]), _np(got[1])
    assert np.array_equal(I, want[1]), f"{what}: ids differ first at {np.argwhere(I != want[1])[:1].tolist()}"
    im.assert_same_bits(D, want[0], what)


def _same(a, b, what):
    assert np.array_equal(_np(a[1]), _np(b[1])), what
    im.assert_same_bits(_np(a[0]), _np(b[0]), what)


@pytest.mark.parametrize("T,d", PATH_CASES)
def test_search_paths_round_their_queries(torch_mod, T, d):
    """dense, classic, masked and range searches over a probe corpus of N_FILTER rows: float32
    catalogue queries must give the model's top-k, and exactly what the same search gives for queries already rounded
    to the storage type."""
    torch = torch_mod
    n = ex.N_FILTER
    corpus, kk, scale = _probe(n, d)
    idx = _ix().FlatIPIndex(d, dtype=T)
    idx.add(_dev(corpus, T))
    q, rq = _queries(200, d, T)
    tq, trq = _dev(q, "f32"), _dev(rq, T)
    want = im.probe_topk(q, T, kk, scale, max(PATH_K))
    for k in PATH_K:
        w64 = (want[0][:64, :k], want[1][:64, :k])
        for name, kw in (("dense", dict(exact_dense=True)), ("classic", dict(classic=True))):
            got, pre = idx.search(tq[:64], k, **kw), idx.search(trq[:64], k, **kw)
            assert idx.last_search_info()["path"] == ("dense" if name == "dense" else "filter"), idx.last_search_info()
            _check(got, w64, f"{name} k={k}")
            _same(got, pre, f"{name} k={k}: float32 against rounded queries")
        _check(idx.search(q[:64], k, classic=True), w64, f"host queries k={k}")
        assert idx.last_search_info()["path"] == "filter", idx.last_search_info()
        if T != "f32":                                       # the masked scan is a 16-bit kernel
            mask = np.random.default_rng(8).random(n) < 0.5
            got, pre = idx.search(tq[:64], k, allowed=mask), idx.search(trq[:64], k, allowed=mask)
            info = idx.last_filter_info()
            assert info["filter_passes"] == 1 and info["dense_passes"] == 0, info
            wm = im.probe_topk(q[:64], T, kk, scale, k, allowed=mask)
            _check(got, wm, f"allowed k={k}")
            _same(got, pre, f"allowed k={k}: float32 against rounded queries")
    # range search: everything at or above each query's 100th best score, in search order
    s = im.probe_scores(q[:33], T, kk, scale)
    radius = want[0][:33, -1]
    res = []
    for x in (tq, trq):
        res.append(idx.range_search(x[:33], radius, sort=True))
        info = idx.last_range_info()
        assert info["filter_passes"] == 1 and info["dense_redo"] == 0, info
    lims, D, I = (_np(a) for a in res[0])
    for b in range(33):
        keep = np.flatnonzero(s[b] >= float(radius[b]))
        order = keep[np.argsort(-s[b][keep], kind="stable")]
        assert np.array_equal(I[lims[b]: lims[b + 1]], order), f"range search query {b}"
        im.assert_same_bits(D[lims[b]: lims[b + 1]], s[b][order].astype(F32), f"range search query {b}")
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(_np(a).view(np.uint8), _np(b).view(np.uint8)), "range search: float32 against rounded queries"
    idx.close()


# The sample that sets a pass's thresholds takes every (nblk / 256)-th row block.  At d = 128 and N_FILTER rows that is
# every 128th row: it sees dimensions 0 .. 31 only, the thresholds come out low, and at k = 100 the library redoes the
# tickets densely (correct, but then the output no longer shows the coalesced image).  There k = 1 is held to "nothing
# redone", and the same corpus continued to 8192 more rows (a stride of 160 rows, which walks every dimension) is held
# to it at both k.
COALESCE_CASES = [(T, d, n) for T in ("f16", "bf16") for d, n in ((99, ex.N_FILTER), (128, ex.N_FILTER),
                                                                  (128, ex.N_FILTER + 8192))]
MAY_REDO = {(128, ex.N_FILTER): (100,)}


@pytest.mark.parametrize("T,d,n", COALESCE_CASES)
def test_coalesced_passes_round_their_queries(torch_mod, T, d, n):
    """Asynchronous batches of 200 queries (tickets of 128 and 72: seven groups of 32 that share corpus passes, the
    groups' images built from the ticket's queries at q0 = 32, 64, 96).  Nothing may be redone, so what is compared is
    what the coalesced passes wrote."""
    torch = torch_mod
    corpus, kk, scale = _probe(n, d)
    idx = _ix().FlatIPIndex(d, dtype=T)
    idx.add(_dev(corpus, T))
    q, rq = _queries(200, d, T)
    tq, trq = _dev(q, "f32"), _dev(rq, T)
    want = im.probe_topk(q, T, kk, scale, max(PATH_K))
    idx.classic_filter, idx.coalesce = True, True
    strict = 0
    for k in PATH_K:
        outs = []
        for x in (tq, trq):
            idx.set_profiling(True, every=1)
            idx.timings(reset=True)
            o = idx.search(x, k, async_=True)
            redone = idx.finish()
            torch.cuda.synchronize()
            assert idx.timings(reset=True)["filter_scan"][1] >= 2      # seven groups: at least two shared passes
            idx.set_profiling(False)
            if k not in MAY_REDO.get((d, n), ()):
                assert redone == [], f"k={k}: tickets {redone} were redone densely"
                assert idx.last_search_info()["path"] == "filter"
                strict += 1
            outs.append(o)
        _check(outs[0], (want[0][:, :k], want[1][:, :k]), f"coalesced k={k}")
        _same(outs[0], outs[1], f"coalesced k={k}: float32 against rounded queries")
    assert strict >= 2
    idx.close()


@pytest.mark.parametrize("T,d", PATH_CASES)
def test_one_launch_scan_rounds_its_queries(torch_mod, T, d):
    """fused_kernel builds its own query image (q_unit): aligned queries take its vector branch where d % 8 == 0,
    offset ones the scalar branch."""
    torch = torch_mod
    n = ex.one_launch_rows(torch.cuda.get_device_properties(0).multi_processor_count)
    corpus, kk, scale = _probe(n, d)
    idx = _ix().FlatIPIndex(d, dtype=T)
    idx.add(_dev(corpus, T))
    q, rq = _queries(64, d, T)
    want = im.probe_topk(q, T, kk, scale, max(PATH_K))
    for k in PATH_K:
        outs = []
        for x, dt in ((q, "f32"), (rq, T)):
            for offset in (False, True):
                outs.append(idx.search(_dev(x, dt, offset=offset), k, one_launch=True))
                info = idx.last_search_info()
                assert info["path"] == "filter" and info["one_launch"], info
        _check(outs[0], (want[0][:, :k], want[1][:, :k]), f"one launch k={k}")
        for o in outs[1:]:
            _same(outs[0], o, f"one launch k={k}: aligned / offset, float32 / rounded queries")
    idx.close()


@pytest.mark.parametrize("T,d", [c for c in PATH_CASES if c[0] != "f32"])
def test_ivf_search_rounds_its_queries(torch_mod, T, d):
    n = ex.N_FILTER
    corpus, kk, scale = _probe(n, d)
    ivf = _ix().IVFFlatIndex(d, 8, dtype=T, nprobe=8)
    ivf.set_centroids(make_corpus(8, d, seed=3, dtype=T))
    ivf.add(_dev(corpus, T))
    q, rq = (x[:64] for x in _queries(200, d, T))
    want = im.probe_topk(q, T, kk, scale, max(PATH_K))
    for k in PATH_K:
        got, pre = ivf.search(_dev(q, "f32"), k, nprobe=8), ivf.search(_dev(rq, T), k, nprobe=8)
        info = ivf.last_search_info()
        # one pass of 64 queries through the IVF filter scan.  At d = 99 nothing is redone; at d = 128 the probe corpus's
        # period meets the threshold sample's stride (see COALESCE_CASES) and the pass may be redone, which in the IVF
        # index scores the same query image again (ts_ivf.hip keeps h->qimg for its dense redo)
        assert info["passes"] == 1 and info["filter_passes"] == 1 and info["redone"] <= (1 if d == 128 else 0), info
        _check(got, (want[0][:, :k], want[1][:, :k]), f"IVF k={k}")
        _same(got, pre, f"IVF k={k}: float32 against rounded queries")
    ivf.close()


@pytest.mark.parametrize("d", [128, 99])
def test_fp8_index_rounds_its_queries_as_its_bf16_mirror(torch_mod, d):
    """An e4m3 index scores a bf16 query image: on the probe corpus (powers of two, exact in e4m3) it must return what
    the bf16 index of the same rows returns, which is the model's top-k for bf16 storage."""
    n = ex.N_FILTER
    corpus, kk, scale = _probe(n, d)
    ix = _ix()
    idx, mirror = ix.FlatIPIndex(d, dtype="fp8", fp8_scale_log2=8), ix.FlatIPIndex(d, dtype="bf16")
    idx.add(_dev(corpus, "f32"))
    mirror.add(_dev(corpus, "bf16"))
    im.assert_same_bits(idx.reconstruct_n(), corpus, "the probe corpus is exact in e4m3")
    q, rq = _queries(64, d, "bf16")
    want = im.probe_topk(q, "bf16", kk, scale, max(PATH_K))
    for k in PATH_K:
        got, pre, mir = idx.search(_dev(q, "f32"), k), idx.search(_dev(rq, "bf16"), k), mirror.search(_dev(q, "f32"), k)
        assert idx.last_search_info()["path"] == "filter", idx.last_search_info()
        _check(got, (want[0][:, :k], want[1][:, :k]), f"fp8 k={k}")
        _same(got, pre, f"fp8 k={k}: float32 against rounded queries")
        _same(got, mir, f"fp8 k={k}: against the bf16 mirror")
    idx.close()
    mirror.close()
