"""FlatIPIndex — the object that stands where the reference keeps its FAISS index.

Reference seam: ``Stage1Retriever.faiss_index`` (reference
src/stage1_retriever.py:126), built by ``faiss.IndexFlatIP(d)`` /
``IndexIVFFlat`` (:256-283) and used through ``.add`` (:270,277,313),
``.search`` (:380), ``.ntotal``.  This class keeps that duck type
(``add``, ``search``, ``ntotal``, ``d``, ``reset``, ``reconstruct_n``) on top of
the C ABI of libtristage.so; the search is always exact (FAISS ``IndexFlatIP``
semantics — the reference's IVF variant above 1000 rows is an approximation of
this result).

Inputs may be numpy arrays (host pointers, FAISS style) or torch tensors on the
index's GPU (device pointers, no copies).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np

from . import _lib

_NP_DTYPES = {np.dtype(np.float32): _lib.TS_F32, np.dtype(np.float16): _lib.TS_F16}
_NAME_TO_DTYPE = {"f32": _lib.TS_F32, "fp32": _lib.TS_F32, "float32": _lib.TS_F32,
                  "f16": _lib.TS_F16, "fp16": _lib.TS_F16, "float16": _lib.TS_F16,
                  "bf16": _lib.TS_BF16, "bfloat16": _lib.TS_BF16,
                  "fp8": _lib.TS_FP8_E4M3, "e4m3": _lib.TS_FP8_E4M3, "float8_e4m3fn": _lib.TS_FP8_E4M3,
                  "fp4": _lib.TS_MXFP4_E2M1, "mxfp4": _lib.TS_MXFP4_E2M1, "e2m1": _lib.TS_MXFP4_E2M1}
_DTYPE_NAME = {_lib.TS_F32: "f32", _lib.TS_F16: "f16", _lib.TS_BF16: "bf16", _lib.TS_FP8_E4M3: "fp8",
               _lib.TS_MXFP4_E2M1: "fp4"}
FP4_INDEX_MAX_D = 2048   # an fp4 index's query image is a bf16 image too, and a lane keeps at most 32 scale bytes
FP8_INDEX_MAX_D = 2048   # an e4m3 index's query image is a bf16 image: 32 queries of it fit the LDS up to here


def _torch():
    import torch
    return torch


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _tensor_dtype(t) -> int:
    torch = _torch()
    if t.dtype == torch.float32:
        return _lib.TS_F32
    if t.dtype == torch.float16:
        return _lib.TS_F16
    if t.dtype == torch.bfloat16:
        return _lib.TS_BF16
    raise TypeError(f"unsupported tensor dtype {t.dtype}")


def pack_allowed(mask, n: int) -> np.ndarray:
    """An allow mask over ``n`` rows -> packed uint32 words (host): bit ``r % 32`` of word ``r // 32`` set
    means row ``r`` is allowed (the layout of ``ts_index_search_filtered``).  ``mask`` is a bool array /
    tensor of length ``n``, or an already packed uint32 array of at least ``ceil(n / 32)`` words."""
    if _is_tensor(mask):
        mask = mask.detach().cpu().numpy()
    m = np.asarray(mask)
    words = (int(n) + 31) // 32
    if m.dtype == np.bool_:
        if m.ndim != 1 or m.shape[0] != n:
            raise ValueError(f"a bool allow mask must have one entry per row ({n}), got shape {m.shape}")
        b = np.packbits(m, bitorder="little")
        out = np.zeros(words * 4, dtype=np.uint8)
        out[: b.shape[0]] = b
        return out.view("<u4").astype(np.uint32)
    if m.dtype in (np.uint32, np.int32):
        if m.ndim != 1 or m.shape[0] < words:
            raise ValueError(f"a packed allow mask needs >= {words} uint32 words, got shape {m.shape}")
        w = np.ascontiguousarray(m[:words]).view(np.uint32).copy()
        if n % 32:   # bits at or beyond n are ignored by the library; cleared here too for a canonical form
            w[-1] &= np.uint32((1 << (n % 32)) - 1)
        return w
    raise TypeError(f"allow mask: expected a bool array or packed uint32 words, got dtype {m.dtype}")


def _stream_ptr(device_index: int) -> int:
    torch = _torch()
    return int(torch.cuda.current_stream(device_index).cuda_stream)


def wide_pass_flags(wide_passes) -> int:
    """Search flags of FlatIPIndex.wide_passes: "auto" (the library's policy), True / False (forced on / off)."""
    if wide_passes is True:
        return _lib.TS_FLAG_WIDE_PASSES
    if wide_passes is False:
        return _lib.TS_FLAG_NO_WIDE_PASSES
    if isinstance(wide_passes, str) and wide_passes == "auto":
        return 0
    raise ValueError(f"wide_passes must be 'auto', True or False, not {wide_passes!r}")


def stationary_pass_flags(stationary_passes) -> int:
    """Search flags of FlatIPIndex.stationary_passes: "auto" (the library's policy), True / False (forced on / off)."""
    if stationary_passes is True:
        return _lib.TS_FLAG_STATIONARY_PASSES
    if stationary_passes is False:
        return _lib.TS_FLAG_NO_STATIONARY_PASSES
    if isinstance(stationary_passes, str) and stationary_passes == "auto":
        return 0
    raise ValueError(f"stationary_passes must be 'auto', True or False, not {stationary_passes!r}")


def pass_prologue_flags(pass_prologue) -> int:
    """Search flags of FlatIPIndex.pass_prologue: "auto" (the library's policy), True / False (forced on / off)."""
    if pass_prologue is True:
        return _lib.TS_FLAG_PASS_PROLOGUE
    if pass_prologue is False:
        return _lib.TS_FLAG_NO_PASS_PROLOGUE
    if isinstance(pass_prologue, str) and pass_prologue == "auto":
        return 0
    raise ValueError(f"pass_prologue must be 'auto', True or False, not {pass_prologue!r}")


def _addr(x) -> Optional[int]:
    """The address of a numpy array or a tensor; None (a NULL pointer) for None.  Every ``c_void_p`` parameter of
    ``_lib.SIGNATURES`` takes it as it is.  Call it in the statement of the library call that consumes the address, so
    that the object outlives the call."""
    if x is None:
        return None
    return x.data_ptr() if _is_tensor(x) else x.ctypes.data


def _raise_empty():
    # same exception type and text as reference src/stage1_retriever.py:370-371
    raise ValueError("No documents indexed. Call add_documents() first.")


def _check(code: int, invalid: bool = False) -> None:
    """A library return code: TS_ERR_EMPTY is the reference's ``ValueError``; with ``invalid``, a refused argument
    (TS_ERR_INVALID, nothing done) is a ``ValueError`` carrying the library's message; the rest is ``_lib.check``."""
    if code == _lib.TS_ERR_EMPTY:
        _raise_empty()
    if invalid and code == _lib.TS_ERR_INVALID:
        raise ValueError(_lib.last_error())
    _lib.check(code)


# ---- arguments -> what a library call takes -------------------------------------------------------------------
# Queries and rows come in under one of two policies, and an entry point keeps the one it has: it decides the call.
#   host pointers (_host_query): a CUDA tensor is read in place on the current stream; anything else stays on the
#     host and the library copies it itself (TS_FLAG_HOST_PTR, the NULL stream).
#   upload (_device_query): whatever is not on the index's GPU goes there through torch first.
# Both return (x, dtype code, B, on_gpu): the object to pass (and keep alive), TS_F32 / TS_F16 / TS_BF16, its rows, and
# whether the input was a CUDA tensor (then the results are tensors too).

def _bad_shape(n, d: int, what: str, shape):
    raise ValueError(f"expected [{n}, {d}] {what}, got {tuple(shape)}")


def _host_query(x, d: int, what: str = "queries", n="B", device: Optional[int] = None):
    """Host-pointer policy.  CUDA tensor: made contiguous, used in place (``device``: it must live there).  CPU tensor:
    ``float().numpy()``.  numpy: f32 / f16 kept, any other dtype to f32, made contiguous.  ``n``: the word for the row
    count in the message, or the count itself, which the input must then have."""
    if _is_tensor(x) and not x.is_cuda:
        x = x.detach().float().numpy()
    on_gpu = _is_tensor(x)
    if not on_gpu:
        x = np.ascontiguousarray(x)
        if x.dtype not in _NP_DTYPES:
            x = x.astype(np.float32)
    if x.ndim != 2 or x.shape[1] != d or (isinstance(n, int) and x.shape[0] != n):
        _bad_shape(n, d, what, x.shape)
    if on_gpu:
        if device is not None and x.device.index != device:
            raise ValueError(f"{what} live on a different GPU than the index")
        x = x.contiguous()
    return x, (_tensor_dtype(x) if on_gpu else _NP_DTYPES[x.dtype]), int(x.shape[0]), on_gpu


def _device_query(x, d: int, device: int, what: str = "queries", n="B"):
    """Upload policy: a contiguous f32 / f16 / bf16 tensor on GPU ``device`` (any other dtype goes to f32)."""
    torch = _torch()
    on_gpu = _is_tensor(x) and x.is_cuda
    if not _is_tensor(x):
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x if x.dtype in _NP_DTYPES else x.astype(np.float32))
    if x.dim() != 2 or x.shape[1] != d or (isinstance(n, int) and x.shape[0] != n):
        _bad_shape(n, d, what, x.shape)
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        x = x.float()
    if not x.is_cuda or x.device.index != device:
        x = x.to(torch.device("cuda", device))
    x = x.contiguous()
    return x, _tensor_dtype(x), int(x.shape[0]), on_gpu


def _outputs(out, B: int, k: int, like):
    """``(D, I)``, float32 / int64 ``[B, k]``: new ones where ``like`` lives (a tensor's device, or numpy), or the
    caller's ``out`` pair, checked."""
    if out is not None:
        torch = _torch()
        D, I = out
        if (D.shape != (B, k) or I.shape != (B, k) or D.dtype != torch.float32 or
                I.dtype != torch.int64 or not D.is_contiguous() or not I.is_contiguous()):
            raise ValueError("out must be contiguous (float32[B,k], int64[B,k]) CUDA tensors")
        return D, I
    if _is_tensor(like):
        torch = _torch()
        return (torch.empty((B, k), dtype=torch.float32, device=like.device),
                torch.empty((B, k), dtype=torch.int64, device=like.device))
    return np.empty((B, k), dtype=np.float32), np.empty((B, k), dtype=np.int64)


def _to_host(x):
    return x.detach().cpu().numpy() if _is_tensor(x) else x


def _id_array(ids) -> np.ndarray:
    """Row ids in any form -> a contiguous flat int64 array on the host."""
    return np.ascontiguousarray(np.asarray(_to_host(ids), dtype=np.int64).reshape(-1))


class _Masks(NamedTuple):
    """``allowed``, marshalled (:func:`_marshal_allowed`)."""
    keep: object                  # the packed masks [max(n_masks, 1), words] the call reads: device tensor or host array
    words: int                    # ceil(ntotal / 32)
    n_masks: int
    moq: Optional[np.ndarray]     # mask_of_query, int32 [B]; -1: the query is unfiltered
    host: Optional[np.ndarray]    # the masks on the host as uint32, when they were packed there

    @property
    def bits(self):
        """No masks at all: a NULL pointer."""
        return self.keep if self.n_masks else None


_NO_MASKS = _Masks(None, 0, 0, None, None)


def _allowed_items(allowed, B: int) -> list:
    """``allowed`` -> one entry per query: a list, a tuple or the rows of a 2-D array are per query; anything else
    serves them all (one object, so one mask)."""
    if not isinstance(allowed, (list, tuple)) and getattr(allowed, "ndim", 1) != 2:
        return [allowed] * B
    if len(allowed) != B:
        raise ValueError(f"allowed: {len(allowed)} masks for {B} queries")
    return list(allowed)


def _marshal_allowed(allowed, B: int, n: int, device=None) -> _Masks:
    """``allowed`` of a search of ``B`` queries over ``n`` rows, for a call that reads the masks on ``device`` (a torch
    device) or on the host (None; needs neither torch nor the library).  The mask objects of a list are told apart by
    identity: one object, one packed mask.  Masks that all are packed int32 tensors on ``device`` already are used
    there (a single contiguous one in place); otherwise all are packed on the host (:func:`pack_allowed`) and uploaded."""
    words = (n + 31) // 32
    uniq, seen = [], {}
    moq = np.full(B, -1, dtype=np.int32)
    for qi, a in enumerate(_allowed_items(allowed, B)):
        if a is not None:
            if id(a) not in seen:
                seen[id(a)] = len(uniq)
                uniq.append(a)
            moq[qi] = seen[id(a)]
    if device is not None and uniq and all(
            _is_tensor(a) and a.is_cuda and a.dtype == _torch().int32 and a.dim() == 1 and a.shape[0] >= words
            and a.device == device for a in uniq):   # (Stage1Retriever's filter cache, tools/filter_probe.py)
        host, rows = None, [a[:words] for a in uniq]
        keep = rows[0].view(1, -1) if len(rows) == 1 and rows[0].is_contiguous() else _torch().stack(rows).contiguous()
    else:
        host = np.ascontiguousarray(np.stack([pack_allowed(a, n) for a in uniq]) if uniq
                                    else np.zeros((1, max(words, 1)), dtype=np.uint32))
        # the device copy lives as long as the _Masks: an asynchronous search keeps it until finish()
        keep = host if device is None else _torch().from_numpy(host.view(np.int32)).to(device)
    return _Masks(keep, words, len(uniq), moq, host)


def _update_call(fn, handle, ids: np.ndarray, x, dtype: int, flags: int, stream) -> None:
    """ts_index_update / ts_update_ivf: a refused id (TS_ERR_INVALID, nothing written) is a ``ValueError``."""
    _check(fn(handle, _addr(ids), int(ids.shape[0]), _addr(x), dtype, flags, stream), invalid=True)


MMR_MAX_FETCH = 1024   # candidates per query of mmr(): the greedy kernel runs one thread per candidate


def mmr_default_fetch_k(k: int) -> int:
    """Candidates ``search_mmr`` fetches when ``fetch_k`` is not given."""
    return min(MMR_MAX_FETCH, max(4 * int(k), 20))


def mmr_check(k, fetch_k, lambda_mult):
    """The argument checks of ``mmr`` / ``search_mmr`` (``ValueError``), made before anything is launched."""
    lam = float(lambda_mult)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_mult must be in [0, 1], got {lambda_mult!r}")
    k, fetch_k = int(k), int(fetch_k)
    if k < 1:
        raise ValueError("k must be positive")
    if k > fetch_k:
        raise ValueError(f"k={k} exceeds fetch_k={fetch_k}: MMR picks k out of fetch_k candidates")
    if fetch_k > MMR_MAX_FETCH:
        raise ValueError(f"fetch_k={fetch_k} exceeds {MMR_MAX_FETCH}")
    return k, fetch_k, lam


def _mmr_call(ix, entry: str, ids, relevance, k, lambda_mult):
    """ts_index_mmr / ts_mmr_ivf (``entry``) on the index ``ix``: CUDA tensors in -> tensors out, enqueued on the current
    stream; anything else goes through host pointers and comes back as numpy.  The arguments are checked first."""
    on_gpu = _is_tensor(ids) and ids.is_cuda
    if on_gpu:
        torch = _torch()
        ids = ids.to(torch.int64).contiguous()
        rel = torch.as_tensor(relevance, device=ids.device).to(torch.float32).contiguous()
    else:
        ids = np.ascontiguousarray(_to_host(ids), dtype=np.int64)
        rel = np.ascontiguousarray(_to_host(relevance), dtype=np.float32)
    if ids.ndim != 2 or tuple(rel.shape) != tuple(ids.shape):
        raise ValueError(f"expected ids and relevance of one shape [B, fetch_k], got {tuple(ids.shape)} and "
                         f"{tuple(rel.shape)}")
    k, C, lam = mmr_check(k, ids.shape[1], lambda_mult)
    if on_gpu and ids.device.index != ix.device:
        raise ValueError("the candidates live on a different GPU than the index")
    B = ids.shape[0]
    D, I = _outputs(None, B, k, ids)
    _check(getattr(ix._lib, entry)(ix._h, _addr(ids), _addr(rel), B, C, k, lam, _addr(D), _addr(I),
                                   0 if on_gpu else _lib.TS_FLAG_HOST_PTR, _stream_ptr(ix.device) if on_gpu else None),
           invalid=True)
    return D, I


FUNNEL_MAX_FETCH = 16384   # shortlist entries per query of the funnel: the select kernels hold 16384 keys in LDS


def funnel_default_fetch_k(k: int) -> int:
    """The shortlist ``search_funnel`` fetches when ``fetch_k`` is not given (at most 2048: the prefix pass's filter path)."""
    return min(2048, max(8 * int(k), 128))


def funnel_check(d: int, dims, k, fetch_k=None):
    """The argument checks of ``search_prefix`` / ``search_funnel`` (``ValueError``), made before anything is launched:
    ``dims`` a multiple of 128 in [128, d), ``1 <= k (<= fetch_k) <= 16384``.  Returns the ints."""
    if isinstance(dims, bool) or int(dims) != dims:
        raise ValueError(f"dims must be an integer, got {dims!r}")
    dims, k = int(dims), int(k)
    if dims % 128 != 0 or not 128 <= dims < int(d):
        raise ValueError(f"dims={dims} must be a multiple of 128 in [128, {int(d)})")
    if k < 1:
        raise ValueError("k must be positive")
    if fetch_k is None:
        if k > FUNNEL_MAX_FETCH:
            raise ValueError(f"k={k} exceeds {FUNNEL_MAX_FETCH}")
        return k, dims
    fetch_k = int(fetch_k)
    if fetch_k < k:
        raise ValueError(f"fetch_k={fetch_k} is below k={k}: the rescore picks k out of fetch_k candidates")
    if fetch_k > FUNNEL_MAX_FETCH:
        raise ValueError(f"fetch_k={fetch_k} exceeds {FUNNEL_MAX_FETCH}")
    return k, dims, fetch_k


BIAS_MAX_K = 16384   # results per query of search_biased(): the select kernels hold 16384 keys in LDS


def bias_check_k(k) -> int:
    """The ``k`` of ``search_biased`` (``ValueError``), checked before anything is launched."""
    k = int(k)
    if not 1 <= k <= BIAS_MAX_K:
        raise ValueError(f"k={k} must be in 1 .. {BIAS_MAX_K}")
    return k


def _marshal_bias(bias, n: int, device, check_finite: bool):
    """``bias`` of a ``search_biased`` over ``n`` rows, for a call that reads it on ``device`` (a torch device) or on the
    host (None): one float32 entry per row, contiguous (16-byte aligned on the device).  A wrong length is a
    ``ValueError``; so is a NaN or an infinity, on the device with ``check_finite`` and on the host always (the library
    refuses such a host array itself)."""
    shape = tuple(bias.shape) if hasattr(bias, "shape") else (len(bias),)
    if shape != (n,):
        raise ValueError(f"bias must hold one entry per row, [{n}], got {shape}")
    if device is None:
        b = np.ascontiguousarray(_to_host(bias), dtype=np.float32)
        if not np.isfinite(b).all():
            raise ValueError("bias holds a NaN or an infinity (every entry must be finite); a bias that goes through the "
                             "host is always checked, check_finite=False applies to CUDA tensors only")
        return b
    else:
        torch = _torch()
        b = bias if _is_tensor(bias) else torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float32))
        b = b.to(device=device, dtype=torch.float32).contiguous()
        if b.data_ptr() % 16:
            b = b.clone()
        if check_finite and not bool(torch.isfinite(b).all()):
            raise ValueError("bias holds a NaN or an infinity (every entry must be finite)")
        return b


GROUP_MAX_FETCH = 16384   # entries per query of group_topk(): one workgroup sorts the list in LDS (the select limit)


def group_default_fetch_k(k: int, group_size: int = 1) -> int:
    """Candidates ``search_grouped`` fetches in its first round when ``fetch_k`` is not given."""
    return min(GROUP_MAX_FETCH, max(4 * int(k) * int(group_size), 64))


def group_check(k, group_size, ncand):
    """The argument checks of ``group_topk`` / ``search_grouped`` (``ValueError``), made before anything is launched."""
    k, group_size, ncand = int(k), int(group_size), int(ncand)
    if k < 1:
        raise ValueError("k must be positive")
    if group_size < 1:
        raise ValueError("group_size must be positive")
    if k * group_size > GROUP_MAX_FETCH:
        raise ValueError(f"k * group_size = {k * group_size} exceeds {GROUP_MAX_FETCH}")
    if ncand < 1:
        raise ValueError("the candidate lists must hold at least one entry")
    if ncand > GROUP_MAX_FETCH:
        raise ValueError(f"{ncand} candidates per query exceed {GROUP_MAX_FETCH}")
    return k, group_size, ncand


def group_topk(ids, scores, groups, k: int, group_size: int = 1, id_base: int = 0):
    """Collapse ranked candidate lists to their first ``k`` distinct groups, at most ``group_size`` entries of each
    (ts_group_topk).  ``ids`` [B, C] int64 (-1 = padding) and ``scores`` [B, C] in rank order (the
    scores are carried, never compared); ``groups`` int32, one entry per row, entry ``id`` belonging to row
    ``id - id_base``; a negative table value makes the entry a group of its own.  Walking a list in position order an
    entry is kept iff fewer than ``k`` distinct groups started before its group did and fewer than ``group_size``
    earlier entries share its group.  Returns ``(D, I, G, n_groups, n_valid)``: scores, ids and groups [B, k *
    group_size] of the kept entries in list order, -FLT_MAX / -1 / -1 padded; the distinct groups among ALL valid
    entries of each list (not capped at ``k``) and its valid entries, int32 [B].
    CUDA tensors in -> tensors out, enqueued on the current stream (no synchronisation; an id outside the table is
    skipped like padding); anything else goes through host pointers and comes back as numpy (such an id is a
    ``ValueError``)."""
    lib = _lib.load()
    if _is_tensor(ids) and ids.is_cuda:
        torch = _torch()
        if ids.dim() != 2 or tuple(scores.shape) != tuple(ids.shape):
            raise ValueError(f"expected ids and scores of one shape [B, C], got {tuple(ids.shape)} and "
                             f"{tuple(scores.shape)}")
        k, group_size, C = group_check(k, group_size, ids.shape[1])
        device = ids.device.index
        ids = ids.to(torch.int64).contiguous()
        sc = torch.as_tensor(scores, device=ids.device).to(torch.float32).contiguous()
        tab = torch.as_tensor(groups, device=ids.device)
        if tab.dim() != 1:
            raise ValueError(f"expected a one-dimensional group table, got shape {tuple(tab.shape)}")
        tab = tab.to(torch.int32).contiguous()
        B, W = ids.shape[0], k * group_size
        D = torch.empty((B, W), dtype=torch.float32, device=ids.device)
        I = torch.empty((B, W), dtype=torch.int64, device=ids.device)
        G = torch.empty((B, W), dtype=torch.int32, device=ids.device)
        ng = torch.empty((B,), dtype=torch.int32, device=ids.device)
        nv = torch.empty((B,), dtype=torch.int32, device=ids.device)
        if tab.shape[0] == 0:   # (an empty tensor has no address: every entry is then invalid, nothing is read)
            tab = torch.zeros((1,), dtype=torch.int32, device=ids.device)
            n_rows = 0
        else:
            n_rows = tab.shape[0]
        flags, stream = 0, _stream_ptr(device)
    else:
        ids = np.ascontiguousarray(_to_host(ids), dtype=np.int64)
        sc = np.ascontiguousarray(_to_host(scores), dtype=np.float32)
        groups = _to_host(groups)
        if ids.ndim != 2 or sc.shape != ids.shape:
            raise ValueError(f"expected ids and scores of one shape [B, C], got {ids.shape} and {sc.shape}")
        k, group_size, C = group_check(k, group_size, ids.shape[1])
        tab = np.asarray(groups)
        if tab.ndim != 1:
            raise ValueError(f"expected a one-dimensional group table, got shape {tab.shape}")
        n_rows = tab.shape[0]
        tab = np.ascontiguousarray(tab if n_rows else np.zeros(1), dtype=np.int32)
        B, W = ids.shape[0], k * group_size
        D = np.empty((B, W), dtype=np.float32)
        I = np.empty((B, W), dtype=np.int64)
        G = np.empty((B, W), dtype=np.int32)
        ng = np.empty((B,), dtype=np.int32)
        nv = np.empty((B,), dtype=np.int32)
        device, flags, stream = 0, _lib.TS_FLAG_HOST_PTR, None
    _check(lib.ts_group_topk(_addr(ids), _addr(sc), B, C, _addr(tab), n_rows, int(id_base), k, group_size, _addr(D),
                             _addr(I), _addr(G), _addr(ng), _addr(nv), flags, device, stream), invalid=True)
    return D, I, G, ng, nv


def grouped_search(ix, search, q, k, groups, group_size=1, fetch_k=None):
    """``search_grouped`` of both index classes (and of Stage1Retriever, whose ``search`` carries its filters):
    ``search(q, fetch) -> (D, I)`` is a plain search of ``ix`` with the caller's filter or probe count bound in."""
    n_tab = groups.shape[0] if hasattr(groups, "shape") and len(groups.shape) == 1 else None
    if n_tab is None:
        groups = np.asarray(groups)
        if groups.ndim != 1:
            raise ValueError(f"expected a one-dimensional group table, got shape {groups.shape}")
        n_tab = groups.shape[0]
    if n_tab != ix.ntotal:
        raise ValueError(f"the group table has {n_tab} entries, the index {ix.ntotal} rows")
    fetch = group_default_fetch_k(k, group_size) if fetch_k is None else int(fetch_k)
    k, group_size, fetch = group_check(k, group_size, fetch)
    if _is_tensor(q) and q.is_cuda:   # one upload for every round of the call (a device table is used as it is)
        torch = _torch()
        groups = torch.as_tensor(groups, device=q.device).to(torch.int32)
    rounds = 0
    while True:
        D, I = search(q, fetch)
        D, I, G, ng, nv = group_topk(I, D, groups, k, group_size, id_base=int(getattr(ix, "_id_offset", 0)))
        rounds += 1
        # the call's one host synchronisation per round: both count arrays
        ng_h = ng.cpu().numpy() if _is_tensor(ng) else ng
        nv_h = nv.cpu().numpy() if _is_tensor(nv) else nv
        short = (ng_h < k) & (nv_h == fetch)   # too few groups in a list that was full: rows may lie behind it
        if not short.any() or fetch >= GROUP_MAX_FETCH:
            break
        fetch = min(GROUP_MAX_FETCH, 4 * fetch)
    ix._group_info = {"fetched": fetch, "rounds": rounds, "n_groups": ng_h.copy(), "complete": ~short}
    return D, I, G


class RangeSearchLimitError(RuntimeError):
    """A range search would return more entries than ``max_results`` allows; the message names both numbers.
    ``counts``: results per query as far as the search got (zero behind that)."""

    def __init__(self, message: str, counts: np.ndarray):
        super().__init__(message)
        self.counts = counts


class _IndexBase:
    """What FlatIPIndex and IVFFlatIndex share: the handle's lifetime and the searches built on ``search`` / ``mmr``."""

    _DESTROY = None   # the entry that frees the handle

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self._DESTROY)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _search_mmr(self, q, k, fetch_k, lambda_mult, **how):
        """``search(q, fetch_k, **how)`` followed by :meth:`mmr` on the same stream."""
        k, fetch_k, lam = mmr_check(k, mmr_default_fetch_k(k) if fetch_k is None else fetch_k, lambda_mult)
        D, I = self.search(q, fetch_k, **how)
        return self.mmr(I, D, k, lam)

    def _search_grouped(self, q, k, groups, group_size, fetch_k, **how):
        return grouped_search(self, lambda x, f: self.search(x, f, **how), q, k, groups, group_size, fetch_k)

    def last_group_info(self) -> dict:
        """``{"fetched", "rounds", "n_groups", "complete"}`` of the last :meth:`search_grouped` (the last two per query)."""
        return dict(getattr(self, "_group_info", {}))


class FlatIPIndex(_IndexBase):
    """Exact inner-product index resident in MI355X HBM."""

    _DESTROY = "ts_index_destroy"

    supports_out = True  # search(..., out=(D, I)) writes into caller tensors
    PENDING_PASSES = 240  # passes of <= 32 queries that may wait for finish() (the library tracks 256)
    MAX_KERNEL_K = 16384  # the select kernels hold 16384 keys in LDS; larger k: _search_large_k
    MAX_ASYNC_QUERIES = 128  # per asynchronous library call (4 passes of >= 32 queries)

    def __init__(self, d: int, dtype: str = "f32", device: int = 0, fp8_scale_log2: int = 8):
        """``dtype="fp8"``: one byte per element (e4m3); element x is stored as e4m3(x * 2^fp8_scale_log2)
        (see :func:`quantize_rows_e4m3_fixed_reference`), the default 8 fits unit-norm rows.
        ``dtype="fp4"``: half a byte per element plus a scale byte per 32 (OCP e2m1 with E8M0 block scales, DESIGN.md
        4.23; see :func:`quantize_rows_mxfp4_reference`): a candidate generator for the stages that rerank."""
        if dtype not in _NAME_TO_DTYPE:
            raise ValueError(f"unknown storage dtype {dtype!r}")
        is_fp8 = _NAME_TO_DTYPE[dtype] == _lib.TS_FP8_E4M3
        if is_fp8 and not 0 <= int(fp8_scale_log2) <= 15:
            raise ValueError(f"fp8_scale_log2 must be in 0 .. 15, got {fp8_scale_log2}")
        if is_fp8 and int(d) > FP8_INDEX_MAX_D:
            raise NotImplementedError(f"an fp8 index takes at most {FP8_INDEX_MAX_D} dimensions, got {d}")
        if _NAME_TO_DTYPE[dtype] == _lib.TS_MXFP4_E2M1 and int(d) > FP4_INDEX_MAX_D:
            raise NotImplementedError(f"an fp4 index takes at most {FP4_INDEX_MAX_D} dimensions, got {d}")
        self._lib = _lib.load()
        self.d = int(d)
        self.device = int(device)
        self.storage_dtype = _DTYPE_NAME[_NAME_TO_DTYPE[dtype]]
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.ts_index_create(self.d, _NAME_TO_DTYPE[dtype],
                                             _lib.TS_METRIC_INNER_PRODUCT, self.device,
                                             ctypes.byref(self._h)))
        if is_fp8:
            self.set_fp8_scale_log2(fp8_scale_log2)
        self.is_trained = True  # FAISS attribute; a flat index needs no training
        self._pending = {}      # ticket -> (q, k, D, I) of unfinished async searches
        self._pending_passes = 0
        self._auto_redone = []  # tickets repeated by an internal finish() the caller has not seen yet
        self.auto_finish = True  # False: the owner (ShardedFlatIPIndex) calls finish() itself, collectively
        self.classic_filter = False  # True: every search takes the five-launch filter path (A/B measurements)
        self.one_launch_filter = False  # True: the one-launch scan wherever it is valid (also pipelined / large corpora)
        # async_ searches may share one corpus pass with the batches that follow them (TS_FLAG_COALESCE); results are
        # identical.  False: one pass per batch, as before (A/B runs, owners that read results in stream order)
        self.coalesce = True
        # coalesced passes of ts_coalesce_groups_wide() groups: "auto" where the corpus is larger than the Infinity
        # Cache (ts_coalesce_wide_min_bytes()), True / False to force them on / off (tests, A/B runs)
        self.wide_passes = "auto"
        # coalesced passes of ts_coalesce_groups_stationary() groups (8 at 512 < d <= 768, f16 / bf16): "auto" wherever
        # "auto" wide passes would run and nothing is removed, True / False to force them on / off (tests, A/B runs)
        self.stationary_passes = "auto"
        # in a queue of stationary passes with nothing removed: sample scans and thresholds enqueued with the pass, one
        # launch each per pass for sample scans, thresholds and selects.  "auto" / True: wherever that applies; False:
        # every batch keeps launches of its own (tests, A/B runs).  Results are identical
        self.pass_prologue = "auto"
        self._filter_info = None  # set by finish() when it redid a filtered search: the counters of what was submitted

    # -- FAISS duck type --------------------------------------------------
    @property
    def ntotal(self) -> int:
        return int(self._lib.ts_index_ntotal(self._h))

    def train(self, x) -> None:  # IndexIVFFlat API used at reference :267; no-op here
        return None

    # -- removal (tombstones) -----------------------------
    @property
    def nlive(self) -> int:
        """Rows not removed (``ntotal`` counts every id assigned since the last :meth:`compact` / :meth:`reset`)."""
        return int(self._lib.ts_index_live_count(self._h))

    def remove_ids(self, ids) -> int:
        """FAISS ``remove_ids`` with stable ids: the rows with these ids (as :meth:`search` returns them, i.e. with
        the id offset) are never returned again, but keep their ids and storage until :meth:`compact`.  Unknown,
        repeated and already removed ids are skipped.  Returns how many rows were removed.  Unfinished ``async_``
        searches are finished first, so that every search submitted before sees the index as it was."""
        arr = _id_array(ids)
        self._finish_pending()
        n = ctypes.c_int64(0)
        _lib.check(self._lib.ts_index_remove(self._h, _addr(arr), int(arr.shape[0]), ctypes.byref(n),
                                             _stream_ptr(self.device)))
        return int(n.value)

    def _finish_pending(self) -> None:
        """Before a synchronous call that must see every search submitted so far complete: finish them, and keep what
        that repeated for the caller's own finish()."""
        if self._pending:
            self._auto_redone = self._auto_redone + self.finish()

    def update_rows(self, ids, x, normalize: bool = False) -> None:
        """Replace the stored rows ``ids`` (as :meth:`search` returns them, i.e. with the id offset) by the rows of ``x``
        [len(ids), d] (numpy or a CUDA tensor, as :meth:`add` takes them); afterwards the index holds exactly what
        :meth:`add` of the final matrix would have written.  All or nothing: an id out of range, given
        twice or removed raises ``ValueError`` and nothing is written.  Unfinished ``async_`` searches are finished
        first, as :meth:`remove_ids` does, so that every search submitted before reads the rows as they were."""
        arr = _id_array(ids)
        x, dt, _, on_gpu = _host_query(x, self.d, "rows", int(arr.shape[0]), self.device)
        flags = (_lib.TS_FLAG_NORMALIZE if normalize else 0) | (0 if on_gpu else _lib.TS_FLAG_HOST_PTR)
        self._finish_pending()
        _update_call(self._lib.ts_index_update, self._h, arr, x, dt, flags, _stream_ptr(self.device))

    def live_words(self) -> np.ndarray:
        """The live set as packed uint32 words (the layout of :func:`pack_allowed`)."""
        words = (self.ntotal + 31) // 32
        out = np.zeros(max(words, 1), dtype=np.uint32)
        _lib.check(self._lib.ts_index_live_words(self._h, _addr(out), None))
        return out[:words]

    def live_mask(self) -> np.ndarray:
        """The live set as a bool array over the ``ntotal`` rows."""
        return np.unpackbits(self.live_words().view(np.uint8), bitorder="little")[: self.ntotal].astype(bool)

    def compact(self) -> np.ndarray:
        """Move the live rows down (order kept), drop the removed ones; ``ntotal`` becomes :attr:`nlive`.  Returns
        the old -> new map int64 [old ntotal] (-1 = removed), monotone, so ties keep their order."""
        self._finish_pending()
        n = self.ntotal
        out = np.empty(max(n, 1), dtype=np.int64)
        _lib.check(self._lib.ts_index_compact(self._h, _addr(out), _stream_ptr(self.device)))
        return out[:n]

    @property
    def fp8_scale_log2(self) -> Optional[int]:
        """The scale exponent of an fp8 index (None for another storage dtype)."""
        s = int(self._lib.ts_index_fp8_scale_log2(self._h))
        return s if s >= 0 else None

    def set_fp8_scale_log2(self, s: int) -> None:
        """fp8 storage: the scale exponent, 0 .. 15; only while the index is empty (``ValueError`` otherwise)."""
        _check(self._lib.ts_index_set_fp8_scale_log2(self._h, int(s)), invalid=True)

    def reset(self) -> None:
        _lib.check(self._lib.ts_index_reset(self._h))

    def reserve(self, nrows: int) -> None:
        _lib.check(self._lib.ts_index_reserve(self._h, int(nrows)))

    def set_id_offset(self, offset: int) -> None:
        _lib.check(self._lib.ts_index_set_id_offset(self._h, int(offset)))
        self._id_offset = int(offset)

    def add(self, x, normalize: bool = False) -> None:
        """Append rows ``x`` [n, d] (numpy float32/float16 or a CUDA tensor)."""
        x, dt, n, on_gpu = _host_query(x, self.d, "rows", "n", self.device)
        flags = (_lib.TS_FLAG_NORMALIZE if normalize else 0) | (0 if on_gpu else _lib.TS_FLAG_HOST_PTR)
        _lib.check(self._lib.ts_index_add(self._h, _addr(x), n, dt, flags, _stream_ptr(self.device) if on_gpu else None))

    def search(self, q, k: int, exact_dense: bool = False, async_: bool = False, out=None,
               inputs_ready: bool = False, classic: bool = False, one_launch: bool = False, allowed=None):
        """Top-``k`` inner products.  numpy in -> ``(D float32[B,k], I int64[B,k])``
        numpy out (FAISS convention, -1 padded); CUDA tensor in -> tensors out.

        ``async_=True`` (CUDA tensors only): the work is only enqueued on the current
        stream and the output tensors are returned at once; they are complete and
        verified after :meth:`finish`.  Batches issued this way run back to back on
        the GPU without a host round trip between them.
        ``out=(D, I)``: CUDA tensors [B,k] float32 / int64 to write into.
        With ``coalesce`` (the default) the scan of an ``async_`` batch may wait for the next ones, so that one
        corpus pass serves up to four 32-query groups; :meth:`finish` (or :meth:`flush`) enqueues what is held.
        ``inputs_ready=True`` (with ``async_``): the caller guarantees ``q`` is already
        complete in memory (not the result of work still pending on the stream); the
        library then pipelines this search's small kernels beside its neighbours' scans
        (TS_FLAG_PIPELINE).
        ``allowed``: restrict the search to a subset of the rows (FAISS ``IDSelector``): a bool array /
        tensor over the rows, packed uint32 words (:func:`pack_allowed`), a list with one of these (or
        ``None``: unfiltered) per query, or ``None``.  The result is what an index holding only the
        allowed rows would return, with the original ids; fewer than ``k`` allowed rows pad with
        -1 / -FLT_MAX.  The scan reads only the 32-row blocks some query of a pass may see."""
        k = int(k)
        if k <= 0:
            raise ValueError("k must be positive")
        if allowed is not None and self.ntotal == 0:
            _raise_empty()
        if k > self.MAX_KERNEL_K and self.ntotal > self.MAX_KERNEL_K:
            return self._search_large_k(q, k, out, allowed)
        if async_ and not (_is_tensor(q) and q.is_cuda):
            raise ValueError("async_ search needs a CUDA tensor")
        q, q_dtype, B, on_gpu = _host_query(q, self.d)
        D, I = _outputs(out if on_gpu else None, B, k, q)
        if async_ and B > self.MAX_ASYNC_QUERIES:
            # the library takes at most 4 passes per asynchronous call: larger batches go in slices, a per-query
            # ``allowed`` sliced with the queries
            items = None if allowed is None else _allowed_items(allowed, B)
            for s in range(0, B, self.MAX_ASYNC_QUERIES):
                e = min(B, s + self.MAX_ASYNC_QUERIES)
                self.search(q[s:e], k, exact_dense=exact_dense, async_=True, out=(D[s:e], I[s:e]),
                            inputs_ready=inputs_ready, classic=classic, one_launch=one_launch,
                            allowed=None if items is None else items[s:e])
            return D, I
        flags = (_lib.TS_FLAG_NO_FILTER if exact_dense else 0) | (0 if on_gpu else _lib.TS_FLAG_HOST_PTR)
        stream = _stream_ptr(self.device) if on_gpu else None
        masks = None
        if allowed is None:
            if classic or self.classic_filter:   # the five-launch filter path even where the one-launch scan is the default (A/B, tests)
                flags |= _lib.TS_FLAG_CLASSIC
            elif one_launch or self.one_launch_filter:   # the one-launch scan also where it is not the default
                flags |= _lib.TS_FLAG_ONE_LAUNCH
            if async_:
                self._admit_async(B)
                flags |= _lib.TS_FLAG_ASYNC
                if inputs_ready:
                    flags |= _lib.TS_FLAG_PIPELINE
                elif self.coalesce:
                    flags |= _lib.TS_FLAG_COALESCE
                    flags |= wide_pass_flags(self.wide_passes)
                    flags |= stationary_pass_flags(self.stationary_passes)
                    flags |= pass_prologue_flags(self.pass_prologue)
            self._search_raw(q, q_dtype, k, D, I, flags, stream)
        else:   # (ts_index_search_filtered resets the counters last_filter_info() reads, and never coalesces)
            self._filter_info = None   # last_filter_info() reads the library's counters of this call again
            masks = _marshal_allowed(allowed, B, self.ntotal, q.device if on_gpu else None)
            if async_:
                self._admit_async(B)
                flags |= _lib.TS_FLAG_ASYNC
            self._filtered_raw(q, q_dtype, k, masks, D, I, flags, stream)
        if async_:   # finish() may have to repeat the search: it keeps the queries, the outputs and the masks alive
            self._pending[int(self._lib.ts_index_last_ticket(self._h))] = (q, k, D, I, masks)
            self._pending_passes += (B + 31) // 32
        return D, I

    def _admit_async(self, n_queries: int) -> None:
        """Room for another asynchronous search (the library tracks a fixed number of unfinished passes), made by an
        internal finish() where the index owns its finish() calls."""
        if self.pending_room(n_queries) < 0:
            if not self.auto_finish:
                raise RuntimeError("too many unfinished asynchronous searches: the owner of this index "
                                   "must call finish() (see pending_room())")
            self._auto_redone = self.finish()   # (finish() hands back what an earlier internal one repeated)

    def _search_raw(self, q, q_dtype: int, k: int, D, I, flags: int, stream) -> None:
        _check(self._lib.ts_index_search(self._h, _addr(q), q.shape[0], q_dtype, k, _addr(D), _addr(I), flags, stream))

    def _filtered_raw(self, q, q_dtype: int, k: int, m: _Masks, D, I, flags: int, stream) -> None:
        _check(self._lib.ts_index_search_filtered(self._h, _addr(q), q.shape[0], q_dtype, k, _addr(m.keep), m.words,
                                                  m.n_masks, _addr(m.moq), _addr(D), _addr(I), flags, stream))

    def _search_large_k(self, q, k: int, out, allowed):
        """k > 16384 on a corpus of more than 16384 rows (the select kernels keep 16384 keys in LDS; FAISS itself takes
        any k on the CPU, reference src/stage1_retriever.py:380): every inner product from the HIP dense scan
        (ts_index_scores), then ONE stable descending device sort per slice of queries — equal scores keep ascending
        row order, the canonical tie rule — and the FAISS padding (-1 / -FLT_MAX) beyond ntotal.  Exact; not a fast path:
        it materialises 4 B x queries x rows."""
        torch = _torch()
        if not (_is_tensor(q) and q.is_cuda):   # host queries are scored as f32, whatever they came as
            q = np.ascontiguousarray(_to_host(q.float() if _is_tensor(q) else q), dtype=np.float32)
        qt, _, B, on_gpu = _device_query(q, self.d, self.device)
        n = self.ntotal
        kk = min(k, n)
        D, I = _outputs(out if on_gpu else None, B, k, qt)
        # filtered: rows outside a query's mask sort behind every allowed row (-inf) and are cut; removed rows: every
        # mask ANDed with the live set, which is also the mask of the unfiltered queries
        bits = moq = None
        if allowed is not None:
            m = _marshal_allowed(allowed, B, n)
            bits, moq = m.host, m.moq
        if self.nlive < n:
            live = self.live_words()[None, :]
            bits = live if bits is None else np.concatenate([bits & live, live])
            moq = np.full(B, bits.shape[0] - 1, np.int32) if moq is None else np.where(moq < 0, bits.shape[0] - 1, moq)
        D[:, kk:] = -3.4028234663852886e38
        I[:, kk:] = -1
        step = max(1, int(2e9 // (4 * max(n, 1))))          # <= 2 GB of scores per slice
        off = int(getattr(self, "_id_offset", 0))
        if bits is not None:
            allow = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(bits.shape[0], -1)[:, :n].astype(bool)
            allow_t = torch.from_numpy(allow).to(qt.device)
        for s in range(0, B, step):
            sc = self.scores(qt[s: s + step])
            if bits is not None:
                m = torch.from_numpy(moq[s: s + step].astype(np.int64)).to(qt.device)
                rows_ok = torch.where((m >= 0)[:, None], allow_t[m.clamp(min=0)], torch.ones_like(allow_t[:1]))
                sc = sc.masked_fill(~rows_ok, float("-inf"))
            srt, idx = torch.sort(sc, dim=1, descending=True, stable=True)
            D[s: s + step, :kk] = srt[:, :kk]
            I[s: s + step, :kk] = idx[:, :kk] + off
            if bits is not None:
                cut = torch.isneginf(D[s: s + step])
                D[s: s + step][cut] = -3.4028234663852886e38
                I[s: s + step][cut] = -1
        return (D, I) if on_gpu else (D.cpu().numpy(), I.cpu().numpy())

    # -- range search -----------------------------------------
    def range_search(self, q, radius, allowed=None, max_results: Optional[int] = None, sort: bool = False,
                     exact_dense: bool = False):
        """FAISS ``range_search``: every live row with ``score >= radius`` (inclusive), per query.  Returns
        ``(lims, D, I)`` in FAISS's CSR form: query ``b`` owns ``D[lims[b]:lims[b + 1]]`` / ``I[...]``; ``lims`` is
        int64 [B + 1].  numpy in -> numpy out; a CUDA tensor in -> tensors out (``lims`` on the device too).

        ``radius``: a scalar or one value per query, on the index's score scale; ``-inf`` returns every live row,
        NaN raises ``ValueError``.  Scores are bit-identical to those of :meth:`search` / :meth:`scores`.
        ``allowed``: as for :meth:`search`; removed rows are never returned.
        Within a query the rows come in ascending id order; ``sort=True`` reorders each query's segment by
        descending score, ties by ascending id (the order of :meth:`search`).
        ``max_results``: the most entries the call may return (default 2^26); exceeding it raises
        :class:`RangeSearchLimitError`, which names the count and the limit, and the index stays usable.
        ``exact_dense=True`` forces the dense path (tests, A/B runs).  Synchronous."""
        if self.storage_dtype in ("fp8", "fp4"):
            raise NotImplementedError(f"range_search is not supported on an {self.storage_dtype} index")
        q, q_dtype, B, on_gpu = _host_query(q, self.d)
        rad = np.asarray(_to_host(radius.float() if _is_tensor(radius) else radius), dtype=np.float32).reshape(-1)
        if rad.size == 1:
            rad = np.full(B, rad[0], dtype=np.float32)
        if rad.size != B:
            raise ValueError(f"radius: {rad.size} values for {B} queries")
        if np.isnan(rad).any():
            raise ValueError("radius must not be NaN")
        rad = np.ascontiguousarray(rad)
        if self.ntotal == 0:
            _raise_empty()
        self._finish_pending()   # unfinished async_ searches are verified first: this call is synchronous
        flags = (_lib.TS_FLAG_NO_FILTER if exact_dense else 0) | (0 if on_gpu else _lib.TS_FLAG_HOST_PTR)
        stream = _stream_ptr(self.device) if on_gpu else None
        m = _NO_MASKS if allowed is None else _marshal_allowed(allowed, B, self.ntotal, q.device if on_gpu else None)
        lims = np.zeros(B + 1, dtype=np.int64)
        code = self._lib.ts_index_range_search(
            self._h, _addr(q), B, q_dtype, _addr(rad), _addr(m.bits), m.words, m.n_masks,
            _addr(m.moq) if m.n_masks else None, int(max_results) if max_results is not None else 0, _addr(lims),
            flags, stream)
        if code == _lib.TS_ERR_UNSUPPORTED and "exceed the limit" in _lib.last_error():
            raise RangeSearchLimitError(_lib.last_error(), np.diff(lims))
        _check(code)
        total = int(lims[B])
        if on_gpu:
            torch = _torch()
            D = torch.empty(total, dtype=torch.float32, device=q.device)
            I = torch.empty(total, dtype=torch.int64, device=q.device)
        else:
            D = np.empty(total, dtype=np.float32)
            I = np.empty(total, dtype=np.int64)
        _lib.check(self._lib.ts_index_range_fetch(self._h, _addr(D), _addr(I), total,
                                                  0 if on_gpu else _lib.TS_FLAG_HOST_PTR, stream))
        if not on_gpu:
            if sort and total:
                seg = np.repeat(np.arange(B), np.diff(lims))
                order = np.lexsort((I, -(D + np.float32(0.0)), seg))   # segment, then score descending, then id
                D, I = D[order], I[order]
            return lims, D, I
        L = torch.from_numpy(lims).to(q.device)
        if sort and total:
            # descending score with -0 equal to +0, then ascending id: ids ascend inside a segment already, so two
            # stable sorts (score, then segment) give the order of search()
            seg = torch.repeat_interleave(torch.arange(B, device=q.device), L[1:] - L[:-1])
            o1 = torch.sort(D + 0.0, descending=True, stable=True).indices
            o2 = torch.sort(seg[o1], stable=True).indices
            order = o1[o2]
            D, I = D[order], I[order]
        return L, D, I

    def last_range_info(self) -> dict:
        """The last :meth:`range_search`: its passes (of <= 64 queries; 32 where the 64-query image does not fit the LDS),
        how many ran the filter scan, and how many of those were redone densely because a query had more than 16384
        results."""
        arr = (ctypes.c_int64 * 4)()
        _lib.check(self._lib.ts_index_last_search_info(self._h, arr))
        if not arr[0] & 32:
            raise RuntimeError("the last search on this index was not a range search")
        return {"passes": int(arr[1]), "filter_passes": int(arr[2]), "dense_redo": int(arr[3])}

    def last_filter_info(self) -> dict:
        """The last filtered search: row blocks (32 rows) its scans read, row blocks of the index, passes on the
        masked filter path and on the dense path (asynchronous searches: complete after :meth:`finish`)."""
        if getattr(self, "_filter_info", None) is not None:
            return dict(self._filter_info)
        return self._read_filter_info()

    def _read_filter_info(self) -> dict:
        arr = (ctypes.c_int64 * 4)()
        _lib.check(self._lib.ts_index_last_filter_info(self._h, arr))
        return {"live_blocks": int(arr[0]), "total_blocks": int(arr[1]), "filter_passes": int(arr[2]),
                "dense_passes": int(arr[3])}

    def scores(self, q):
        """All inner products, in row order: float32 [B, ntotal] (a CUDA tensor for tensor
        input, numpy for numpy input).  No selection; the dense scan writes the matrix."""
        was_np = not _is_tensor(q)
        if was_np:   # a host array is scored as f32, whatever it came as
            q = np.ascontiguousarray(q, dtype=np.float32)
        qt, q_dtype, B, _ = _device_query(q, self.d, self.device)
        n = self.ntotal
        if n == 0:
            _raise_empty()
        ld = (n + 31) // 32 * 32
        out = _torch().empty((B, ld), dtype=_torch().float32, device=qt.device)
        _lib.check(self._lib.ts_index_scores(self._h, _addr(qt), B, q_dtype, _addr(out), ld, _stream_ptr(self.device)))
        out = out[:, :n]
        return out.cpu().numpy() if was_np else out

    def search_in_stream_order(self, q, k: int):
        """search() for a caller that consumes (D, I) on the current stream only: when the dense path will be taken
        (small corpora, k > 2048 — exact by construction) the search is just ENQUEUED and the host does not wait; on the
        filter path it is the ordinary synchronous, verified search.  CUDA tensor queries only."""
        path = int(self._lib.ts_index_filter_path(self._h, int(k)))
        if path != 0 or not (_is_tensor(q) and q.is_cuda) or not self.auto_finish:
            return self.search(q, k)
        return self.search(q, k, async_=True)     # (its ticket is retired by the next finish(); nothing to verify)

    def pending_room(self, n_queries: int) -> int:
        """>= 0 while another asynchronous search of `n_queries` queries fits before a finish()."""
        return self.PENDING_PASSES - self._pending_passes - (int(n_queries) + 31) // 32

    def flush(self) -> None:
        """Enqueue the scans that coalesced ``async_`` searches are holding, without a host sync: their results
        are then ordered on the current stream (still verified only by :meth:`finish`)."""
        _lib.check(self._lib.ts_index_flush(self._h, _stream_ptr(self.device)))

    def finish(self):
        """Complete every asynchronous search: one stream sync, then the (rare)
        batches whose fused filter could not prove exactness are repeated on the
        exact dense path, in place.  Returns the tickets that were repeated since the
        caller's previous finish() (including those an internal finish() — issued when
        too many searches were pending — had to repeat)."""
        failed = (ctypes.c_int64 * 256)()
        nf = ctypes.c_int32(0)
        _lib.check(self._lib.ts_index_finish(self._h, _stream_ptr(self.device), failed, 256, ctypes.byref(nf)))
        redone = []
        if any(self._pending[int(failed[i])][4] is not None for i in range(nf.value)):
            # a redo is a new library call that resets the filter counters: last_filter_info() keeps describing the
            # searches that were submitted (complete now that ts_index_finish has run)
            self._filter_info = self._read_filter_info()
        for i in range(nf.value):
            q, k, D, I, masks = self._pending[int(failed[i])]
            if masks is None:
                self._search_raw(q, _tensor_dtype(q), k, D, I, _lib.TS_FLAG_NO_FILTER, _stream_ptr(self.device))
            else:   # a filtered search: redone on the exact dense path with the masks it kept alive
                self._filtered_raw(q, _tensor_dtype(q), k, masks, D, I, _lib.TS_FLAG_NO_FILTER, _stream_ptr(self.device))
            redone.append(int(failed[i]))
        self._pending.clear()
        self._pending_passes = 0
        if self._auto_redone:
            redone = self._auto_redone + redone
            self._auto_redone = []
        return redone

    # -- diversified selection (MMR) -------------------------
    def mmr(self, ids, relevance, k: int, lambda_mult: float = 0.5):
        """Maximal marginal relevance over stored rows: per query pick ``k`` of the candidates ``ids`` [B, fetch_k]
        (ids as :meth:`search` returns them, -1 = padding, ``fetch_k <= 1024``) with relevances ``relevance``
        [B, fetch_k].  Step 0 takes the largest relevance, step t the candidate maximising
        ``lambda_mult * relevance - (1 - lambda_mult) * max similarity to the picks so far`` in f32, ties to the lower
        position; the similarity is the inner product of the stored rows.  Returns ``(D, I)`` [B, k] in selection
        order, ``D`` the relevances of the picks, -FLT_MAX / -1 padded.  Removed rows are skipped like padding.
        CUDA tensors in -> tensors out, enqueued on the current stream (no synchronisation); numpy in -> numpy out."""
        self._no_fp4("mmr")
        return _mmr_call(self, "ts_index_mmr", ids, relevance, k, lambda_mult)

    def _no_fp4(self, what: str) -> None:
        if getattr(self, "storage_dtype", None) == "fp4":
            raise NotImplementedError(f"{what} is not supported on an fp4 index")

    def mmr_timings(self, on: Optional[bool] = None, reset: bool = True) -> dict:
        """Measurement aid: ``on`` switches the per-kernel timing of :meth:`mmr` (timed calls synchronise); returns the
        milliseconds summed since the last reset."""
        if on is not None:
            _lib.check(self._lib.ts_index_mmr_set_timing(self._h, 1 if on else 0))
        ms = (ctypes.c_double * 3)()
        calls = ctypes.c_int64(0)
        _lib.check(self._lib.ts_index_mmr_get_timings(self._h, ms, ctypes.byref(calls), 1 if reset else 0))
        return {"gather_ms": ms[0], "gram_ms": ms[1], "greedy_ms": ms[2], "calls": int(calls.value)}

    def search_mmr(self, q, k: int, fetch_k: Optional[int] = None, lambda_mult: float = 0.5, allowed=None):
        """``search(q, fetch_k, allowed=allowed)`` followed by :meth:`mmr` on the same stream; ``fetch_k`` defaults to
        ``min(1024, max(4 k, 20))``."""
        self._no_fp4("search_mmr")
        return self._search_mmr(q, k, fetch_k, lambda_mult, allowed=allowed)

    # -- grouped search --------------------------------------
    def search_grouped(self, q, k: int, groups, group_size: int = 1, fetch_k: Optional[int] = None, allowed=None):
        """``search(q, fetch)`` followed by :func:`group_topk` on the same stream: per query the ``k`` best distinct
        groups, at most ``group_size`` rows of each, as ``(D, I, G)`` [B, k * group_size] in ``search``'s canonical order
        (-FLT_MAX / -1 / -1 padded).  ``groups``: int32, one entry per row of the index (``ntotal``; a negative value
        makes the row a group of its own), indexed by row: the index's id offset is taken off the ids.
        ``fetch`` starts at ``fetch_k``, by default ``min(16384, max(4 k group_size, 64))``.  After each round the two
        count arrays are read (the call's one host synchronisation per round); while some query found fewer than ``k``
        groups in a list that came back full and ``fetch < 16384``, ``fetch`` is multiplied by four and the whole
        batch is redone, so every query of a call is collapsed over the same final fetch.  :meth:`last_group_info`
        reports ``fetched``, ``rounds``, ``n_groups`` and ``complete`` (per query: ``k`` groups were found or the list
        was exhaustive); an incomplete query is reported there, not raised.
        ``group_size == 1``: for a complete query the result is exactly the ``k`` groups with the best best-row, in the
        order of those rows, each represented by that row.  ``group_size > 1``: a group's rows are its best rows WITHIN
        THE FIRST ``fetched`` PLACES (the non-strict group size of Milvus): a further row of a returned group that
        ranks behind place ``fetched`` is not returned."""
        return self._search_grouped(q, k, groups, group_size, fetch_k, allowed=allowed)

    # -- funnel search ----------------------------------------
    def _funnel_storage(self, what: str) -> None:
        if self.storage_dtype not in ("f16", "bf16"):
            raise NotImplementedError(f"{what} takes an f16 or bf16 index, not {self.storage_dtype}")

    def search_prefix(self, q, k: int, dims: int, allowed=None, exact_dense: bool = False):
        """Top-``k`` on the inner product over the first ``dims`` components only: ``q`` is the full ``[B, d]`` query,
        the pass uses ``q[:, :dims]`` and reads the first ``dims / 16`` KiB of every 32-row block.  Stored rows are used
        as they are (nothing is renormalised).  The result is, bit for bit and id for id, what ``search(q[:, :dims], k,
        allowed=allowed)`` returns on an index of ``dims`` dimensions holding ``reconstruct_n()[:, :dims]`` under the same
        ids with the same rows removed.  ``dims % 128 == 0``, ``128 <= dims < d``, ``k <= 16384`` (``ValueError``
        otherwise); f16 / bf16 storage.  Synchronous, on the current stream.  numpy in -> numpy out; CUDA tensor in ->
        tensors out.  ``allowed``: every form :meth:`search` takes."""
        self._funnel_storage("search_prefix")
        k, dims = funnel_check(self.d, dims, k)
        if self.ntotal == 0:
            _raise_empty()
        q, q_dtype, B, on_gpu = _host_query(q, self.d)
        q = q[:, :dims].contiguous() if on_gpu else np.ascontiguousarray(q[:, :dims])
        D, I = _outputs(None, B, k, q)
        flags = (_lib.TS_FLAG_NO_FILTER if exact_dense else 0) | (0 if on_gpu else _lib.TS_FLAG_HOST_PTR)
        m = _NO_MASKS if allowed is None else _marshal_allowed(allowed, B, self.ntotal, q.device if on_gpu else None)
        _check(self._lib.ts_index_search_prefix(
            self._h, _addr(q), B, q_dtype, dims, k, _addr(m.bits), m.words if m.n_masks else 0, m.n_masks,
            _addr(m.moq), _addr(D), _addr(I), flags, _stream_ptr(self.device) if on_gpu else None), invalid=True)
        return D, I

    def rescore(self, q, ids, k: Optional[int] = None):
        """Exact full-dimension scores of given candidates: ``ids`` int64 ``[B, C]`` (numpy or a CUDA tensor, ids as
        :meth:`search` returns them, ``C <= 16384``) -> ``(D, I)`` ``[B, k]``, ``k = C`` by default.  Per query the valid
        entries ordered by score descending, then id ascending; entries that are -1, out of range or removed become
        -1 / -FLT_MAX at the end; a duplicate id stays a duplicate.  Every score is bit-identical to
        ``scores(q)[b, id]``, and so to :meth:`search`.  Synchronous, on the current stream; tensors out when ``q`` or
        ``ids`` is a CUDA tensor, numpy otherwise."""
        self._funnel_storage("rescore")
        if q.ndim != 2 or q.shape[1] != self.d:   # (every argument is checked before anything is uploaded)
            _bad_shape("B", self.d, "queries", q.shape)
        if ids.ndim != 2 or ids.shape[0] != q.shape[0]:
            raise ValueError(f"expected ids [B, C] with B = {q.shape[0]}, got {tuple(ids.shape)}")
        C = int(ids.shape[1])
        k = C if k is None else int(k)
        if not 1 <= C <= FUNNEL_MAX_FETCH:
            raise ValueError(f"rescore takes 1 .. {FUNNEL_MAX_FETCH} candidates per query, got {C}")
        if not 1 <= k <= C:
            raise ValueError(f"k={k} must be in 1 .. C = {C}")
        if self.ntotal == 0:
            _raise_empty()
        torch = _torch()
        q, q_dtype, B, on_gpu = _device_query(q, self.d, self.device)
        was_np = not (on_gpu or (_is_tensor(ids) and ids.is_cuda))
        ids = ids if _is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64))
        ids = ids.to(device=q.device, dtype=torch.int64).contiguous()
        D, I = _outputs(None, B, k, q)
        if B:
            _check(self._lib.ts_index_rescore(self._h, _addr(q), B, q_dtype, _addr(ids), C, k, _addr(D), _addr(I),
                                              _stream_ptr(self.device)), invalid=True)
        return (D.cpu().numpy(), I.cpu().numpy()) if was_np else (D, I)

    def search_funnel(self, q, k: int, dims: int, fetch_k: Optional[int] = None, allowed=None):
        """Funnel retrieval: ``rescore(q, search_prefix(q, fetch_k, dims, allowed)[1], k)`` on one stream; no row and no
        list leaves the GPU between the passes.  The scores are the exact scores of :meth:`search`; a row of the exact
        top ``k`` is missed only when its prefix score ranks behind place ``fetch_k``.  ``fetch_k`` defaults to
        ``min(2048, max(8 k, 128))`` (the filter path of the prefix pass); ``k <= fetch_k <= 16384``.
        :meth:`last_funnel_info` describes the call."""
        self._funnel_storage("search_funnel")
        k, dims, fetch_k = funnel_check(self.d, dims, k, funnel_default_fetch_k(k) if fetch_k is None else fetch_k)
        if self.ntotal == 0:
            _raise_empty()
        q, _, _, on_gpu = _device_query(q, self.d, self.device)
        _, cand = self.search_prefix(q, fetch_k, dims, allowed=allowed)
        path = "filter" if self.last_search_info()["path"] == "filter" else "dense"
        D, I = self.rescore(q, cand, k)
        self._funnel_info = {"dims": dims, "fetch_k": fetch_k, "prefix_path": path}
        return (D, I) if on_gpu else (D.cpu().numpy(), I.cpu().numpy())

    def last_funnel_info(self) -> dict:
        """``{"dims", "fetch_k", "prefix_path"}`` of the last :meth:`search_funnel`; ``prefix_path`` is ``"filter"`` when
        the prefix pass's threshold filter gave the shortlist, ``"dense"`` when the dense path did (small corpora,
        ``fetch_k > 2048``, or the exact fallback)."""
        return dict(getattr(self, "_funnel_info", {}))

    # -- boosted search ---------------------------------------
    def search_biased(self, q, k: int, bias, allowed=None, exact_dense: bool = False, check_finite: bool = True):
        """Top-``k`` by ``score + bias``: ``bias`` is float32 with one entry per row (``ntotal``, indexed by local row:
        the index's id offset is taken off the ids), added to every query's score inside the scan, so the result is
        exact: the ``k`` allowed live rows with the largest ``float32(score + bias[row])``, ties to the lower id,
        -1 / -FLT_MAX padded.  ``D`` holds the boosted scores; each is one f32 addition of the score :meth:`search` and
        :meth:`scores` give the pair and the row's bias.  ``k <= 16384`` (``ValueError`` otherwise); f16 / bf16 storage.
        ``check_finite`` (default): a NaN or an infinity in ``bias`` is a ``ValueError``.  ``check_finite=False`` applies
        to CUDA tensor queries only (the bias is then read on the device as it is): a row whose boosted score is NaN is
        never returned and the effect of an infinite entry is undefined.  With numpy queries the bias goes through the
        host, where it is always checked.  Synchronous, on the current
        stream.  numpy queries in -> numpy out (``bias`` then goes through the host); CUDA tensor queries in -> tensors
        out (``bias`` is used in place when it is a 16-byte aligned float32 tensor on the index's GPU, uploaded
        otherwise).  ``allowed``: every form :meth:`search` takes.  :meth:`last_bias_info` describes the call."""
        if self.storage_dtype not in ("f16", "bf16"):
            raise NotImplementedError(f"search_biased takes an f16 or bf16 index, not {self.storage_dtype}")
        k = bias_check_k(k)
        n = self.ntotal
        if n == 0:
            _raise_empty()
        q, q_dtype, B, on_gpu = _host_query(q, self.d)
        b = _marshal_bias(bias, n, q.device if on_gpu else None, check_finite)
        D, I = _outputs(None, B, k, q)
        flags = (_lib.TS_FLAG_NO_FILTER if exact_dense else 0) | (0 if on_gpu else _lib.TS_FLAG_HOST_PTR)
        m = _NO_MASKS if allowed is None else _marshal_allowed(allowed, B, n, q.device if on_gpu else None)
        _check(self._lib.ts_index_search_biased(
            self._h, _addr(q), B, q_dtype, k, _addr(b), n, _addr(m.bits), m.words if m.n_masks else 0, m.n_masks,
            _addr(m.moq), _addr(D), _addr(I), flags, _stream_ptr(self.device) if on_gpu else None), invalid=True)
        return D, I

    def last_bias_info(self) -> dict:
        """The last :meth:`search_biased`: its passes (of <= 64 queries; 32 where the 64-query image does not fit the LDS),
        those whose first attempt was the fused path
        (thresholds and the biased filter scan), those of them redone on the exact dense path, and the 32-row blocks
        its scans read."""
        arr = (ctypes.c_int64 * 4)()
        _lib.check(self._lib.ts_index_last_bias_info(self._h, arr))
        return {"passes": int(arr[0]), "fused_passes": int(arr[1]), "redone": int(arr[2]), "blocks_read": int(arr[3])}

    def reconstruct_n(self, i0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Rows [i0, i0+n) as float32 (after storage rounding)."""
        if n is None:
            n = self.ntotal - i0
        out = np.empty((n, self.d), dtype=np.float32)
        if n:
            _lib.check(self._lib.ts_index_reconstruct(self._h, int(i0), int(n), _addr(out), _lib.TS_FLAG_HOST_PTR, None))
        return out

    PHASES = ("qprep", "sample_scan", "tau", "filter_scan", "select", "dense", "_6", "_7")

    def set_profiling(self, on: bool = True, every: int = 1) -> None:
        """HIP-event timing of the search phases; ``every=N`` times each N-th search only."""
        _lib.check(self._lib.ts_index_set_profiling(self._h, (max(int(every), 1) if on else 0)))

    def timings(self, reset: bool = True) -> dict:
        """{phase: (total_ms, count)} measured with HIP events on the search stream."""
        ms = (ctypes.c_double * 8)()
        cnt = (ctypes.c_int64 * 8)()
        _lib.check(self._lib.ts_index_get_timings(self._h, ms, cnt, 1 if reset else 0))
        return {self.PHASES[i]: (float(ms[i]), int(cnt[i])) for i in range(6)}

    def read_probe(self, reps: int = 5) -> dict:
        """Read-only pass over the index's own tiled corpus with the scan's access pattern (no LDS, no MFMA):
        the streaming ceiling of THIS box, measured with HIP events.  {"bytes", "ms_avg", "ms_best", "gbps_avg",
        "gbps_best"}."""
        ms_avg, ms_best, nbytes = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
        _lib.check(self._lib.ts_index_read_probe(self._h, int(reps), ctypes.byref(ms_avg), ctypes.byref(ms_best),
                                                 ctypes.byref(nbytes), _stream_ptr(self.device)))
        return {"bytes": int(nbytes.value), "ms_avg": ms_avg.value, "ms_best": ms_best.value,
                "gbps_avg": nbytes.value / (ms_avg.value * 1e-3) / 1e9, "gbps_best": nbytes.value / (ms_best.value * 1e-3) / 1e9}

    def last_search_info(self) -> dict:
        arr = (ctypes.c_int64 * 4)()
        _lib.check(self._lib.ts_index_last_search_info(self._h, arr))
        if arr[0] & 32:   # a range search: last_range_info() reads these counters
            return {"path": ("dense", "filter", "filter+dense-fallback")[arr[0] & 3], "one_launch": False, "range": True,
                    "passes": int(arr[1]), "filter_passes": int(arr[2]), "dense_redo": int(arr[3])}
        return {"path": ("dense", "filter", "filter+dense-fallback")[arr[0] & 15],
                "one_launch": bool(arr[0] & 16),   # query image + thresholds + scan+filter in ONE kernel
                "max_candidates": int(arr[1]), "sample_rows": int(arr[2]),
                "sample_rank": int(arr[3])}


def merge_topk(scores, ids, k: Optional[int] = None):
    """Merge per-shard sorted lists ``scores``/``ids`` [R, B, k] (CUDA tensors)
    into the global top-k [B, k] with the canonical (score desc, id asc) order."""
    torch = _torch()
    lib = _lib.load()
    if scores.dim() != 3 or ids.shape != scores.shape:
        raise ValueError("expected scores/ids of shape [R, B, k]")
    R, B, kk = scores.shape
    if k is not None and k != kk:
        raise ValueError("k must equal the list length")
    scores = scores.contiguous().float()
    ids = ids.contiguous().to(torch.int64)
    out_s = torch.empty((B, kk), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((B, kk), dtype=torch.int64, device=scores.device)
    dev = scores.device.index
    _lib.check(lib.ts_merge_topk(_addr(scores), _addr(ids), R, B, kk, _addr(out_s), _addr(out_i), dev,
                                 _stream_ptr(dev)))
    return out_s, out_i


def packed_layout(B: int, k: int):
    """(offset of the int64 id block, bytes per rank) of one rank's packed partial result:
    float32 scores [B,k], padded to a multiple of 8 bytes, then int64 ids [B,k]."""
    ids_at = (4 * B * k + 7) & ~7
    return ids_at, ids_at + 8 * B * k


def merge_topk_packed(gathered, R: int, B: int, k: int):
    """Merge straight out of an all-gather buffer: `gathered` is a uint8 CUDA tensor of R
    blocks, each laid out as packed_layout(B, k) says."""
    torch = _torch()
    lib = _lib.load()
    ids_at, nbytes = packed_layout(B, k)
    if gathered.dtype != torch.uint8 or gathered.numel() != R * nbytes or gathered.data_ptr() % 8:
        raise ValueError("bad packed buffer")
    out_s = torch.empty((B, k), dtype=torch.float32, device=gathered.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=gathered.device)
    base = gathered.data_ptr()
    dev = gathered.device.index
    _lib.check(lib.ts_merge_topk_strided(base, base + ids_at, R, B, k, nbytes // 4, nbytes // 8, _addr(out_s),
                                         _addr(out_i), dev, _stream_ptr(dev)))
    return out_s, out_i


def maxsim(q, docs, doc_offsets, mode: str = "maxsim"):
    """Stage-2 scores of every candidate for one query (CUDA tensors).

    q [Lq, H]; docs [sum(Ld), H] packed token embeddings; doc_offsets int32
    [n_docs+1].  mode 'maxsim' | 'colbert' (reference src/stage2_rescorer.py:167-201)."""
    torch = _torch()
    lib = _lib.load()
    if q.dtype != docs.dtype:
        docs = docs.to(q.dtype)
    q = q.contiguous()
    docs = docs.contiguous()
    doc_offsets = doc_offsets.to(device=q.device, dtype=torch.int32).contiguous()
    n_docs = doc_offsets.numel() - 1
    out = torch.empty((max(n_docs, 0),), dtype=torch.float32, device=q.device)
    if n_docs <= 0:
        return out
    dev = q.device.index
    _lib.check(lib.ts_maxsim(_addr(q), q.shape[0], _addr(docs), _addr(doc_offsets), n_docs, q.shape[1],
                             _tensor_dtype(q), 0 if mode == "maxsim" else 1, _addr(out), dev, _stream_ptr(dev)))
    return out


def maxsim_indexed(q, store, starts, lens, mode: str = "maxsim"):
    """Stage-2 scores for candidates that live in a resident token store: document i
    is rows [starts[i], starts[i]+lens[i]) of ``store`` [rows, H] (CUDA tensors; starts
    int64, lens int32).  The kernel reads the store in place.  A float8_e4m3fn store (quantize_rows_fp8) is
    scored against the query in bf16 / f16 (an f32 query goes to bf16)."""
    torch = _torch()
    lib = _lib.load()
    if not store.is_contiguous():
        raise ValueError("token store must be contiguous")
    if _is_fp8(store):   # an e4m3 store: the query stays bf16 / f16
        return _maxsim_indexed_fp8(q, store, starts, lens, mode)
    if q.dtype != store.dtype:
        q = q.to(store.dtype)
    q = q.contiguous()
    starts = starts.to(device=q.device, dtype=torch.int64).contiguous()
    lens = lens.to(device=q.device, dtype=torch.int32).contiguous()
    n = starts.numel()
    out = torch.empty((n,), dtype=torch.float32, device=q.device)
    if n == 0:
        return out
    dev = q.device.index
    _lib.check(lib.ts_maxsim_indexed(_addr(q), q.shape[0], _addr(store), _addr(starts), _addr(lens), n, q.shape[1],
                                     _tensor_dtype(q), 0 if mode == "maxsim" else 1, _addr(out), dev, _stream_ptr(dev)))
    return out


def maxsim_indexed_batch(q_packed, q_offsets, store, starts, lens, cand_offsets, mode: str = "maxsim"):
    """Stage-2 scores for SEVERAL queries in one launch: query j has tokens
    q_packed[q_offsets[j]:q_offsets[j+1]] and candidates starts/lens[cand_offsets[j]:cand_offsets[j+1]]
    (rows of the resident token ``store``; a float8_e4m3fn store as in maxsim_indexed).  q_offsets / cand_offsets:
    host int sequences of nq+1 values starting at 0.  Returns float32 [cand_offsets[-1]] on the GPU."""
    import numpy as np
    torch = _torch()
    lib = _lib.load()
    fp8 = _is_fp8(store)
    if fp8:   # an e4m3 store: the query stays bf16 / f16
        q_packed = q_packed.to(fp8_query_dtype(q_packed.dtype))
    elif q_packed.dtype != store.dtype:
        q_packed = q_packed.to(store.dtype)
    q_packed = q_packed.contiguous()
    if not store.is_contiguous():
        raise ValueError("token store must be contiguous")
    qo = np.ascontiguousarray(np.asarray(q_offsets, dtype=np.int32))
    co = np.ascontiguousarray(np.asarray(cand_offsets, dtype=np.int32))
    if qo.ndim != 1 or qo.shape != co.shape or qo.size < 1 or qo[0] != 0 or co[0] != 0:
        raise ValueError("q_offsets / cand_offsets must be 1-D, of equal length nq+1, starting at 0")
    nq = qo.size - 1
    if int(qo[-1]) != q_packed.shape[0]:
        raise ValueError("q_offsets[-1] must equal the number of packed query tokens")
    starts = starts.to(device=q_packed.device, dtype=torch.int64).contiguous()
    lens = lens.to(device=q_packed.device, dtype=torch.int32).contiguous()
    n = int(co[-1])
    if starts.numel() != n or lens.numel() != n:
        raise ValueError("starts / lens must hold cand_offsets[-1] entries")
    out = torch.empty((n,), dtype=torch.float32, device=q_packed.device)
    if n == 0 or nq == 0:
        return out
    dev = q_packed.device.index
    if fp8:
        _lib.check(lib.ts_maxsim_indexed_batch_fp8(_addr(q_packed), _tensor_dtype(q_packed), _addr(qo), nq,
                                                   _addr(store), _addr(starts), _addr(lens), _addr(co),
                                                   q_packed.shape[1], 0 if mode == "maxsim" else 1, _addr(out), dev,
                                                   _stream_ptr(dev)))
        return out
    _lib.check(lib.ts_maxsim_indexed_batch(_addr(q_packed), _addr(qo), nq, _addr(store), _addr(starts), _addr(lens),
                                           _addr(co), q_packed.shape[1], _tensor_dtype(q_packed),
                                           0 if mode == "maxsim" else 1, _addr(out), dev, _stream_ptr(dev)))
    return out


# ---- best passage per candidate (include/tristage.h) ----------------------------------------
PASSAGE_MAX_LQ, PASSAGE_MAX_LD = 256, 1024


def passage_check(window, H: int, store, max_lq: int, max_len: int) -> None:
    """The refusals of ts_maxsim_passages_indexed(_batch), raised before anything is launched."""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"window must be an integer >= 1, got {window!r}")
    if _is_fp8(store):
        raise NotImplementedError("best passages over an e4m3 token store are not supported")
    if (H * store.element_size()) % 16:
        raise ValueError(f"token rows of {H * store.element_size()} bytes (H = {H}): a multiple of 16 bytes is needed")
    if max_lq > PASSAGE_MAX_LQ:
        raise ValueError(f"a query of {max_lq} tokens: at most {PASSAGE_MAX_LQ}")
    if max_len > PASSAGE_MAX_LD:
        raise ValueError(f"a candidate of {max_len} token rows: at most {PASSAGE_MAX_LD}")


def maxsim_passages_indexed(q, store, starts, lens, window: int, align: bool = False, max_len: Optional[int] = None):
    """The best passage of every candidate for one query: for candidate i (rows [starts[i], starts[i] + lens[i]) of
    the resident token ``store``) the window of min(window, lens[i]) consecutive token rows whose windowed MaxSim —
    the sum over the query tokens of the best cosine inside the window — is largest (ties: the lowest start).
    Returns device tensors (start int32 [n], length int32 [n], score float32 [n] = that sum / Lq[, align int32
    [n, Lq]: each query token's best row inside the window, as a position in the document]).  A candidate without
    rows gets (-1, 0, -FLT_MAX, -1).  ``max_len``: an upper bound of ``lens`` the caller knows; without it the
    lengths are read back once to refuse a candidate of more than 1024 rows."""
    Lq = int(q.shape[0])
    if Lq < 1:
        raise ValueError("the query has no tokens")
    n = int(starts.numel())
    out = maxsim_passages_indexed_batch(q, [0, Lq], store, starts, lens, [0, n], window, align=align, max_len=max_len)
    return out


def maxsim_passages_indexed_batch(q_packed, q_offsets, store, starts, lens, cand_offsets, window: int,
                                  align: bool = False, max_len: Optional[int] = None):
    """maxsim_passages_indexed for SEVERAL queries in one call, with the argument conventions of
    maxsim_indexed_batch.  The alignment has max Lq columns; row r of query j holds -1 at t >= Lq_j."""
    torch = _torch()
    lib = _lib.load()
    if not store.is_contiguous():
        raise ValueError("token store must be contiguous")
    qo = np.ascontiguousarray(np.asarray(q_offsets, dtype=np.int32))
    co = np.ascontiguousarray(np.asarray(cand_offsets, dtype=np.int32))
    if qo.ndim != 1 or qo.shape != co.shape or qo.size < 1 or qo[0] != 0 or co[0] != 0:
        raise ValueError("q_offsets / cand_offsets must be 1-D, of equal length nq+1, starting at 0")
    if (np.diff(qo) < 0).any() or (np.diff(co) < 0).any():
        raise ValueError("q_offsets / cand_offsets must be non-decreasing")
    nq = qo.size - 1
    if int(qo[-1]) != q_packed.shape[0]:
        raise ValueError("q_offsets[-1] must equal the number of packed query tokens")
    n = int(co[-1])
    if starts.numel() != n or lens.numel() != n:
        raise ValueError("starts / lens must hold cand_offsets[-1] entries")
    lqs = np.diff(qo)
    if ((np.diff(co) > 0) & (lqs < 1)).any():
        raise ValueError("a query with candidates has no tokens")
    max_lq = int(lqs.max()) if nq else 0
    H = int(q_packed.shape[1])
    if store.dim() != 2 or store.shape[1] != H:
        raise ValueError("q and store must have the same row length")
    lens = lens.to(device=q_packed.device, dtype=torch.int32).contiguous()
    if max_len is None:
        max_len = int(lens.max().item()) if n else 0
    passage_check(window, H, store, max_lq, int(max_len))
    if q_packed.dtype != store.dtype:
        q_packed = q_packed.to(store.dtype)
    q_packed = q_packed.contiguous()
    starts = starts.to(device=q_packed.device, dtype=torch.int64).contiguous()
    dev_t = q_packed.device
    o_start = torch.empty((n,), dtype=torch.int32, device=dev_t)
    o_len = torch.empty((n,), dtype=torch.int32, device=dev_t)
    o_score = torch.empty((n,), dtype=torch.float32, device=dev_t)
    o_align = torch.empty((n, max_lq), dtype=torch.int32, device=dev_t) if align else None
    if n and nq:
        dev = dev_t.index
        _lib.check(lib.ts_maxsim_passages_indexed_batch(_addr(q_packed), _addr(qo), nq, _addr(store), _addr(starts),
                                                        _addr(lens), _addr(co), H, _tensor_dtype(q_packed),
                                                        int(min(window, 1 << 30)), _addr(o_start), _addr(o_len),
                                                        _addr(o_score), _addr(o_align), max_lq, dev, _stream_ptr(dev)))
    return (o_start, o_len, o_score, o_align) if align else (o_start, o_len, o_score)


# ---- e4m3 token store (include/tristage.h) --------------------------------------------------
FP8_STORE_MAX_H = 2048   # the largest H whose query image fits the streaming kernel's LDS budget (at H % 16 == 0)


def fp8_store_supported(H: int) -> bool:
    """Whether the e4m3-store MaxSim kernel takes rows of H elements (there is no general kernel behind it)."""
    return H > 0 and H % 16 == 0 and H <= FP8_STORE_MAX_H


def _is_fp8(t) -> bool:
    return t.dtype == _torch().float8_e4m3fn


def quantize_rows_fp8_reference(x):
    """The stored format of an e4m3 token store, in plain torch on the CPU: row x -> e4m3_rne(x * 2^k), k the largest
    integer with max|x_i| * 2^k <= 448 (taken from the exponent of max|x_i|, exact at powers of two), e4m3 subnormals
    kept; a zero row stores zeros, a row with a NaN or an Inf stores NaN (0x7F) in every element.  k is not kept: the
    stage-2 scores are cosines, which no positive per-row factor changes.  x [rows, H] of f32 / f16 / bf16 ->
    float8_e4m3fn [rows, H] on the CPU."""
    torch = _torch()
    x = x.detach().to("cpu", torch.float32)
    if x.dim() != 2:
        raise ValueError("quantize_rows_fp8: x must be [rows, H]")
    bad = ~torch.isfinite(x).all(dim=1)
    m = x.abs().amax(dim=1) if x.shape[1] else torch.zeros(x.shape[0])
    mant, e = torch.frexp(m)                      # m = mant * 2^e, mant in [0.5, 1); 448 = 0.875 * 2^9
    k = torch.where(mant <= 0.875, 9 - e, 8 - e)
    k = torch.where((m == 0) | bad, torch.zeros_like(k), k)
    # x * 2^k is exact in float64 (|k| <= 158) and, wherever it can round to a non-zero e4m3 value, in float32 too
    y = (x.double() * torch.pow(2.0, k.double()).unsqueeze(1)).float()
    y[bad] = 0.0
    q = y.to(torch.float8_e4m3fn)
    q.view(torch.uint8)[bad] = 0x7F
    return q


def quantize_rows_e4m3_fixed_reference(x, scale_log2: int = 8) -> np.ndarray:
    """The stored bytes of an fp8 FlatIPIndex, in numpy integer arithmetic: element x ->
    e4m3fn_rne(x * 2^scale_log2).  x * 2^s is taken in float32 (exact, or Inf on overflow); rounding is to nearest, ties
    to the even mantissa, on the float32 bits; e4m3 subnormals (multiples of 2^-9) are kept; magnitudes above 448 and
    +-Inf saturate to +-448 (0x7E / 0xFE); NaN stores 0x7F; the sign is kept, also of a zero.  There is no per-row
    scale: stage-1 scores are compared across rows.  x: f32 / f16 / bf16 array or tensor of any shape -> uint8 array."""
    if not 0 <= int(scale_log2) <= 15:
        raise ValueError(f"scale_log2 must be in 0 .. 15, got {scale_log2}")
    if _is_tensor(x):
        x = x.detach().to("cpu", _torch().float32).numpy()
    with np.errstate(over="ignore"):
        y = np.ascontiguousarray(x, dtype=np.float32) * np.float32(2.0 ** int(scale_log2))
    u = y.view(np.uint32).astype(np.int64)
    sign = (u >> 24) & 0x80
    a = u & 0x7FFFFFFF
    e = a >> 23
    # normal e4m3 values (|y| >= 2^-6): 20 mantissa bits dropped with round-to-nearest-even; exponent bias 127 -> 7
    normal = np.minimum(((a + 0x7FFFF + ((a >> 20) & 1)) >> 20) - 960, 0x7E)
    # subnormal: |y| * 2^9 rounded to nearest even, 0 .. 8 (8 is the byte of 2^-6)
    m = (a & 0x7FFFFF) | 0x800000
    sh = np.clip(141 - e, 1, 40)
    qv = m >> sh
    rem, half = m & ((np.int64(1) << sh) - 1), np.int64(1) << (sh - 1)
    sub = qv + ((rem > half) | ((rem == half) & ((qv & 1) == 1)))
    b = np.where(e >= 121, normal, np.where(e < 117, 0, sub)) | sign
    return np.where(a > 0x7F800000, 0x7F, b).astype(np.uint8)


def decode_rows_e4m3_fixed(b, scale_log2: int = 8) -> np.ndarray:
    """The values an fp8 FlatIPIndex scores and ``reconstruct_n`` returns: e4m3fn(b) * 2^-scale_log2 as float32 (exact;
    0x7F / 0xFF decode to NaN).  b: uint8 array."""
    b = np.asarray(b, dtype=np.uint8).astype(np.int64)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e.astype(np.float64) - 10))
    mag = np.where((b & 0x7F) == 0x7F, np.nan, mag)
    v = np.where(b & 0x80, -mag, mag) * 2.0 ** -int(scale_log2)
    return v.astype(np.float32)


MXFP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)   # the magnitudes of OCP e2m1, by 3-bit index


def _mxfp4_block_dims(dpad: int) -> np.ndarray:
    """[dpad // 32, 32]: the dimensions of scale block 2 g + h, k = 64 g + 16 m + 8 h + j in the order (m, j)."""
    g, h, m, j = np.meshgrid(np.arange(dpad // 64), np.arange(2), np.arange(4), np.arange(8), indexing="ij")
    return (64 * g + 16 * m + 8 * h + j).reshape(dpad // 32, 32)


def quantize_rows_mxfp4_reference(x):
    """The stored values of an fp4 FlatIPIndex, in numpy: OCP e2m1 elements with one E8M0 scale per
    32 elements.  x [n, d] (f32 / f16 / bf16 array or tensor; taken as float32, NaN as 0, +-Inf as +-FLT_MAX) is
    zero-padded to dpad, a multiple of 64.  Scale block (g, h), h = 0/1, holds the dimensions k = 64 g + 16 m + 8 h + j
    (m = 0..3, j = 0..7); its exponent e, column 2 g + h of ``exps``, is 0 for an all-zero block and otherwise
    floor(log2 amax) - 2 on the float32 bits of the block's largest magnitude, plus 1 if amax > 6 * 2^e, clamped to
    -100 .. 100 (the stored byte is e + 127).  Code = 8 * (sign bit of x) + the index of the value of
    :data:`MXFP4_GRID` nearest to |x| / 2^e, ties to the even index, values above 6 to index 7.
    Returns (codes uint8 [n, dpad], exps int8 [n, dpad // 32])."""
    if _is_tensor(x):
        x = x.detach().to("cpu", _torch().float32).numpy()
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("quantize_rows_mxfp4_reference: x must be [n, d]")
    n, d = x.shape
    dpad = -(-d // 64) * 64
    v = np.zeros((n, dpad), dtype=np.float32)
    v[:, :d] = x
    bits = v.view(np.uint32)
    mag = bits & np.uint32(0x7FFFFFFF)
    v[mag > 0x7F800000] = 0.0                                           # NaN -> +0
    inf = mag == 0x7F800000
    bits[inf] = (bits[inf] & np.uint32(0x80000000)) | np.uint32(0x7F7FFFFF)   # +-Inf -> +-FLT_MAX
    dims = _mxfp4_block_dims(dpad)
    blocks = v[:, dims]                                                  # [n, dpad // 32, 32]
    amax = np.abs(blocks).max(axis=2)
    a = amax.view(np.uint32).astype(np.int64)
    e = (a >> 23) - 127 - 2 + ((a & 0x7FFFFF) > 0x400000)               # (f32 subnormals land below the clamp)
    e = np.where(a == 0, 0, np.clip(e, -100, 100))
    # |x| * 2^-e in float32: exact, or underflows far below 0.25, or overflows far above 6
    with np.errstate(over="ignore", under="ignore"):
        y = np.abs(blocks) * np.ldexp(np.float32(1.0), -e).astype(np.float32)[:, :, None]
    f = np.float32
    idx = ((y > f(0.25)).astype(np.uint8) + (y >= f(0.75)) + (y > f(1.25)) + (y >= f(1.75)) + (y > f(2.5))
           + (y >= f(3.5)) + (y > f(5.0))).astype(np.uint8)
    code = idx | ((blocks.view(np.uint32) >> 28) & 8).astype(np.uint8)
    codes = np.zeros((n, dpad), dtype=np.uint8)
    codes[:, dims] = code
    return codes, e.astype(np.int8)


def decode_rows_mxfp4(codes, exps, d: int) -> np.ndarray:
    """The values an fp4 FlatIPIndex scores and ``reconstruct_n`` returns: sign * MXFP4_GRID[index] * 2^e as float32
    [n, d] (exact, also in bf16), from what :func:`quantize_rows_mxfp4_reference` returns."""
    codes = np.asarray(codes, dtype=np.uint8)
    exps = np.asarray(exps, dtype=np.int8)
    n, dpad = codes.shape
    if dpad % 64 or exps.shape != (n, dpad // 32) or not 0 < int(d) <= dpad:
        raise ValueError("decode_rows_mxfp4: codes [n, dpad], exps [n, dpad // 32], dpad % 64 == 0, 0 < d <= dpad")
    dims = _mxfp4_block_dims(dpad)
    mag = np.asarray(MXFP4_GRID, dtype=np.float32)[codes[:, dims] & 7]
    val = np.ldexp(mag, exps.astype(np.int32)[:, :, None]).astype(np.float32)
    val = np.where(codes[:, dims] & 8, -val, val)
    out = np.zeros((n, dpad), dtype=np.float32)
    out[:, dims] = val
    return np.ascontiguousarray(out[:, :int(d)])


def quantize_rows_fp8(x):
    """Rows -> the e4m3 token-store format (see quantize_rows_fp8_reference, which it equals bit for bit): the
    ts_quantize_rows_fp8 kernel for a GPU tensor, the torch reference for a CPU one.  x [rows, H] f32 / f16 / bf16."""
    torch = _torch()
    if x.dim() != 2:
        raise ValueError("quantize_rows_fp8: x must be [rows, H]")
    if not x.is_cuda:
        return quantize_rows_fp8_reference(x)
    lib = _lib.load()
    rows, H = int(x.shape[0]), int(x.shape[1])
    if H % 16 != 0:
        raise ValueError(f"quantize_rows_fp8: H = {H} is not a multiple of 16")
    x = x.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    out = torch.empty((rows, H), dtype=torch.float8_e4m3fn, device=x.device)
    if rows == 0:
        return out
    dev = x.device.index
    _lib.check(lib.ts_quantize_rows_fp8(_addr(x), _tensor_dtype(x), rows, H, _addr(out), dev, _stream_ptr(dev)))
    return out


def fp8_query_dtype(q_dtype):
    """The type a query keeps against an e4m3 store: its own if bf16 / f16, else bf16 (it is never quantised)."""
    torch = _torch()
    return q_dtype if q_dtype in (torch.float16, torch.bfloat16) else torch.bfloat16


def _maxsim_indexed_fp8(q, store, starts, lens, mode):
    torch = _torch()
    lib = _lib.load()
    q = q.to(fp8_query_dtype(q.dtype)).contiguous()
    starts = starts.to(device=q.device, dtype=torch.int64).contiguous()
    lens = lens.to(device=q.device, dtype=torch.int32).contiguous()
    n = starts.numel()
    out = torch.empty((n,), dtype=torch.float32, device=q.device)
    if n == 0:
        return out
    dev = q.device.index
    _lib.check(lib.ts_maxsim_indexed_fp8(_addr(q), _tensor_dtype(q), q.shape[0], _addr(store), _addr(starts),
                                         _addr(lens), n, q.shape[1], 0 if mode == "maxsim" else 1, _addr(out), dev,
                                         _stream_ptr(dev)))
    return out


def add_layernorm(x, residual, gamma, beta, eps: float, lp_dtype=None, want_f32: bool = True, prenorm: bool = False):
    """``LayerNorm(x + residual) * gamma + beta`` over the last dimension in ONE pass on the GPU (ts_add_layernorm):
    x [..., H] (fp32 / fp16 / bf16), residual fp32 of the same shape or None, gamma fp32 [H], beta fp32 [H] or None.
    Returns (y as fp32 or None, y in ``lp_dtype`` or None) — the next residual and the next GEMM's input.
    ``prenorm=True`` (ts_add_prenorm, pre-LN models): the fp32 result is ``x + residual`` — the residual stream — and the
    ``lp_dtype`` one its LayerNorm."""
    torch = _torch()
    lib = _lib.load()
    H = int(x.shape[-1])
    x = x.contiguous()
    rows = x.numel() // H
    if residual is not None:
        residual = residual.contiguous()
        if residual.dtype != torch.float32 or residual.shape != x.shape:
            raise ValueError("residual must be float32 with x's shape")
    gamma = gamma.detach().contiguous()
    beta = beta.detach().contiguous() if beta is not None else None
    for t in (gamma, beta):
        if t is not None and (t.dtype != torch.float32 or t.numel() != H or t.device != x.device):
            raise ValueError("gamma / beta must be float32 [H] on x's device")
    out32 = torch.empty(x.shape, dtype=torch.float32, device=x.device) if want_f32 else None
    outlp = torch.empty(x.shape, dtype=lp_dtype, device=x.device) if lp_dtype is not None else None
    dev = x.device.index
    fn = lib.ts_add_prenorm if prenorm else lib.ts_add_layernorm
    _lib.check(fn(_addr(x), _tensor_dtype(x), _addr(residual), _addr(gamma), _addr(beta), float(eps), rows, H,
                  _addr(out32), _addr(outlp), _tensor_dtype(outlp) if outlp is not None else _lib.TS_BF16, dev,
                  _stream_ptr(dev)))
    return out32, outlp


def attention_varlen(qkv, lens, heads: int, out=None, scale: Optional[float] = None, window: int = 0, rope=None,
                     offs=None, max_len: Optional[int] = None):
    """Self-attention of a right-padded batch on the GPU (ts_attention_varlen): ``qkv`` [B, L, 3*heads*dh] (fp16 / bf16,
    the fused projection's output, read in place), ``lens`` int32 [B] on the device.  Returns [B, L, heads*dh]; rows at
    padded positions are zeros (``out`` given: left as they are).  ``window`` > 0: keys within that distance only.
    ``rope`` = (cos, sin) float32 [L, dh]: rotary embedding applied to q and k on the fly (qkv is not modified).
    PACKED batches: ``qkv`` [T, 3*heads*dh] with ``offs`` int32 [B] (first token of each sequence, on the device) and
    ``max_len`` >= every length; returns [T, heads*dh]."""
    torch = _torch()
    lib = _lib.load()
    packed = offs is not None
    if packed:
        if qkv.dim() != 2 or max_len is None:
            raise ValueError("a packed batch is qkv [T, 3 * heads * head_dim] with offs and max_len")
        T, W = (int(v) for v in qkv.shape)
        B, L = int(lens.numel()), int(max_len)
        if offs.dtype != torch.int32 or offs.numel() != B or offs.device != qkv.device:
            raise ValueError("offs must be int32 [B] on qkv's device")
    else:
        B, L, W = (int(v) for v in qkv.shape)
    if W % (3 * heads):
        raise ValueError("last dimension must be 3 * heads * head_dim")
    dh = W // (3 * heads)
    if not qkv.is_contiguous() or lens.dtype != torch.int32 or lens.numel() != B or lens.device != qkv.device:
        raise ValueError("qkv must be contiguous and lens int32 [B] on the same device")
    if out is None:
        out = torch.zeros(((T,) if packed else (B, L)) + (heads * dh,), dtype=qkv.dtype, device=qkv.device)
    dev = qkv.device.index
    cos = sin = None
    if rope is not None:
        cos, sin = rope
        for t in (cos, sin):
            if (t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < L or t.shape[1] != dh or not t.is_contiguous()
                    or t.device != qkv.device):
                raise ValueError("rope tables must be contiguous float32 [>= L, head_dim] on qkv's device")
    _lib.check(lib.ts_attention_varlen(_addr(qkv), _addr(lens), B, L, heads, dh, _tensor_dtype(qkv),
                                       float(scale if scale is not None else dh ** -0.5), int(window), _addr(cos),
                                       _addr(sin), _addr(offs), _addr(out), dev, _stream_ptr(dev)))
    return out


def rope_inplace(qkv, cos, sin, heads: int):
    """Rotary position embedding of the q and k thirds of ``qkv`` [B, L, 3*heads*dh] (fp16 / bf16) in place
    (ts_rope_inplace); ``cos`` / ``sin`` float32 [L, dh]."""
    torch = _torch()
    lib = _lib.load()
    B, L, W = (int(v) for v in qkv.shape)
    dh = W // (3 * heads)
    if W != 3 * heads * dh or not qkv.is_contiguous():
        raise ValueError("qkv must be contiguous [B, L, 3 * heads * head_dim]")
    for t in (cos, sin):
        if t.dtype != torch.float32 or tuple(t.shape) != (L, dh) or not t.is_contiguous() or t.device != qkv.device:
            raise ValueError("cos / sin must be contiguous float32 [L, head_dim] on qkv's device")
    dev = qkv.device.index
    _lib.check(lib.ts_rope_inplace(_addr(qkv), _tensor_dtype(qkv), _addr(cos), _addr(sin), B, L, heads, dh, dev,
                                   _stream_ptr(dev)))
    return qkv


def geglu(u):
    """``gelu(u[..., :I]) * u[..., I:]`` for u [..., 2 I] (fp16 / bf16) in one pass on the GPU (ts_geglu)."""
    torch = _torch()
    lib = _lib.load()
    if not u.is_contiguous() or u.shape[-1] % 2:
        raise ValueError("u must be contiguous with an even last dimension")
    I = int(u.shape[-1]) // 2
    out = torch.empty(tuple(u.shape[:-1]) + (I,), dtype=u.dtype, device=u.device)
    dev = u.device.index
    _lib.check(lib.ts_geglu(_addr(u), _tensor_dtype(u), u.numel() // (2 * I), I, _addr(out), dev, _stream_ptr(dev)))
    return out


def embed_layernorm(ids, pos_ids, type_ids, word, pos, typ, gamma, beta, eps: float, lp_dtype=None, want_f32: bool = True):
    """The embedding layer of a BERT-family model in one pass on the GPU (ts_embed_layernorm):
    ``LayerNorm((word[ids] + typ[type_ids]) + pos[pos_ids])``; ids / pos_ids / type_ids int64 of one shape (type_ids None =
    type 0), tables fp32 [*, H].  Indices must be in range (the caller's tokenizer guarantees it).  Returns (fp32 or None,
    ``lp_dtype`` copy or None) of shape ids.shape + (H,)."""
    torch = _torch()
    lib = _lib.load()
    H = int(word.shape[-1])
    tabs = [t.detach() if t is not None else None for t in (word, pos, typ, gamma, beta)]
    if any(t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != ids.device) for t in tabs):
        raise ValueError("embedding tables and LayerNorm parameters must be contiguous float32 on the ids' device")
    if any(t.dim() != 2 or t.shape[-1] != H for t in tabs[:3]) or tabs[3].numel() != H or (tabs[4] is not None and tabs[4].numel() != H):
        raise ValueError("embedding tables must be [*, H] and gamma / beta [H]")
    idx = [ids.contiguous(), pos_ids.contiguous(), type_ids.contiguous() if type_ids is not None else None]
    if any(t is not None and (t.dtype != torch.int64 or t.shape != ids.shape) for t in idx):
        raise ValueError("ids, pos_ids and type_ids must be int64 of one shape")
    shape = tuple(ids.shape) + (H,)
    out32 = torch.empty(shape, dtype=torch.float32, device=ids.device) if want_f32 else None
    outlp = torch.empty(shape, dtype=lp_dtype, device=ids.device) if lp_dtype is not None else None
    dev = ids.device.index
    _lib.check(lib.ts_embed_layernorm(_addr(idx[0]), _addr(idx[1]), _addr(idx[2]), _addr(tabs[0]), _addr(tabs[1]),
                                      _addr(tabs[2]), _addr(tabs[3]), _addr(tabs[4]), float(eps), ids.numel(), H,
                                      _addr(out32), _addr(outlp),
                                      _tensor_dtype(outlp) if outlp is not None else _lib.TS_BF16, dev,
                                      _stream_ptr(dev)))
    return out32, outlp


def mlp_add_layernorm(up: "TiledLinear", down: "TiledLinear", x, residual, gamma, beta, eps: float, want_f32: bool = True):
    """``LayerNorm(down(gelu(up(x))) + residual) * gamma + beta`` — BertIntermediate + BertOutput — in ONE kernel
    (ts_mlp_add_layernorm): the intermediate never goes to HBM.  ``up`` [I, H] / ``down`` [H, I] are TiledLinear weights
    (``mlp_usable(up, down)``), x [..., H] of their dtype, residual fp32 [..., H] or None, gamma / beta fp32 [H].  Returns
    (y fp32 or None, y in the weights' dtype) — bit-identical to ``down.add_layernorm(up(x, gelu=True), residual, ...)``."""
    torch = _torch()
    if not mlp_usable(up, down):
        raise ValueError("mlp_add_layernorm takes an up weight [I, 384] and a down weight [384, I] with I % 384 == 0 (mlp_usable)")
    H = up.K
    if x.dtype != up.dtype or x.shape[-1] != H or not x.is_contiguous() or x.device != up.device:
        raise ValueError("x must be a contiguous [..., H] tensor of the weights' dtype on their device")
    if residual is not None:
        residual = residual.contiguous()
        if residual.dtype != torch.float32 or residual.shape != x.shape or residual.device != x.device:
            raise ValueError("residual must be float32 with x's shape on x's device")
    gamma = gamma.detach().contiguous()
    beta = beta.detach().contiguous() if beta is not None else None
    for t in (gamma, beta):
        if t is not None and (t.dtype != torch.float32 or t.numel() != H or t.device != x.device):
            raise ValueError("gamma / beta must be float32 [H] on x's device")
    out32 = torch.empty(x.shape, dtype=torch.float32, device=x.device) if want_f32 else None
    outlp = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    dev = x.device.index
    _lib.check(_lib.load().ts_mlp_add_layernorm(_addr(up.tiled), _addr(up.bias), _addr(down.tiled), _addr(down.bias),
                                                _addr(x), _addr(residual), _addr(gamma), _addr(beta), float(eps),
                                                _tensor_dtype(x), x.numel() // H, H, up.N, _addr(out32), _addr(outlp),
                                                dev, _stream_ptr(dev)))
    return out32, outlp


def mlp_usable(up, down) -> bool:
    """Whether ``mlp_add_layernorm`` takes this pair of TiledLinear weights: hidden size 384 (a workgroup owns whole rows),
    intermediate size a multiple of 384, same dtype and device."""
    return (up is not None and down is not None and up.K == 384 and down.N == 384 and up.N == down.K and up.N % 384 == 0
            and up.dtype == down.dtype and up.device == down.device)


class TiledLinear:
    """A torch.nn.Linear-style weight [N, K] (fp16 / bf16, on the GPU) re-tiled once for ts_linear_act: ``y = act(x W^T + b)``
    with the weight streamed from L2 and x's rows in LDS — for reduction dimensions up to 384 (MiniLM-class encoders), where
    the library GEMM re-reads its operands many times and this kernel is 1.2-1.5x faster; at K = 768 the library's
    stream-K GEMMs (1.16 PFLOP/s) win and the encoders keep them.  ``TiledLinear.usable(N, K)`` says
    whether a shape qualifies."""

    @staticmethod
    def usable(N: int, K: int) -> bool:
        return N % 32 == 0 and K % 128 == 0 and K <= 384

    @staticmethod
    def usable_with_layernorm(N: int, K: int) -> bool:
        """Shapes ``add_layernorm`` takes: a workgroup owns whole rows of the output (N <= 384), the reduction is walked
        in chunks of 384 (the attention-output and feed-forward down projections of MiniLM-class encoders)."""
        return N % 32 == 0 and N <= 384 and K % 384 == 0

    def __init__(self, weight, bias=None, with_layernorm: bool = False):
        torch = _torch()
        lib = _lib.load()
        w = weight.detach().contiguous()
        self.N, self.K = int(w.shape[0]), int(w.shape[1])
        ok = self.usable_with_layernorm(self.N, self.K) if with_layernorm else self.usable(self.N, self.K)
        if not w.is_cuda or w.dtype not in (torch.float16, torch.bfloat16) or not ok:
            raise ValueError("TiledLinear takes a 16-bit CUDA weight [N, K] with N % 32 == 0, K % 128 == 0, K <= 384 "
                             "(with_layernorm: N <= 384, K % 384 == 0)")
        self.dtype, self.device = w.dtype, w.device
        self.bias = bias.detach().to(w.dtype).contiguous() if bias is not None else None
        self.tiled = torch.empty_like(w)
        dev = w.device.index
        _lib.check(lib.ts_linear_tile_weight(_addr(w), _tensor_dtype(w), self.N, self.K, _addr(self.tiled), dev,
                                             _stream_ptr(dev)))

    def __call__(self, x, gelu: bool = False):
        torch = _torch()
        if x.dtype != self.dtype or x.shape[-1] != self.K or not x.is_contiguous() or x.device != self.device:
            raise ValueError("x must be a contiguous [..., K] tensor of the weight's dtype on its device")
        out = torch.empty(tuple(x.shape[:-1]) + (self.N,), dtype=x.dtype, device=x.device)
        dev = x.device.index
        _lib.check(_lib.load().ts_linear_act(_addr(self.tiled), _addr(x), _addr(self.bias), _tensor_dtype(x),
                                             x.numel() // self.K, self.N, self.K, 1 if gelu else 0, _addr(out), dev,
                                             _stream_ptr(dev)))
        return out

    def add_layernorm(self, x, residual, gamma, beta, eps: float, want_f32: bool = True, gelu_input: bool = False):
        """``LayerNorm(linear(x) + residual) * gamma + beta`` in ONE kernel (ts_linear_add_layernorm; BertSelfOutput /
        BertOutput): x [..., K] of the weight's dtype, residual fp32 [..., N] or None, gamma / beta fp32 [N].  Returns
        (y fp32 or None, y in the weight's dtype) — bit-identical to ``add_layernorm(self(x), residual, ...)``.
        ``gelu_input=True``: ``linear(gelu(x))`` — x is the up projection's output BEFORE its activation, the erf GELU (and
        its rounding to the 16-bit type) is applied while the rows are staged: bit-identical to passing
        ``F.gelu``-of-x as produced by ``TiledLinear.__call__(..., gelu=True)``."""
        torch = _torch()
        if not self.usable_with_layernorm(self.N, self.K):
            raise ValueError("this weight's shape has no fused LayerNorm kernel (TiledLinear.usable_with_layernorm)")
        if x.dtype != self.dtype or x.shape[-1] != self.K or not x.is_contiguous() or x.device != self.device:
            raise ValueError("x must be a contiguous [..., K] tensor of the weight's dtype on its device")
        shape = tuple(x.shape[:-1]) + (self.N,)
        if residual is not None:
            residual = residual.contiguous()
            if residual.dtype != torch.float32 or tuple(residual.shape) != shape or residual.device != x.device:
                raise ValueError("residual must be float32 [..., N] on x's device")
        gamma = gamma.detach().contiguous()
        beta = beta.detach().contiguous() if beta is not None else None
        for t in (gamma, beta):
            if t is not None and (t.dtype != torch.float32 or t.numel() != self.N or t.device != x.device):
                raise ValueError("gamma / beta must be float32 [N] on x's device")
        out32 = torch.empty(shape, dtype=torch.float32, device=x.device) if want_f32 else None
        outlp = torch.empty(shape, dtype=x.dtype, device=x.device)
        dev = x.device.index
        _lib.check(_lib.load().ts_linear_add_layernorm(_addr(self.tiled), _addr(x), _addr(self.bias), _addr(residual),
                                                       _addr(gamma), _addr(beta), float(eps), _tensor_dtype(x),
                                                       x.numel() // self.K, self.N, self.K, 1 if gelu_input else 0,
                                                       _addr(out32), _addr(outlp), dev, _stream_ptr(dev)))
        return out32, outlp


class IVFFlatIndex(_IndexBase):
    """Inverted-file index over f16 / bf16 rows resident in MI355X HBM: FAISS ``IndexIVFFlat`` with inner product
    (reference src/stage1_retriever.py:256-283, ``nlist`` lists, ``nprobe`` probed per query).

    ``train`` runs spherical k-means on the device; ``search`` returns the exact top-k over the rows of the query's
    ``nprobe`` probed lists, with scores bit-identical to :class:`FlatIPIndex` on the same rows and ties by ascending id.
    Inputs may be numpy arrays or torch tensors; host inputs are copied to the index's GPU first."""

    _DESTROY = "ts_ivf_destroy"
    MAX_KERNEL_K = 16384

    def __init__(self, d: int, nlist: int, dtype: str = "f16", device: int = 0, nprobe: int = 10):
        if _NAME_TO_DTYPE.get(dtype) == _lib.TS_FP8_E4M3:
            raise NotImplementedError("IVFFlatIndex has no fp8 storage (fp8 is a flat-index storage dtype)")
        if _NAME_TO_DTYPE.get(dtype) == _lib.TS_MXFP4_E2M1:
            raise NotImplementedError("IVFFlatIndex has no fp4 storage (fp4 is a flat-index storage dtype)")
        if dtype not in _NAME_TO_DTYPE or _NAME_TO_DTYPE[dtype] == _lib.TS_F32:
            raise ValueError(f"IVF storage dtype must be f16 or bf16, got {dtype!r}")
        self._lib = _lib.load()
        self.d = int(d)
        self.nlist = int(nlist)
        self.nprobe = int(nprobe)
        self.device = int(device)
        self.storage_dtype = _DTYPE_NAME[_NAME_TO_DTYPE[dtype]]
        self.seed = 1234
        self.niter = 25
        self.objective = []   # per k-means iteration: sum over the training points of their best centroid score
        self._id_offset = 0
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.ts_ivf_create(self.d, self.nlist, _NAME_TO_DTYPE[dtype], self.device,
                                           ctypes.byref(self._h)))

    # -- helpers -------------------------------------------------------------
    def _dev(self, x, what: str):
        """The upload policy for [n, d] ``what``: (tensor on the index's GPU, dtype code, n, whether x was a CUDA tensor)."""
        return _device_query(x, self.d, self.device, what, "n")

    def _stream(self) -> int:
        return _stream_ptr(self.device)

    # -- FAISS duck type -----------------------------------------------------
    @property
    def ntotal(self) -> int:
        return int(self._lib.ts_ivf_ntotal(self._h))

    @property
    def is_trained(self) -> bool:
        return int(self._lib.ts_ivf_is_trained(self._h)) == 1

    @property
    def nlive(self) -> int:
        """Rows not removed (``ntotal`` counts every id assigned since the last :meth:`compact` / :meth:`reset`)."""
        return int(self.list_sizes().sum())

    def remove_ids(self, ids) -> int:
        """:meth:`FlatIPIndex.remove_ids` for the IVF index: removed rows leave their lists (holes stay until
        :meth:`compact`).  Returns how many rows were removed."""
        arr = _id_array(ids)
        n = ctypes.c_int64(0)
        _lib.check(self._lib.ts_remove_ivf(self._h, _addr(arr), int(arr.shape[0]), ctypes.byref(n), self._stream()))
        return int(n.value)

    def update_rows(self, ids, x, normalize: bool = False) -> None:
        """:meth:`FlatIPIndex.update_rows` for the IVF index: each row leaves its list, is assigned by the quantizer as
        :meth:`add` assigns a new row and joins the end of its new list under its old id (the hole stays, as after a
        removal, until :meth:`compact`).  All or nothing: an id out of range, given twice or removed raises
        ``ValueError``."""
        arr = _id_array(ids)
        x, x_dtype, n, _ = self._dev(x, "rows")
        if n != arr.shape[0]:
            _bad_shape(arr.shape[0], self.d, "rows", x.shape)
        _update_call(self._lib.ts_update_ivf, self._h, arr, x, x_dtype, _lib.TS_FLAG_NORMALIZE if normalize else 0,
                     self._stream())

    def compact(self) -> np.ndarray:
        """:meth:`FlatIPIndex.compact` for the IVF index: the live rows are renumbered densely in id order, the holes of
        removals and updates are closed and ``ntotal`` becomes :attr:`nlive`.  Rows stay in their lists and the
        centroids and the id offset stay; afterwards the index is the one a fresh index with the same centroids holds
        after ``add`` of the surviving rows.  Returns the old -> new map int64 [old ntotal] (-1 =
        removed), monotone, so ties keep their order."""
        n = self.ntotal
        out = np.empty(max(n, 1), dtype=np.int64)
        _lib.check(self._lib.ts_compact_ivf(self._h, _addr(out), self._stream()))
        return out[:n]

    def train(self, x, seed: Optional[int] = None, niter: Optional[int] = None) -> None:
        x, x_dtype, n, _ = self._dev(x, "training points")
        if n < self.nlist:
            raise ValueError(f"{n} training points for nlist={self.nlist}: need at least nlist")
        it = self.niter if niter is None else int(niter)
        obj = (ctypes.c_double * max(it, 1))()
        _lib.check(self._lib.ts_ivf_train(self._h, _addr(x), n, x_dtype, int(self.seed if seed is None else seed), it,
                                          obj, self._stream()))
        self.objective = [float(obj[i]) for i in range(it)]

    def add(self, x, normalize: bool = False) -> None:
        if not self.is_trained:
            raise RuntimeError("IVFFlatIndex.add before train(): the index has no centroids")
        x, x_dtype, n, _ = self._dev(x, "rows")
        _lib.check(self._lib.ts_ivf_add(self._h, _addr(x), n, x_dtype, _lib.TS_FLAG_NORMALIZE if normalize else 0,
                                        self._stream()))

    def reset(self) -> None:
        _lib.check(self._lib.ts_ivf_reset(self._h))

    def set_id_offset(self, offset: int) -> None:
        _lib.check(self._lib.ts_ivf_set_id_offset(self._h, int(offset)))
        self._id_offset = int(offset)

    @property
    def centroids(self) -> np.ndarray:
        """[nlist, d] float32 (host)."""
        torch = _torch()
        out = torch.empty((self.nlist, self.d), dtype=torch.float32, device=torch.device("cuda", self.device))
        _lib.check(self._lib.ts_ivf_get_centroids(self._h, _addr(out), self._stream()))
        return out.cpu().numpy()

    def set_centroids(self, c) -> None:
        """Load trained centroids [nlist, d] (no training); the index must be empty."""
        c = self._dev(c, "centroids")[0].float().contiguous()
        if c.shape[0] != self.nlist:
            raise ValueError(f"expected {self.nlist} centroids, got {c.shape[0]}")
        _lib.check(self._lib.ts_ivf_set_centroids(self._h, _addr(c), self._stream()))
        _torch().cuda.current_stream(self.device).synchronize()

    def list_sizes(self) -> np.ndarray:
        out = np.zeros(self.nlist, dtype=np.int64)
        _lib.check(self._lib.ts_ivf_list_sizes(self._h, _addr(out)))
        return out

    def probe(self, q, nprobe: Optional[int] = None):
        """``(scores float32 [B, nprobe], lists int64 [B, nprobe])``: the lists a search probes, best first."""
        q, q_dtype, B, on_gpu = self._dev(q, "queries")
        p = min(self.nprobe if nprobe is None else int(nprobe), self.nlist)
        if p <= 0:
            raise ValueError("nprobe must be positive")
        S, L = _outputs(None, B, p, q)
        _lib.check(self._lib.ts_ivf_probe(self._h, _addr(q), B, q_dtype, p, _addr(S), _addr(L), self._stream()))
        return (S, L) if on_gpu else (S.cpu().numpy(), L.cpu().numpy())

    def search(self, q, k: int, async_: bool = False, out=None, allowed=None, nprobe: Optional[int] = None):
        """Top-``k`` over the rows of each query's probed lists (FAISS convention, -1 / -FLT_MAX padded).  numpy in
        -> numpy out, CUDA tensor in -> tensors out.  ``async_`` is accepted and completes synchronously (:meth:`finish`
        then has nothing to report)."""
        if allowed is not None:
            raise NotImplementedError("filtered search (allowed=) is not supported by IVFFlatIndex")
        k = int(k)
        if k <= 0:
            raise ValueError("k must be positive")
        if k > self.MAX_KERNEL_K:
            raise NotImplementedError(f"IVFFlatIndex.search: k={k} exceeds the select limit {self.MAX_KERNEL_K}")
        if not self.is_trained:
            raise RuntimeError("IVFFlatIndex.search before train()")
        if self.ntotal == 0:
            _raise_empty()
        q, q_dtype, B, on_gpu = self._dev(q, "queries")
        D, I = _outputs(out, B, k, q)
        p = self.nprobe if nprobe is None else int(nprobe)
        if p <= 0:
            raise ValueError("nprobe must be positive")
        _lib.check(self._lib.ts_ivf_search(self._h, _addr(q), B, q_dtype, k, min(p, self.nlist), _addr(D), _addr(I),
                                           self._stream()))
        return (D, I) if on_gpu else (D.cpu().numpy(), I.cpu().numpy())

    def mmr(self, ids, relevance, k: int, lambda_mult: float = 0.5):
        """:meth:`FlatIPIndex.mmr` over the rows of this index (ids go through the id-to-slot table on the device)."""
        return _mmr_call(self, "ts_mmr_ivf", ids, relevance, k, lambda_mult)

    def search_mmr(self, q, k: int, fetch_k: Optional[int] = None, lambda_mult: float = 0.5,
                   nprobe: Optional[int] = None):
        """``search(q, fetch_k, nprobe=nprobe)`` followed by :meth:`mmr` on the same stream."""
        return self._search_mmr(q, k, fetch_k, lambda_mult, nprobe=nprobe)

    def search_prefix(self, q, k: int, dims: int, allowed=None):
        raise NotImplementedError("funnel search is not supported on an IVF index (its lists hold whole rows; use a flat index)")

    def rescore(self, q, ids, k: Optional[int] = None):
        raise NotImplementedError("funnel search is not supported on an IVF index (its lists hold whole rows; use a flat index)")

    def search_funnel(self, q, k: int, dims: int, fetch_k: Optional[int] = None, allowed=None):
        raise NotImplementedError("funnel search is not supported on an IVF index (its lists hold whole rows; use a flat index)")

    def search_biased(self, q, k: int, bias, allowed=None, exact_dense: bool = False, check_finite: bool = True):
        raise NotImplementedError("boosted search (search_biased) is not supported on an IVF index (use a flat index)")

    def search_grouped(self, q, k: int, groups, group_size: int = 1, fetch_k: Optional[int] = None,
                       nprobe: Optional[int] = None):
        """:meth:`FlatIPIndex.search_grouped` over ``search(q, fetch, nprobe=nprobe)``: the rows a query can reach are
        those of its probed lists, and a list is exhaustive when it holds all of them."""
        return self._search_grouped(q, k, groups, group_size, fetch_k, nprobe=nprobe)

    def finish(self):
        """Asynchronous searches complete synchronously here: nothing is pending, no ticket failed."""
        return []

    def flush(self) -> None:
        return None

    def reconstruct_n(self, i0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Rows [i0, i0+n) in id order as float32 (after storage rounding)."""
        torch = _torch()
        if n is None:
            n = self.ntotal - i0
        out = torch.empty((max(n, 0), self.d), dtype=torch.float32, device=torch.device("cuda", self.device))
        if n:
            _lib.check(self._lib.ts_ivf_reconstruct(self._h, int(i0), int(n), _addr(out), self._stream()))
        return out.cpu().numpy()

    def last_search_info(self) -> dict:
        info = (ctypes.c_int64 * 4)()
        _lib.check(self._lib.ts_ivf_last_search_info(self._h, info))
        return {"passes": int(info[0]), "filter_passes": int(info[1]), "redone": int(info[2]),
                "live_blocks": int(info[3])}
