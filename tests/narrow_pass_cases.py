"""The case table of the narrow-pass tests: every stage-1 entry point where a pass holds 32 queries.

A stage-1 call is cut into passes of ``queries_per_pass`` queries (ts_index.hip): 64 while the 64-query image fits the
LDS, 32 above d = 1024 (f16 / bf16 / fp8 / fp4 storage) and above d = 512 (fp32).  In the 32-query regime query 32
starts a new pass, a new workspace set and a new slice of every per-query argument (masks, radii, limits, outputs,
the bias counters), and an asynchronous call of 128 queries is the library's maximum of four passes.  This file holds
what needs no GPU: the shapes, the exactly summable inputs (tests/exact_inputs.py), the variants and their models,
and the Python mirror of the chunk rule of ``ts_index_rescore``.  tests/test_narrow_pass_host.py checks all of it,
tests/test_narrow_pass_gpu.py runs it.

As in tests/handle_reuse_cases.py (4.24) the float64 score matrix IS the reference, bit for bit, and every model is an
existing one fed with rows of that matrix.  Which storage type takes which variant is read from that file's
``SUPPORTED`` table: every variant here names the row of that table it is ``like``.

No torch import at module level."""
import functools
from typing import NamedTuple

import numpy as np

import bias_model as bm
import exact_inputs as ex
import funnel_model as fu
import group_model as gm
import handle_reuse_cases as hc
import range_model as rm

N_DENSE = ex.N_DENSE          # 33 row blocks and a partial one: every pass is dense
N_FILTER = ex.N_FILTER        # just above the filter path's floor, a partial last block
N_IVF = ex.N_IVF
NQ = 130                      # ordinary queries of a pool (B <= 129); query NQ is the tie query where there is one
TIE_Q = NQ
TIE_N = 17_000                # rows [tie0, tie0 + TIE_N) of a corpus with a tie block are copies of one row (> 16384 slots)
TIE0 = 20_011                 # ... of the one-launch corpora (f16 / bf16)
TIE0_FILTER = 5_003           # ... of the fp32, fp8 and fp4 filter corpora
CAND_CAP = rm.CAND_CAP
SYNC_B = (32, 33, 64, 65)     # one full pass; a second pass of one query; two full passes; a third pass
ASYNC_B = (128, 129)          # the library's four passes; the Python slice behind them
FLT_MAX = ex.FLT_MAX
NLIST = 8


class Ix(NamedTuple):
    storage: str
    d: int
    rows: str        # dense | filter | one (ex.one_launch_rows of the device: 16-bit storage at d = 1100 only)

    @property
    def id(self):
        return f"{self.storage}-{self.d}-{self.rows}"


# 16-bit storage: d = 1100 pads to 1152, the first width of the regime (a zero tail); d = 2176 is the limit.  fp32: the
# split scan (600) and the exact-f32 kernel (776).  fp8 / fp4: 1280 and the limit 2048.
INDEXES = (
    Ix("f16", 1100, "dense"), Ix("f16", 2176, "dense"), Ix("f16", 1100, "filter"), Ix("f16", 1100, "one"),
    Ix("bf16", 1100, "dense"), Ix("bf16", 2176, "dense"), Ix("bf16", 2176, "filter"), Ix("bf16", 1100, "one"),
    Ix("f32", 600, "dense"), Ix("f32", 776, "dense"), Ix("f32", 776, "filter"),
    Ix("fp8", 1280, "dense"), Ix("fp8", 2048, "dense"), Ix("fp8", 2048, "filter"),
    Ix("fp4", 1280, "dense"), Ix("fp4", 2048, "dense"), Ix("fp4", 1280, "filter"),
)
CONTROL = Ix("f16", 1024, "dense")        # the widest 64-query index: the same calls report half the passes
# ts_ivf_create takes d <= 1088: its quantizer is an fp32 index, whose 32-query image fits the LDS up to there.
# d = 1030 pads to 1152 (a zero tail), d = 1088 is that limit; both lie above 1024, so an IVF pass holds 32 queries.
IVF_CASES = (("f16", 1030), ("bf16", 1088))
IVF_REFUSED_D = 1100
IVF_N = (N_IVF, N_FILTER)
IVF_NPROBE = (1, 3, 8)


def queries_per_pass(storage, d):
    """The host rule (ts_index.hip ``queries_per_pass``) by its documented border."""
    return 64 if d <= (512 if storage == "f32" else 1024) else 32


def n_rows(ix, num_cus=256):
    return {"dense": N_DENSE, "filter": N_FILTER, "one": ex.one_launch_rows(num_cus)}[ix.rows]


# ------------------------------------------------------------------------------------------------------------ inputs
class Data:
    """corpus float32 [n, d] (what reconstruct_n() must return), queries float32 [NQ (+ 1), d], the unit of
    exact_inputs, S float64 [queries, n]: the exact scores.  ``Sp(dims)``: over the first ``dims`` dimensions."""

    def __init__(self, corpus, queries, unit, tie0=None):
        self.corpus, self.queries, self.unit, self.tie0 = corpus, queries, unit, tie0
        self.n, self.d = corpus.shape
        self.S = hc.chunked_scores(corpus, queries)
        for a in (corpus, queries, self.S):
            a.setflags(write=False)
        self._sp = {}

    def Sp(self, dims):
        if dims not in self._sp:
            self._sp[dims] = hc.chunked_scores(self.corpus, self.queries, dims)
            self._sp[dims].setflags(write=False)
        return self._sp[dims]


def gen_rows(storage, n, d, nq, seed=25):
    """handle_reuse_cases._rows for any (n, d): integers in [-63, 63] on both sides (exact in f16, bf16 and f32); fp8:
    the e4m3 integers |v| <= 15 at scale 0; fp4: the e2m1 grid with one +-6 in each scale block."""
    c, q, unit = ex.gen_ints(n, d, nq, seed=seed)
    if storage == "fp8":
        c = np.random.default_rng([seed, 8]).integers(-15, 16, size=(n, d)).astype(np.float32)
    if storage == "fp4":
        rng = np.random.default_rng([seed, 4])
        c = hc.FP4_GRID[rng.integers(0, 8, size=(n, d))] * (rng.integers(0, 2, size=(n, d)) * 2 - 1).astype(np.float32)
        for k0 in (0, 8):
            c[:, k0::64] = np.float32(6.0) * (rng.integers(0, 2, size=c[:, k0::64].shape) * 2 - 1)
        unit = 0.5        # integers times multiples of 0.5
    return np.ascontiguousarray(c, dtype=np.float32), q, unit


@functools.lru_cache(maxsize=3)
def _data(kind, d, n, tie0=None, prefix=False):
    c, q, unit = gen_rows(kind, n, d, NQ)
    if tie0 is not None:
        row = c[tie0].copy()
        if prefix:
            row[:1024] = 0.0      # every prefix pass scores the copied row 0
        c[tie0:tie0 + TIE_N] = row
        if kind == "fp4":
            unit = 0.25           # the tie query is a corpus row: multiples of 0.5 on both sides
        dot = q.astype(np.float64) @ row.astype(np.float64)
        q = np.where(dot[:, None] > 0, -q, q).astype(np.float32)      # every ordinary query scores it below zero
        q = np.concatenate([q, row[None, :]])
    return Data(c, q, unit, tie0)


def tie0_of(ix):
    """Where the index's corpus carries its tie block (None: it has none).  f16 / bf16 carry it in the one-launch
    corpus, whose prefix passes must score it 0; the other storage types, which have no one-launch corpus here, in
    their filter corpus, where the repair of an overflowing pass is that of the five-launch filter scan."""
    if ix.rows == "one":
        return TIE0
    if ix.rows == "filter" and ix.storage in ("f32", "fp8", "fp4"):
        return TIE0_FILTER
    return None


def data(ix, num_cus=256):
    kind = "ints" if ix.storage in ("f16", "bf16", "f32") else ix.storage
    return _data(kind, ix.d, n_rows(ix, num_cus), tie0_of(ix), ix.storage in ("f16", "bf16"))


@functools.lru_cache(maxsize=None)
def aux(name, n):
    """The masks, the bias, the group table and the live set of an index of ``n`` rows."""
    rng = np.random.default_rng([25, n, sum(map(ord, name))])
    if name == "m30":
        out = rng.random(n) < 0.3
    elif name == "m50":
        out = rng.random(n) < 0.5
    elif name == "mod5":
        out = np.arange(n) % 5 == 0
    elif name == "few":                                   # 37 rows: fewer than any k it is used with
        out = np.zeros(n, dtype=bool)
        out[rng.choice(n, size=37, replace=False)] = True
    elif name == "b":                                     # integer-valued: the f32 sum score + bias is exact
        out = rng.integers(-2000, 2001, size=n).astype(np.float32)
        if n > TIE0 + TIE_N:
            out[TIE0:TIE0 + TIE_N] = 5.0                  # (the one-launch corpus: the copies' ties stay ties)
    elif name == "groups":
        out = (np.arange(n) // 5).astype(np.int32)
    elif name == "live":                                  # the tombstone phase removes every third row
        out = np.arange(n) % 3 != 0
    else:
        raise KeyError(name)
    out.setflags(write=False)
    return out


MASKS = ("m30", "m50", "mod5", "few")


def allowed_names(spec, nq):
    """One mask name or None per query, or one name for all: how a per-query ``allowed`` lies across the pass border."""
    if spec is None or spec in MASKS:
        return spec
    if spec == "tail":            # the first pass is an ordinary pass inside a filtered call
        return [None if j < 32 else "m30" for j in range(nq)]
    if spec == "head":            # ... the second one is
        return ["m50" if j < 32 else None for j in range(nq)]
    if spec == "mix":             # three different masks and None interleaved
        return [("m30", "m50", None, "mod5")[j % 4] for j in range(nq)]
    raise KeyError(spec)


def allowed_of(spec, nq, n):
    names = allowed_names(spec, nq)
    if names is None or isinstance(names, str):
        return None if names is None else aux(names, n)
    return [None if m is None else aux(m, n) for m in names]


def ranks_of(nq):
    """A rank per query that differs on both sides of the pass border: 5 .. 109 results."""
    return 5 + 13 * (np.arange(nq) % 9)


# ---------------------------------------------------------------------------------------------------------- variants
class Variant(NamedTuple):
    name: str
    kind: str        # search | biased | range | prefix | funnel | scores | grouped | mmr | async
    like: str        # the row of handle_reuse_cases.SUPPORTED that says which storage types take it
    qi: tuple
    k: int
    opt: dict


def _q(a, b):
    return tuple(range(a, b))


def async_subs(kmax=None, tie=False):
    """The eight submissions of an asynchronous block, as hc.ASYNC_SUBS: large then small then large, with the
    library's maximum of four passes (128) and the Python slice behind it (129)."""
    subs = [(_q(0, 64), 100), (_q(0, 33), 10), (_q(5, 6), 1), (_q(0, 65), 500), (_q(20, 53), 100), (_q(0, 128), 7),
            (_q(1, 130), 257), (_q(40, 45), 100)]
    if tie:       # the tie query is query 35 of submission 4: the second pass of its submission
        subs[4] = (_q(60, 95) + (TIE_Q,) + _q(96, 100), 100)
    return tuple((qi, k if kmax is None else min(k, kmax)) for qi, k in subs)


TIE_SUB = 4


def variants(ix):
    """The variants of one index, before the storage type's refusals (``supported``)."""
    d, V = ix.d, []

    def add(name, kind, like, qi, k=0, **opt):
        V.append(Variant(name, kind, like, tuple(qi), int(k), opt))

    n3 = N_DENSE + 3
    if ix.rows == "dense":      # every pass on the dense path
        add("dense_32x100", "search", "dense_5x3000", _q(0, 32), 100, path="dense")
        add("dense_33x1", "search", "dense_5x3000", _q(3, 36), 1, path="dense")
        add("dense_64xN3", "search", "dense_5x3000", _q(0, 64), n3, path="dense")
        add("dense_65x100", "search", "dense_5x3000", _q(60, 125), 100, path="dense")
    else:
        add("classic_65x100", "search", "classic_64x100", _q(0, 65), 100, classic=True, path="filter")
        add("classic_33x1", "search", "classic_64x100", _q(3, 36), 1, classic=True, path="filter")
        add("classic_64x1000", "search", "classic_64x100", _q(60, 124), 1000, classic=True, path="filter")
        # (the one-launch plan takes k <= 100: it has no k = 1000 case)
        add("one_65x100", "search", "one_64x100", _q(0, 65), 100, one_launch=True,
            **({"path": "filter", "one": True} if ix.rows == "one" else {}))
        add("one_33x1", "search", "one_64x100", _q(3, 36), 1, one_launch=True,
            **({"path": "filter", "one": True} if ix.rows == "one" else {}))
        add("exact_dense_64x1000", "search", "dense_40x10", _q(0, 64), 1000, exact_dense=True, path="dense")
        add("exact_dense_32x100", "search", "dense_40x10", _q(0, 32), 100, exact_dense=True, path="dense")
        add("exact_dense_65x1", "search", "dense_40x10", _q(40, 105), 1, exact_dense=True, path="dense")
    add("host_33x100", "search", "host_17x50", _q(10, 43), 100, host=True)
    # filtered: per-query lists across the pass border
    add("mask_tail_64x100", "search", "mask_perq_33x50", _q(0, 64), 100, allowed="tail")
    add("mask_head_65x50", "search", "mask_perq_33x50", _q(0, 65), 50, allowed="head")
    add("mask_mix_33x100", "search", "mask_perq_33x50", _q(10, 43), 100, allowed="mix")
    add("mask_few_64x100", "search", "mask_few_20x100", _q(0, 64), 100, allowed="few")
    # boosted
    add("bias_65x100", "biased", "bias_64x100", _q(0, 65), 100)
    add("bias_mix_64x50", "biased", "bias_mask_33x50", _q(0, 64), 50, allowed="mix")
    # range: a rank per query; query 32 of one batch takes every row (above 16384 rows: its pass is redone densely)
    add("range_65_ranks", "range", "range_33_rank300", _q(0, 65), sort=True)
    add("range_33_all", "range", "range_2_all", _q(20, 53), all_at=32)
    add("range_tail_64", "range", "range_mask_20_rank200", _q(0, 64), allowed="tail")
    add("range_mix_33", "range", "range_mask_20_rank200", _q(0, 33), allowed="mix", sort=True)
    # prefix and funnel
    for dims in (128, 1024, 2048):
        if dims < d:
            add(f"prefix{dims}_33x100", "prefix", "prefix_33x100", _q(0, 33), 100, dims=dims)
    pd = 2048 if d > 2048 else 1024
    add("prefix_mix_65x50", "prefix", "prefix_33x100", _q(0, 65), 50, dims=pd, allowed="mix")
    add("funnel_65x20", "funnel", "funnel_33x20", _q(0, 65), 20, dims=pd, fetch_k=None)
    add("funnel_33x20_f4000", "funnel", "funnel_33x20", _q(7, 40), 20, dims=128, fetch_k=4000, prefix_path="dense")
    add("scores_65", "scores", "scores_40", _q(0, 65))
    add("grouped_33x10", "grouped", "grouped_20x10", _q(0, 33), 10, group_size=2, fetch_k=80)
    add("mmr_33x10", "mmr", "mmr_9x10", _q(0, 33), 10, fetch_k=40, lam=0.5)
    # asynchronous blocks: eight submissions, one finish()
    add("async_plain", "async", "async_plain", (), subs=async_subs(), classic=True, coalesce=False)
    add("async_pipelined", "async", "async_pipelined", (), subs=async_subs(), inputs_ready=True, coalesce=False)
    add("async_one", "async", "async_one", (), subs=async_subs(100), one_launch=True, coalesce=False)
    add("async_mask", "async", "async_mask", (), subs=async_subs(), allowed="tail", coalesce=False)
    add("async_coalesced", "async", "async_co_resident", (), subs=async_subs(), coalesce=True)
    # the tie query in the second pass of submission TIE_SUB: its candidate lists overflow, finish() must report that
    # ticket alone and repair it.  The one-launch scan on the one-launch corpus, the five-launch filter scan elsewhere
    if ix.rows == "one":
        add("async_tie", "async", "async_tie", (), subs=async_subs(100, tie=True), one_launch=True, coalesce=False,
            failed=(TIE_SUB,))
    elif tie0_of(ix) is not None:
        add("async_tie", "async", "async_tie", (), subs=async_subs(100, tie=True), classic=True, coalesce=False,
            failed=(TIE_SUB,))
    return tuple(V)


def supported(ix):
    return tuple(v for v in variants(ix) if v.like in hc.SUPPORTED[ix.storage])


def refused_kinds(storage):
    """The kinds of which handle_reuse_cases.SUPPORTED holds no variant for this storage type."""
    return {v.kind for v in hc.VARIANTS} - {hc.BY_NAME[n].kind for n in hc.SUPPORTED[storage]}


def refused(ix):
    """The variants whose entry point the storage type refuses: each must raise NotImplementedError, as it does today.
    (One-launch and coalescing requests are not refused but ignored, and a masked fp32 pass is a dense one: the table
    leaves those out.)"""
    return tuple(v for v in variants(ix) if v.kind in refused_kinds(ix.storage))


TOMBSTONE = ("dense_65x100", "classic_65x100", "mask_tail_64x100", "bias_65x100", "range_65_ranks", "prefix128_33x100",
             "scores_65")
TABLE_SIZE = {"f16-1100-dense": 28, "f16-2176-dense": 29, "f16-1100-filter": 32, "f16-1100-one": 33,
              "bf16-1100-dense": 28, "bf16-2176-dense": 29, "bf16-2176-filter": 33, "bf16-1100-one": 33,
              "f32-600-dense": 13, "f32-776-dense": 13, "f32-776-filter": 18,
              "fp8-1280-dense": 14, "fp8-2048-dense": 14, "fp8-2048-filter": 19,
              "fp4-1280-dense": 13, "fp4-2048-dense": 13, "fp4-1280-filter": 18}


# ------------------------------------------------------------------------------------------------------------ models
def _topk(S, k, live, allowed):
    D, I = ex.expected_topk(*hc._as_inputs(S), k, live=live, allowed=allowed)
    return D, I


def radius_of(v, dat, live=None):
    """The radius argument of a range variant: float32 [nq]."""
    qi = list(v.qi)
    rad = rm.rank_radius(*hc._as_inputs(dat.S[qi]), ranks_of(len(qi)), live=live,
                         allowed=allowed_of(v.opt.get("allowed"), len(qi), dat.n))
    if "all_at" in v.opt:
        rad = rad.copy()
        rad[v.opt["all_at"]] = -np.inf
    return rad


def expected(v, dat, live=None):
    """The arrays variant ``v`` must return on ``dat`` with the rows ``live`` (bool [n]; None: all), in the order of
    the call's outputs; an asynchronous block: (outputs of every submission in order, positions finish() reports)."""
    n = dat.n
    if v.kind == "async":
        outs = []
        for qi, k in v.opt["subs"]:
            outs += list(_topk(dat.S[list(qi)], k, live, allowed_of(v.opt.get("allowed"), len(qi), n)))
        return tuple(outs), tuple(v.opt.get("failed", ()))
    qi = list(v.qi)
    S = dat.S[qi]
    allowed = allowed_of(v.opt.get("allowed"), len(qi), n)
    if v.kind == "search":
        return _topk(S, v.k, live, allowed)
    if v.kind == "biased":
        return bm.topk_model(S.astype(np.float32), aux("b", n), v.k, live=live, allowed=allowed)
    if v.kind == "range":
        lims, D, I = rm.expected_range(*hc._as_inputs(S), radius_of(v, dat, live), live=live, allowed=allowed)
        if v.opt.get("sort"):
            D, I = rm.sort_segments(lims, D, I)
        return lims, D, I
    if v.kind == "prefix":
        return _topk(dat.Sp(v.opt["dims"])[qi], v.k, live, allowed)
    if v.kind == "funnel":
        fetch = v.opt["fetch_k"] or min(2048, max(8 * v.k, 128))
        _, cand = _topk(dat.Sp(v.opt["dims"])[qi], fetch, live, allowed)
        return fu.rescore_model(S.astype(np.float32), cand, v.k, live=live)
    if v.kind == "scores":
        return (S.astype(np.float32),)
    if v.kind == "grouped":
        D, I = _topk(S, v.opt["fetch_k"], live, allowed)
        gD, gI, gG, ng, nv = gm.group_topk(I, D, aux("groups", n), v.k, v.opt["group_size"])
        assert not ((ng < v.k) & (nv == v.opt["fetch_k"])).any()      # one round: the first fetch is complete
        return gD, gI, gG
    if v.kind == "mmr":
        D, I = _topk(S, v.opt["fetch_k"], live, allowed)
        return hc._mmr(D, I, dat.corpus, v.k, v.opt["lam"])
    raise KeyError(v.kind)


def brute_force_topk(S, k, ok):
    """The model of the models: a float64 sort per query, (score descending, id ascending), -1 / -FLT_MAX padded."""
    B, n = S.shape
    D = np.full((B, k), -FLT_MAX, dtype=np.float32)
    I = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        rows = sorted((r for r in range(n) if ok[b, r]), key=lambda r: (-S[b, r], r))[:k]
        D[b, :len(rows)] = S[b, rows]
        I[b, :len(rows)] = rows
    return D, I


# ------------------------------------------------------------------------------------------------ rescore chunk rule
SCRATCH_CAP = 384 << 20


def rescore_chunk(storage, d, B, C):
    """(qc, qp) of ``ts_index_rescore`` (ts_index.hip): the queries of one launch of the gather, the rescore kernel and
    the select, and of one pass.  16-bit storage: a 32-row tile is kg = dpad / 16 KiB, dpad a multiple of 128."""
    assert storage in ("f16", "bf16")
    kg = -(-d // 128) * 128 // 16
    cbp = -(-C // 32)
    per_q = cbp * kg * 1024 + cbp * 128 + C * 8 + (C * 4 + 15) // 16 * 16
    qp = queries_per_pass(storage, d)
    return max(1, min(min(B, qp), SCRATCH_CAP // per_q)), qp


def chunk_starts(storage, d, B, C):
    """[(pass start q0, column c0 in the pass's image, queries)] of every launch, in order."""
    qc, qp = rescore_chunk(storage, d, B, C)
    return [(q0, c0, min(qc, min(qp, B - q0) - c0)) for q0 in range(0, B, qp) for c0 in range(0, min(qp, B - q0), qc)]


# (storage, d, B, C): in each the scratch cap binds (qc < min(B, qp)) and the last chunk is shorter than qc.
# d = 768 is the 64-query regime: a chunk that crosses column 32 reads both halves of the image in one launch.
RESCORE_CHUNKED = (("f16", 768, 64, 4096), ("bf16", 768, 64, 16384), ("f16", 1100, 33, 8192), ("bf16", 1100, 33, 16384),
                   ("f16", 2176, 32, 4096))
# the (d, B, C) tests/test_funnel_gpu.py rescores, directly (f16 at d = 768, bf16 with an id offset) and through its
# funnel tests (the largest shortlist of each shape): none is chunked
RESCORE_BEFORE = ((768, 5, 1), (768, 5, 31), (768, 5, 32), (768, 65, 33), (768, 33, 1000), (768, 2, 16384),
                  (256, 65, 100),
                  (768, 7, 4000), (768, 65, 128), (768, 33, 800), (384, 33, 5000), (384, 33, 5100), (384, 33, 200),
                  (256, 33, 200))
RESCORE_N = 3001
RESCORE_OFFSET = 1_000_000


def rescore_candidates(B, C, n, live, seed):
    """tests/test_funnel_gpu.py ``_candidates``: padding, ids out of range, a removed row and a duplicate per query."""
    rng = np.random.default_rng([25, seed])
    ids = rng.integers(0, n, size=(B, C)).astype(np.int64)
    dead = np.flatnonzero(~live)
    for b in range(B):
        ids[b, rng.integers(1, C - 1)] = -1
        ids[b, rng.integers(1, C - 1)] = n + 5
        ids[b, rng.integers(1, C - 1)] = -9
        ids[b, rng.integers(1, C - 1)] = dead[b % 7]
        ids[b, C - 1] = ids[b, 0]
    return ids


@functools.lru_cache(maxsize=2)
def rescore_data(d):
    c, q, unit = ex.gen_ints(RESCORE_N, d, 64, seed=26)
    return Data(c, q, unit)


# --------------------------------------------------------------------------------------- running a variant on a handle
class Env:
    """What a run needs on the device, built once per index: the query pool in the type the index takes, the packed
    masks, the bias and the group table."""

    def __init__(self, torch, storage, dat, live=None):
        from tristage_rag_amd.index import pack_allowed
        self.torch, self.storage, self.dat, self.live = torch, storage, dat, live
        qdt = {"f16": torch.float16, "bf16": torch.bfloat16}.get(storage, torch.float32)
        pool = torch.tensor(dat.queries).cuda()
        assert torch.equal(pool.to(qdt).float(), pool)                  # the queries are exact in the query type
        self.pool = pool.to(qdt)
        self._q = {}
        self.masks = {m: torch.from_numpy(pack_allowed(aux(m, dat.n), dat.n).view(np.int32)).cuda() for m in MASKS}
        self.bias = torch.tensor(aux("b", dat.n)).cuda()
        self.groups = torch.tensor(aux("groups", dat.n)).cuda()

    def q(self, qi):
        if qi not in self._q:
            self._q[qi] = self.pool[self.torch.tensor(list(qi), device="cuda")].contiguous()
        return self._q[qi]

    def allowed(self, spec, nq):
        names = allowed_names(spec, nq)
        if names is None or isinstance(names, str):
            return None if names is None else self.masks[names]
        return [None if m is None else self.masks[m] for m in names]


def run(v, idx, env):
    """One call of variant ``v`` on ``idx``: the outputs in the order of ``expected``; an asynchronous block:
    (outputs, positions of the submissions finish() reported)."""
    o = v.opt
    if v.kind == "async":
        idx.coalesce = o.get("coalesce", False)
        outs, tickets = [], []
        for qi, k in o["subs"]:
            before = set(idx._pending)
            outs += list(idx.search(env.q(qi), k, async_=True, classic=o.get("classic", False),
                                    one_launch=o.get("one_launch", False), inputs_ready=o.get("inputs_ready", False),
                                    allowed=env.allowed(o.get("allowed"), len(qi))))
            tickets.append(set(idx._pending) - before)
            assert len(tickets[-1]) == -(-len(qi) // idx.MAX_ASYNC_QUERIES), (v.name, qi[:2], tickets[-1])
        redone = idx.finish()
        assert len(set(redone)) == len(redone) and all(any(t in ts for ts in tickets) for t in redone), (redone, tickets)
        return tuple(outs), tuple(sorted({j for j, ts in enumerate(tickets) for t in redone if t in ts}))
    nq = len(v.qi)
    allowed = env.allowed(o.get("allowed"), nq)
    if v.kind == "search":
        q = env.dat.queries[list(v.qi)] if o.get("host") else env.q(v.qi)
        return idx.search(q, v.k, classic=o.get("classic", False), one_launch=o.get("one_launch", False),
                          exact_dense=o.get("exact_dense", False), allowed=allowed)
    q = env.q(v.qi)
    if v.kind == "biased":
        return idx.search_biased(q, v.k, env.bias, allowed=allowed)
    if v.kind == "range":
        return idx.range_search(q, radius_of(v, env.dat, env.live), allowed=allowed, max_results=o.get("max_results"),
                                sort=o.get("sort", False))
    if v.kind == "prefix":
        return idx.search_prefix(q, v.k, o["dims"], allowed=allowed)
    if v.kind == "funnel":
        return idx.search_funnel(q, v.k, o["dims"], fetch_k=o["fetch_k"], allowed=allowed)
    if v.kind == "scores":
        return (idx.scores(q),)
    if v.kind == "grouped":
        return idx.search_grouped(q, v.k, env.groups, group_size=o["group_size"], fetch_k=o["fetch_k"], allowed=allowed)
    if v.kind == "mmr":
        return idx.search_mmr(q, v.k, fetch_k=o["fetch_k"], lambda_mult=o["lam"], allowed=allowed)
    raise KeyError(v.kind)
