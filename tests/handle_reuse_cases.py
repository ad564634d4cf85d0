"""The case table of the handle-reuse tests: every stage-1 entry point as a **variant**, one call on a
``FlatIPIndex`` with fixed arguments, and the function that gives its expected output from exact scores.

A handle owns eight workspace sets handed out round robin, so what one entry point leaves in a set is read by the
ninth acquisition after it.  tests/test_handle_reuse_gpu.py calls a variant eight times in a row (a **block**) and
puts every ordered pair of variants back to back on ONE handle; this file holds what needs no GPU: the inputs, the
variants, their models and the block sequence.  tests/test_handle_reuse_host.py checks all of it.

Inputs are exactly summable (tests/exact_inputs.py): every score is an f32 number whatever the accumulation order, so
the float64 score matrix IS the reference, bit for bit.  It is computed once per corpus, in row chunks, and every
model below is an existing one (exact_inputs.expected_topk, bias_model, range_model, funnel_model, group_model,
mmr_model) fed with rows of that matrix: ``_as_inputs`` hands a model the pair (S^T, identity), whose product is S.

No torch import at module level; ``Env`` (the device copies a run needs) imports it when a GPU test builds one."""
import functools
from typing import NamedTuple

import numpy as np

import bias_model as bm
import exact_inputs as ex
import funnel_model as fu
import group_model as gm
import mmr_model as mm
import range_model as rm

N = 2 * 32768 + 37            # >= ex.one_launch_rows() on 256 CUs and >= 32 * 2048 (k = 2048 stays on the filter path);
                              # the last row block holds 5 rows
TIE0, TIE_N = 30_011, 20_000  # rows [TIE0, TIE0 + TIE_N) are copies of one row: more than the 16384 candidate slots
NQ = 64                       # ordinary queries; query NQ of the pool is the tie query (the copied row itself)
TIE_Q = NQ
CAND_CAP = rm.CAND_CAP
PREFIX_DIMS = 256
BLOCK = 8                     # calls per block: the handle's workspace sets (ts_index.hip TS_NSETS)
STORAGE_D = {"f16": 768, "bf16": 768, "f32": 96, "fp8": 256, "fp4": 256}
FP8_SCALE_LOG2 = 0            # e4m3 holds the integers |v| <= 15 exactly at scale 1
FP4_GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)   # e2m1 at scale 1
FLT_MAX = ex.FLT_MAX


# ------------------------------------------------------------------------------------------------------------ inputs
class Data(NamedTuple):
    corpus: np.ndarray     # float32 [N, d], what reconstruct_n() must return
    queries: np.ndarray    # float32 [NQ + 1, d]; row TIE_Q is the tie query
    unit: float
    S: np.ndarray          # float64 [NQ + 1, N]: the exact scores
    Sp: np.ndarray         # float64 [NQ + 1, N] over the first PREFIX_DIMS dimensions (None where d is not larger)


def _kind(storage):
    return {"f16": "ints768", "bf16": "ints768", "f32": "ints96", "fp8": "fp8", "fp4": "fp4"}[storage]


def _rows(kind):
    d = {"ints768": 768, "ints96": 96, "fp8": 256, "fp4": 256}[kind]
    c, q, unit = ex.gen_ints(N, d, NQ, seed=24)
    if kind == "fp8":
        c = np.random.default_rng([24, 8]).integers(-15, 16, size=(N, d)).astype(np.float32)
    if kind == "fp4":
        rng = np.random.default_rng([24, 4])
        c = FP4_GRID[rng.integers(0, 8, size=(N, d))] * (rng.integers(0, 2, size=(N, d)) * 2 - 1).astype(np.float32)
        # one +-6 in each scale block (dimensions 64 g + 16 m + 8 h + j): the block's scale is 1 and every value exact
        for k0 in (0, 8):
            c[:, k0::64] = np.float32(6.0) * (rng.integers(0, 2, size=c[:, k0::64].shape) * 2 - 1)
        unit = 0.25       # the tie query is a corpus row: multiples of 0.5 on both sides
    return np.ascontiguousarray(c, dtype=np.float32), q, unit


def chunked_scores(corpus, queries, dims=None, step=8192):
    """float64 [B, n] of ``queries @ corpus.T`` over the first ``dims`` dimensions, in row chunks (no float64 corpus)."""
    q = np.asarray(queries, np.float64)[:, :dims]
    out = np.empty((q.shape[0], corpus.shape[0]), dtype=np.float64)
    for r0 in range(0, corpus.shape[0], step):
        out[:, r0:r0 + step] = q @ corpus[r0:r0 + step, :dims].astype(np.float64).T
    return out


@functools.lru_cache(maxsize=None)
def _data(kind):
    c, q, unit = _rows(kind)
    tie = c[TIE0].copy()
    if kind == "ints768":
        tie[:PREFIX_DIMS] = 0.0       # the prefix passes score the copied row 0: below their thresholds too
    c[TIE0:TIE0 + TIE_N] = tie
    # every ordinary query scores the copied row below zero (a query's negative is as good a query)
    dot = q.astype(np.float64) @ tie.astype(np.float64)
    q = np.where(dot[:, None] > 0, -q, q).astype(np.float32)
    Q = np.concatenate([q, tie[None, :]])
    d = c.shape[1]
    S = chunked_scores(c, Q)
    Sp = chunked_scores(c, Q, PREFIX_DIMS) if d > PREFIX_DIMS and kind == "ints768" else None
    for a in (c, Q, S) + (() if Sp is None else (Sp,)):
        a.setflags(write=False)
    return Data(c, Q, unit, S, Sp)


def data(storage):
    return _data(_kind(storage))


@functools.lru_cache(maxsize=None)
def aux(name):
    """The masks, biases, group table and candidate ids the variants name (the same for every storage type)."""
    rng = np.random.default_rng([24, sum(map(ord, name))])
    if name == "m30":
        out = rng.random(N) < 0.3
    elif name == "m05":
        out = rng.random(N) < 0.05
    elif name == "mod97":
        out = np.arange(N) % 97 == 0
    elif name == "few":                                   # 37 rows: fewer than any k it is used with
        out = np.zeros(N, dtype=bool)
        out[rng.choice(N, size=37, replace=False)] = True
    elif name == "b":                                     # integer-valued: the f32 sum score + bias is exact
        out = rng.integers(-2000, 2001, size=N).astype(np.float32)
    elif name == "btie":                                  # ... constant over the copied rows: their ties stay ties
        out = rng.integers(-2000, 2001, size=N).astype(np.float32)
        out[TIE0:TIE0 + TIE_N] = 5.0
    elif name == "groups":
        out = (np.arange(N) // 5).astype(np.int32)
    elif name == "ids":                                   # rescore candidates: padding, repeats, ids out of range
        out = rng.integers(0, N, size=(16, 300)).astype(np.int64)
        out[rng.random(out.shape) < 0.05] = -1
        out[:, 7] = out[:, 3]
        out[2, 11], out[5, 0] = N + 3, -7
    elif name == "live":                                  # the tombstone phase removes every third row
        out = np.arange(N) % 3 != 0
    else:
        raise KeyError(name)
    out.setflags(write=False)
    return out


def allowed_of(spec, nq):
    """The ``allowed`` argument a variant names, as the models take it: None, one mask, or a per-query list."""
    if spec is None:
        return None
    if spec == "perq":
        return [None if j % 4 == 3 else aux(("m30", "m05", "mod97")[j % 3]) for j in range(nq)]
    return aux(spec)


# ---------------------------------------------------------------------------------------------------------- variants
class Variant(NamedTuple):
    name: str
    kind: str        # search | biased | range | prefix | rescore | funnel | scores | grouped | mmr | async
    qi: tuple        # rows of the query pool
    k: int
    opt: dict


def _q(a, b):
    return tuple(range(a, b))


TIE8 = (8, 9, 10, TIE_Q, 12, 13, 14, 15)   # a batch of eight holding the tie query

# the eight submissions of an asynchronous block: (queries, k), large then small then large
ASYNC_SUBS = ((_q(0, 64), 100), (_q(0, 33), 10), (_q(5, 6), 1), (_q(0, 64), 500), (_q(20, 37), 100), (_q(0, 64), 7),
              (_q(32, 64), 257), (_q(40, 45), 100))
ASYNC_SUBS_ONE = tuple((qi, min(k, 100)) for qi, k in ASYNC_SUBS)          # the one-launch plan: k <= 100
ASYNC_SUBS_TIE = ASYNC_SUBS_ONE[:4] + ((TIE8, 100),) + ASYNC_SUBS_ONE[5:]  # submission 4 overflows: finish() redoes it


def _build():
    V = []

    def add(name, kind, qi, k=0, **opt):
        V.append(Variant(name, kind, tuple(qi), int(k), opt))

    # a. five-launch search
    add("classic_64x100", "search", _q(0, 64), 100, classic=True)
    add("classic_1x1", "search", _q(5, 6), 1, classic=True)
    add("classic_33x2048", "search", _q(0, 33), 2048, classic=True)
    add("classic_tie_8x500", "search", TIE8, 500, classic=True)
    # b. one-launch search, forced
    add("one_64x100", "search", _q(0, 64), 100, one_launch=True)
    add("one_33x7", "search", _q(20, 53), 7, one_launch=True)
    add("one_tie_8x100", "search", TIE8, 100, one_launch=True)
    # c. dense path
    add("dense_40x10", "search", _q(0, 40), 10, exact_dense=True)
    add("dense_5x3000", "search", _q(40, 45), 3000)
    # d. host queries and outputs (the handle's staging buffers)
    add("host_17x50", "search", _q(3, 20), 50, host=True)
    # e. filtered
    add("mask_one_64x100", "search", _q(0, 64), 100, allowed="m30")
    add("mask_perq_33x50", "search", _q(10, 43), 50, allowed="perq")
    add("mask_few_20x100", "search", _q(0, 20), 100, allowed="few")
    # f. boosted
    add("bias_64x100", "biased", _q(0, 64), 100, bias="b")
    add("bias_mask_33x50", "biased", _q(5, 38), 50, bias="b", allowed="m30")
    add("bias_tie_8x100", "biased", TIE8, 100, bias="btie")
    # g. range
    add("range_33_rank300", "range", _q(0, 33), rank=300, sort=True)
    add("range_2_all", "range", _q(1, 3), radius=-np.inf, max_results=2 * N)
    add("range_mask_20_rank200", "range", _q(30, 50), rank=200, allowed="m30")
    add("range_limit_16", "range", _q(0, 16), rank=300, max_results=1000, raises=True)
    # h. funnel
    add("prefix_33x100", "prefix", _q(0, 33), 100)
    add("rescore_16x300", "rescore", _q(0, 16), 50)
    add("funnel_33x20", "funnel", _q(7, 40), 20, fetch_k=160)
    # i. scores
    add("scores_40", "scores", _q(0, 40))
    # j. on top of a search
    add("grouped_20x10", "grouped", _q(0, 20), 10, group_size=2, fetch_k=80)
    add("mmr_9x10", "mmr", _q(0, 9), 10, fetch_k=40, lam=0.5)
    # k. asynchronous: eight submissions and one finish()
    add("async_plain", "async", (), subs=ASYNC_SUBS, classic=True, coalesce=False)
    add("async_pipelined", "async", (), subs=ASYNC_SUBS, inputs_ready=True, coalesce=False)
    add("async_one", "async", (), subs=ASYNC_SUBS_ONE, one_launch=True, coalesce=False)
    add("async_co_resident", "async", (), subs=ASYNC_SUBS, classic=True, coalesce=True, wide=False, stat=False)
    add("async_co_wide", "async", (), subs=ASYNC_SUBS, classic=True, coalesce=True, wide=True, stat=False)
    add("async_co_stat", "async", (), subs=ASYNC_SUBS, classic=True, coalesce=True, stat=True, prologue=False)
    add("async_co_stat_prologue", "async", (), subs=ASYNC_SUBS, classic=True, coalesce=True, stat=True, prologue=True)
    add("async_mask", "async", (), subs=ASYNC_SUBS, allowed="m30", coalesce=False)
    add("async_tie", "async", (), subs=ASYNC_SUBS_TIE, one_launch=True, coalesce=False, failed=(4,))
    return tuple(V)


VARIANTS = _build()
BY_NAME = {v.name: v for v in VARIANTS}

_SEARCHES = ("classic_64x100", "classic_1x1", "classic_33x2048", "classic_tie_8x500", "one_64x100", "one_33x7",
             "one_tie_8x100", "dense_40x10", "dense_5x3000", "host_17x50")
_MASKED = ("mask_one_64x100", "mask_perq_33x50", "mask_few_20x100")
# What each storage type takes, after the library's refusals: range search has no fp8 / fp4 form, the prefix, rescore,
# funnel and boosted passes are f16 / bf16 only, so are the coalesced passes' kernels (an fp32, fp8 or fp4 index never
# joins the queue), MMR has no fp4 form; fp8 and fp4 ignore the one-launch request (kept once: "one-launch requested")
# and a masked fp32 pass is a dense one (left out: "the unfiltered, dense and scores variants").
SUPPORTED = {
    "f16": tuple(v.name for v in VARIANTS),
    "bf16": tuple(v.name for v in VARIANTS),
    "f32": _SEARCHES + ("range_33_rank300", "range_2_all", "range_limit_16", "scores_40", "grouped_20x10", "mmr_9x10",
                        "async_plain", "async_pipelined", "async_one", "async_tie"),
    "fp8": _SEARCHES[:5] + _SEARCHES[7:] + _MASKED + ("scores_40", "grouped_20x10", "mmr_9x10", "async_plain",
                                                      "async_mask", "async_tie"),
    "fp4": _SEARCHES[:5] + _SEARCHES[7:] + _MASKED + ("scores_40", "grouped_20x10", "async_plain", "async_mask",
                                                      "async_tie"),
}
TABLE_SIZE = {"f16": 35, "bf16": 35, "f32": 20, "fp8": 17, "fp4": 16}
assert {s: len(v) for s, v in SUPPORTED.items()} == TABLE_SIZE and all(len(set(v)) == len(v) for v in SUPPORTED.values())

# after every third row is removed (every search is a filtered one through the live bitmap; 13 334 copies are left,
# so nothing overflows any more)
TOMBSTONE = ("classic_64x100", "one_64x100", "mask_one_64x100", "bias_64x100", "range_33_rank300", "prefix_33x100",
             "scores_40", "async_plain", "async_co_resident")
# one thread each, on its own stream, 10 repetitions (no asynchronous submitter: FlatIPIndex.range_search finishes
# pending searches first, which only their submitting thread may do)
CONCURRENT = ("classic_64x100", "one_64x100", "mask_one_64x100", "bias_64x100", "range_33_rank300", "prefix_33x100",
              "rescore_16x300", "scores_40", "host_17x50")


def variants_of(storage, names=None):
    return [BY_NAME[n] for n in (SUPPORTED[storage] if names is None else names) if n in SUPPORTED[storage]]


# ---------------------------------------------------------------------------------------------------- block sequence
def sequence(names, a):
    """The blocks of variant ``a``'s test: a, b1, a, b2, ..., a, bn over every other name, in table order."""
    out = []
    for b in names:
        if b != a:
            out += [a, b]
    return out


def pairs_of(seq):
    return set(zip(seq[:-1], seq[1:]))


def split_sequence(names, a, parts=1):
    """``sequence`` cut into ``parts`` tests, each starting with an ``a`` block: no pair (a, b) is lost, and the pairs
    (b, a) a cut drops are in b's own tests."""
    others = [b for b in names if b != a]
    step = -(-len(others) // parts)
    return [sequence([a] + others[i:i + step], a) for i in range(0, len(others), step)]


# ------------------------------------------------------------------------------------------------------------ models
def _as_inputs(S):
    """(corpus, queries) whose exact score matrix is S: for the models that take inputs, not scores."""
    return S.T, np.eye(S.shape[0])


def _topk(S, k, live=None, allowed=None):
    return ex.expected_topk(*_as_inputs(S), k, live=live, allowed=allowed)


_TOPK = {}


def _topk_of(dat, which, qi, k, live, spec):
    """``_topk`` of rows ``qi`` of ``dat.S`` / ``dat.Sp`` under the named mask, kept: many variants share a list."""
    key = (id(dat.S), which, tuple(qi), k, live is None, spec)
    if key not in _TOPK:
        D, I = _topk(getattr(dat, which)[list(qi)], k, live, allowed_of(spec, len(qi)))
        D.setflags(write=False)
        I.setflags(write=False)
        _TOPK[key] = (D, I)
    return _TOPK[key]


def _radius(v, S, live, allowed):
    if "radius" in v.opt:
        return np.float32(v.opt["radius"])
    return rm.rank_radius(*_as_inputs(S), v.opt["rank"], live=live, allowed=allowed)


def _mmr(D, I, corpus, k, lam):
    rows = np.where(I[..., None] >= 0, corpus[np.clip(I, 0, None)], np.float32(0.0)).astype(np.float64)
    gram = rows @ rows.transpose(0, 2, 1)
    assert np.abs(gram).max() < 2 ** 22 and np.abs(D[I >= 0]).max() < 2 ** 22     # f32 holds every objective exactly
    picks = mm.mmr_select_batch(D, gram, k, lam, I >= 0)
    outD = np.full((I.shape[0], k), -mm.FLT_MAX, dtype=np.float32)
    outI = np.full((I.shape[0], k), -1, dtype=np.int64)
    ok = picks >= 0
    r, _ = np.nonzero(ok)
    outD[ok], outI[ok] = D[r, picks[ok]], I[r, picks[ok]]
    return outD, outI


def expected(v, dat, live=None):
    """The arrays variant ``v`` must return on data ``dat`` with the rows ``live`` (bool [N], None: all).  A tuple of
    numpy arrays in the order of the call's outputs; an asynchronous block: (outputs of every submission in order,
    positions of the submissions finish() must report).  ``range_limit``: the per-query counts the error carries."""
    if v.kind == "async":
        outs = []
        for qi, k in v.opt["subs"]:
            outs += list(_topk_of(dat, "S", qi, k, live, v.opt.get("allowed")))
        return tuple(outs), tuple(v.opt.get("failed", ()))
    qi = list(v.qi)
    S = dat.S[qi]
    allowed = allowed_of(v.opt.get("allowed"), len(qi))
    spec = v.opt.get("allowed")
    if v.kind == "search":
        return _topk_of(dat, "S", v.qi, v.k, live, spec)
    if v.kind == "biased":
        return bm.topk_model(S.astype(np.float32), aux(v.opt["bias"]), v.k, live=live, allowed=allowed)
    if v.kind == "range":
        rad = _radius(v, S, live, allowed)
        lims, D, I = rm.expected_range(*_as_inputs(S), rad, live=live, allowed=allowed)
        if v.opt.get("raises"):
            return (np.diff(lims),)
        if v.opt.get("sort"):
            D, I = rm.sort_segments(lims, D, I)
        return lims, D, I
    if v.kind == "prefix":
        return _topk_of(dat, "Sp", v.qi, v.k, live, spec)
    if v.kind == "rescore":
        return fu.rescore_model(S.astype(np.float32), aux("ids"), v.k, live=live)
    if v.kind == "funnel":
        _, cand = _topk_of(dat, "Sp", v.qi, v.opt["fetch_k"], live, spec)
        return fu.rescore_model(S.astype(np.float32), cand, v.k, live=live)
    if v.kind == "scores":
        return (S.astype(np.float32),)
    if v.kind == "grouped":
        D, I = _topk_of(dat, "S", v.qi, v.opt["fetch_k"], live, spec)
        gD, gI, gG, ng, nv = gm.group_topk(I, D, aux("groups"), v.k, v.opt["group_size"])
        assert not ((ng < v.k) & (nv == v.opt["fetch_k"])).any()      # one round: the first fetch is complete
        return gD, gI, gG
    if v.kind == "mmr":
        D, I = _topk_of(dat, "S", v.qi, v.opt["fetch_k"], live, spec)
        return _mmr(D, I, dat.corpus, v.k, v.opt["lam"])
    raise KeyError(v.kind)


def range_radius(v, dat, live=None):
    """The radius argument of a range variant (float32 scalar or [nq])."""
    qi = list(v.qi)
    return _radius(v, dat.S[qi], live, allowed_of(v.opt.get("allowed"), len(qi)))


# --------------------------------------------------------------------------------------- running a variant on a handle
class Env:
    """What a run needs on the device, built once per storage type: the query pool in the type the index takes, the
    packed masks, biases, group table and candidate ids."""

    def __init__(self, torch, storage, dat, live=None):
        from tristage_rag_amd.index import pack_allowed
        self.torch, self.storage, self.dat, self.live = torch, storage, dat, live
        qdt = {"f16": torch.float16, "bf16": torch.bfloat16}.get(storage, torch.float32)
        pool = torch.tensor(dat.queries).cuda()                            # (a copy: the shared arrays are read-only)
        assert torch.equal(pool.to(qdt).float(), pool)                  # the queries are exact in the query type
        self.pool = pool.to(qdt)
        self.pool_host = dat.queries
        self._q = {}
        self.masks = {m: torch.from_numpy(pack_allowed(aux(m), N).view(np.int32)).cuda() for m in ("m30", "m05", "mod97", "few")}
        self.bias = {b: torch.tensor(aux(b)).cuda() for b in ("b", "btie")}
        self.groups = torch.tensor(aux("groups")).cuda()
        self.ids = torch.tensor(aux("ids")).cuda()
        self._radius = {}

    def q(self, qi):
        if qi not in self._q:
            self._q[qi] = self.pool[self.torch.tensor(list(qi), device="cuda")].contiguous()
        return self._q[qi]

    def allowed(self, spec, nq):
        if spec is None:
            return None
        if spec == "perq":
            return [None if j % 4 == 3 else self.masks[("m30", "m05", "mod97")[j % 3]] for j in range(nq)]
        return self.masks[spec]

    def radius(self, v):
        if v.name not in self._radius:
            self._radius[v.name] = range_radius(v, self.dat, self.live)
        return self._radius[v.name]


def run(v, idx, env):
    """One call of variant ``v`` on ``idx``: the outputs as a tuple in the order of ``expected``; an asynchronous block:
    (outputs, positions finish() reported).  ``range_limit``: the counts of the error the call must raise."""
    o = v.opt
    if v.kind == "async":
        idx.coalesce = o.get("coalesce", False)
        idx.wide_passes = o.get("wide", "auto")
        idx.stationary_passes = o.get("stat", "auto")
        idx.pass_prologue = o.get("prologue", "auto")
        outs, tickets = [], []
        for qi, k in o["subs"]:
            outs += list(idx.search(env.q(qi), k, async_=True, classic=o.get("classic", False),
                                    one_launch=o.get("one_launch", False), inputs_ready=o.get("inputs_ready", False),
                                    allowed=env.allowed(o.get("allowed"), len(qi))))
            tickets.append(int(idx._lib.ts_index_last_ticket(idx._h)))
        redone = idx.finish()
        assert all(t in tickets for t in redone), (redone, tickets)
        return tuple(outs), tuple(sorted(tickets.index(t) for t in redone))
    nq = len(v.qi)
    allowed = env.allowed(o.get("allowed"), nq)
    if v.kind == "search":
        q = env.pool_host[list(v.qi)] if o.get("host") else env.q(v.qi)
        return idx.search(q, v.k, classic=o.get("classic", False), one_launch=o.get("one_launch", False),
                          exact_dense=o.get("exact_dense", False), allowed=allowed)
    q = env.q(v.qi)
    if v.kind == "biased":
        return idx.search_biased(q, v.k, env.bias[o["bias"]], allowed=allowed)
    if v.kind == "range":
        from tristage_rag_amd.index import RangeSearchLimitError
        try:
            out = idx.range_search(q, env.radius(v), allowed=allowed, max_results=o.get("max_results"),
                                   sort=o.get("sort", False))
        except RangeSearchLimitError as e:
            assert o.get("raises"), f"{v.name}: {e}"
            return (np.asarray(e.counts),)
        assert not o.get("raises"), f"{v.name}: the call must raise RangeSearchLimitError"
        return out
    if v.kind == "prefix":
        return idx.search_prefix(q, v.k, PREFIX_DIMS, allowed=allowed)
    if v.kind == "rescore":
        return idx.rescore(q, env.ids, v.k)
    if v.kind == "funnel":
        return idx.search_funnel(q, v.k, PREFIX_DIMS, fetch_k=o["fetch_k"], allowed=allowed)
    if v.kind == "scores":
        return (idx.scores(q),)
    if v.kind == "grouped":
        return idx.search_grouped(q, v.k, env.groups, group_size=o["group_size"], fetch_k=o["fetch_k"], allowed=allowed)
    if v.kind == "mmr":
        return idx.search_mmr(q, v.k, fetch_k=o["fetch_k"], lambda_mult=o["lam"], allowed=allowed)
    raise KeyError(v.kind)


_INFO_KEYS = ("path", "one_launch", "max_candidates", "sample_rows")


def path_info(v, idx):
    """What the path check compares after a call of ``v``: the counters of the entry points it went through.  Rescore
    and scores set none; the funnel's and the grouped and diversified searches' are those of their search."""
    if v.kind in ("rescore", "scores"):
        return {}
    if v.kind == "range":
        if v.opt.get("raises"):
            return {}
        return {"range": idx.last_range_info(), "path": idx.last_search_info()["path"]}
    info = idx.last_search_info()
    out = {"search": {key: info[key] for key in _INFO_KEYS}}
    if v.kind == "biased":
        out["bias"] = idx.last_bias_info()
    if v.opt.get("allowed") is not None and v.kind != "biased":
        out["filter"] = idx.last_filter_info()
    if v.kind == "funnel":
        out["funnel"] = idx.last_funnel_info()
    if v.kind == "grouped":
        g = idx.last_group_info()
        out["group"] = {"fetched": g["fetched"], "rounds": g["rounds"]}
    return out
