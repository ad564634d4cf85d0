"""float64 model of the best-passage call (include/tristage.h "best passage per candidate"), the
near-tie rule for inputs that are not exactly summable, and the exact inputs of its tests.

Semantics.  Query token rows q_t (t < Lq), document token rows x_j (j < Ld), c[t][j] = cos(q_t, x_j) with the
kernels' clamp (x / max(|x|, 1e-12): a zero row gives 0).  Window w >= 1: we = min(w, Ld), positions p in
[0, Ld - we], S[p] = sum_t max_{p <= j < p + we} c[t][j]; p* = the lowest p with the largest S[p] (a NaN sum ranks
last); start = p*, length = we, score = S[p*] / Lq, align[t] = the lowest j in [p*, p* + we) with the largest c[t][j].
A document without rows: start -1, length 0, score -FLT_MAX, align -1.

Exact inputs (tests/exact_maxsim_inputs.py): every cosine is a multiple of 2^-10 in [-1, 1], so a window sum over
Lq <= 192 tokens is exact in fp32 in any order (|S| <= 192 in steps of 2^-10: 18 bits) and the score is one fp32
division of two exact operands: `exact_score` gives its bits, and a kernel has to EQUAL the model there.
"""
from collections import namedtuple

import numpy as np

import exact_maxsim_inputs as X

FLT_MAX = float(np.finfo(np.float32).max)
TOL_F32, TOL_16 = 2e-6, 1e-5            # the project's MaxSim bound (tests/test_stage1_gpu.py; X.COLBERT_ATOL = 2e-6)
assert X.COLBERT_ATOL == TOL_F32

Passage = namedtuple("Passage", "start length score align window_scores cos")


def tol_of(store):
    return TOL_F32 if store == "f32" else TOL_16


def cosines(q, d):
    """float64 [Lq, Ld] with the kernels' clamp."""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    qn = np.maximum(np.sqrt((q * q).sum(1)), 1e-12)
    dn = np.maximum(np.sqrt((d * d).sum(1)), 1e-12)
    return (q @ d.T) / qn[:, None] / dn[None, :]


def _rank_first(scores):
    """the lowest index of the largest value, a NaN last"""
    s = np.where(np.isnan(scores), -np.inf, scores)
    if np.isnan(scores).all():
        return 0
    return int(np.argmax(s))


def passage(q, d, w):
    """One candidate."""
    q = np.asarray(q, np.float64)
    d = np.asarray(d, np.float64)
    Lq, Ld = q.shape[0], d.shape[0]
    assert Lq >= 1 and w >= 1
    if Ld == 0:
        return Passage(-1, 0, -FLT_MAX, np.full(Lq, -1, np.int32), np.zeros(0), np.zeros((Lq, 0)))
    c = cosines(q, d)
    we = min(int(w), Ld)
    win = np.lib.stride_tricks.sliding_window_view(c, we, axis=1)          # [Lq, Ld - we + 1, we]
    S = win.max(axis=2).sum(axis=0)                                        # [Ld - we + 1]
    p = _rank_first(S)
    align = (p + np.argmax(c[:, p: p + we], axis=1)).astype(np.int32)      # argmax: the lowest j of the largest
    return Passage(p, we, float(S[p] / Lq), align, S, c)


def passages(q, docs, w):
    """A list of candidates of one query."""
    return [passage(q, d, w) for d in docs]


def passages_batch(queries, docs_per_query, w):
    """The batched form: query j against its own list; one flat list in the order of the call's outputs."""
    out = []
    for q, docs in zip(queries, docs_per_query):
        out += passages(q, docs, w)
    return out


def exact_score(S_p, Lq):
    """float32: the bits of S[p] / Lq on exact inputs (S[p] is an fp32 number there)."""
    num = np.float32(S_p)
    assert float(num) == float(S_p)
    return np.float32(num / np.float32(Lq))


def passage_valid(got, model, tol):
    """The near-tie rule.  got = (start, length, score, align or None) of one candidate; True when it is acceptable
    for `model`: the length is the model's; the returned start p has a float64 window score >= best - 2 tol; the
    returned score is within tol of the float64 score at p; every align[t] lies in the window and its float64 cosine
    is >= that token's float64 window maximum - 2 tol."""
    start, length, score, align = got
    start, length = int(start), int(length)
    if length != model.length:
        return False
    if model.length == 0:
        return start == -1 and float(score) == -FLT_MAX and (align is None or (np.asarray(align) == -1).all())
    S = model.window_scores
    if not (0 <= start < S.shape[0]):
        return False
    Lq = model.cos.shape[0]
    if not S[start] >= np.nanmax(S) - 2 * tol:           # (on the sums, not the means: the stricter reading)
        return False
    if not abs(float(score) - S[start] / Lq) <= tol:
        return False
    if align is not None:
        a = np.asarray(align)[:Lq].astype(np.int64)
        if ((a < start) | (a >= start + length)).any():
            return False
        wmax = model.cos[:, start: start + length].max(axis=1)
        if not (model.cos[np.arange(Lq), a] >= wmax - 2 * tol).all():
            return False
    return True


def equal_exact(got, model):
    """On exact inputs: start, length, score bits and alignment EQUAL the model's.  Returns a message or None."""
    start, length, score, align = got
    Lq = model.cos.shape[0]
    if int(start) != model.start or int(length) != model.length:
        return f"span ({int(start)}, {int(length)}) != model ({model.start}, {model.length})"
    want = np.float32(-FLT_MAX) if model.length == 0 else exact_score(model.window_scores[model.start], Lq)
    if np.float32(score).view(np.uint32) != want.view(np.uint32):
        return f"score {float(score)!r} != model {float(want)!r}"
    if align is not None and not np.array_equal(np.asarray(align)[:Lq], model.align):
        return "alignment differs from the model"
    return None


# ------------------------------------------------------------------------------------------------- planted passages
PLANT_H = 64
_TOK_COLS = 4           # columns of one query token's support
_BG_COLS = 16           # columns reserved for the background rows: orthogonal to every query token


def _plant_query(rng, Lq):
    """Lq query tokens with pairwise disjoint supports (so cos(q_s, q_t) = 0 for s != t), exact rows."""
    assert Lq * _TOK_COLS + _BG_COLS <= PLANT_H
    cols = rng.permutation(PLANT_H - _BG_COLS)
    return np.stack([X._row(rng, cols[t * _TOK_COLS: (t + 1) * _TOK_COLS], PLANT_H) for t in range(Lq)])


def _background(rng, Ld):
    """Rows on the reserved columns (cosine 0 with every query token), some of them all-zero."""
    bg = np.stack([X._row(rng, np.arange(PLANT_H - _BG_COLS, PLANT_H), PLANT_H) for _ in range(Ld)])
    bg[rng.random(Ld) < 0.2] = 0.0
    return bg


Planted = namedtuple("Planted", "name q doc w want_start")


def plant(name, Ld, w, clusters, m=4, Lq=12, seed=0):
    """A document of Ld rows whose window score at p is the number of DISTINCT query tokens with a copy inside
    [p, p + w): a cluster of copies of tokens 0 .. m-1 spans exactly [a, a + w) for every a of `clusters` (first copy
    at a, last at a + w - 1), single copies of the other tokens lie at least w rows from every cluster and from one
    another, so no window but a cluster's own holds m of them.  The expected start is the lowest a."""
    rng = np.random.default_rng([seed, Ld, w, len(clusters)])
    assert 2 <= m <= w and m < Lq
    q = _plant_query(rng, Lq)
    doc = _background(rng, Ld)
    taken = np.zeros(Ld, bool)
    for a in clusters:
        assert 0 <= a and a + w <= Ld
        rows = [a, a + w - 1] + sorted(rng.permutation(np.arange(a + 1, a + w - 1))[: m - 2].tolist())
        for t, r in enumerate(sorted(rows)):
            doc[r] = X._scaled_copy(rng, q[t])
        taken[max(0, a - w): a + 2 * w] = True
    t = m
    for r in range(Ld):
        if t < Lq and not taken[r]:
            doc[r] = X._scaled_copy(rng, q[t])
            taken[max(0, r - w): r + w + 1] = True
            t += 1
    return Planted(name, q, doc, w, min(clusters))


def planted_cases():
    return [
        plant("cluster-beats-scattered", 100, 6, [41]),
        plant("duplicate-clusters", 100, 6, [60, 20]),
        plant("cluster-over-rows-31-32", 100, 4, [30]),
        plant("cluster-over-rows-63-64", 100, 4, [62]),
        plant("cluster-ends-at-last-row", 70, 5, [65]),
        plant("cluster-begins-at-row-0", 70, 5, [0]),
        plant("cluster-over-rows-191-192-of-a-long-document", 300, 8, [188]),
    ]


# ----------------------------------------------------------------------------------------------- exact launch table
Launch = namedtuple("Launch", "name H Lq lens windows seed")


def _windows(lens):
    top = max(lens)
    return sorted({1, 2, 31, 32, 33, max(1, top - 1), top, top + 1, 4096})


def exact_launches():
    """The pruned product of the issue's H x Ld x w x Lq: every Ld and every Lq appears with every H class at least
    once, every launch mixes lengths (a zero-length candidate between two real ones) and is run at every w."""
    LD = [1, 2, 31, 32, 33, 63, 64, 65, 192]
    out = []
    for i, (H, Lq) in enumerate(((64, 1), (64, 31), (64, 33), (64, 192), (72, 32), (72, 65), (768, 64), (768, 33))):
        lens = LD[:4] + [0] + LD[4:] if i % 2 == 0 else [33, 0, 192, 1, 64, 31, 2, 65, 32, 63]
        wins = _windows(lens) if H != 768 else [1, 32, 33, 191, 192, 4096]
        out.append(Launch(f"H{H}-Lq{Lq}", H, Lq, tuple(lens), tuple(wins), 100 + i))
    # the long-document kernel: Ld in (192, 1024], rounds of 16 query tokens; a short and an empty one beside them
    out.append(Launch("long-H64-Lq33", 64, 33, (1024, 0, 193, 64, 1000), (1, 32, 33, 1023, 1024, 1025, 4096), 201))
    out.append(Launch("long-H72-Lq17", 72, 17, (256, 1024, 31), (2, 31, 512, 4096), 202))
    return out


def launch_data(L):
    """(q [Lq, H], docs) of a launch: rows of the exact generators (planted copies of query tokens included)."""
    case = X.Case(L.name, "plant", L.H, L.Lq, len(L.lens), ("f16", "bf16", "f32"), L.seed, "default")
    d = X.generate(case, lens=tuple(int(x) for x in L.lens))
    return d.q, d.docs
