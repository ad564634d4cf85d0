"""Host model of maximal marginal relevance, in float64.

One query: ``rel`` [C] relevances, ``S`` [C, C] similarities, ``valid`` [C] (False = padding or a removed row).
Step 0 picks the largest relevance; step t the unpicked valid candidate with the largest
``lam * rel[i] - (1 - lam) * max_{j picked} S[i, j]``; ties go to the lower position.  No GPU is needed here.
"""
import itertools

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def _objective(rel, S, picked, lam):
    """float64 objective of every candidate given the picks so far (step 0: the relevance)."""
    rel = np.asarray(rel, dtype=np.float64)
    if not picked:
        return rel.copy()
    S = np.asarray(S, dtype=np.float64)
    return lam * rel - (1.0 - lam) * S[:, picked].max(axis=1)


def mmr_select(rel, S, k, lam, valid=None):
    """Positions of the picks in selection order (at most ``k``; fewer when fewer candidates are valid)."""
    rel = np.asarray(rel, dtype=np.float64)
    C = rel.shape[0]
    free = np.ones(C, dtype=bool) if valid is None else np.asarray(valid, dtype=bool).copy()
    picks = []
    for _ in range(min(int(k), C)):
        if not free.any():
            break
        obj = np.where(free, _objective(rel, S, picks, lam), -np.inf)
        best = obj.max()
        p = int(np.nonzero(free & (obj == best))[0][0])      # ties: the lower position
        picks.append(p)
        free[p] = False
    return picks


def mmr_select_batch(rel, S, k, lam, valid=None):
    """``mmr_select`` for B queries at once (rel [B, C], S [B, C, C] of any float dtype, valid [B, C]): the same
    float64 arithmetic with the running maximum kept per candidate, one vectorised step for all queries.  Returns
    picks int64 [B, k], -1 where a query has run out of valid candidates.  The picks of a smaller k are a prefix."""
    rel = np.asarray(rel, dtype=np.float64)
    B, C = rel.shape
    free = np.ones((B, C), dtype=bool) if valid is None else np.asarray(valid, dtype=bool).copy()
    maxsim = np.full((B, C), -np.inf)
    picks = np.full((B, int(k)), -1, dtype=np.int64)
    rows = np.arange(B)
    for t in range(min(int(k), C)):
        with np.errstate(invalid="ignore"):   # (0 * -inf of a query that never had a valid candidate: masked below)
            obj = rel if t == 0 else lam * rel - (1.0 - lam) * maxsim
        obj = np.where(free, obj, -np.inf)
        best = obj.max(axis=1, keepdims=True)
        p = np.argmax(free & (obj == best), axis=1)            # the first position holding the maximum
        live = free[rows, p]
        if not live.any():
            break
        picks[live, t] = p[live]
        free[rows[live], p[live]] = False
        maxsim[live] = np.maximum(maxsim[live], np.asarray(S[rows[live], p[live], :], dtype=np.float64))
    return picks


def mmr_output(ids, rel, picks, k):
    """``(D float32 [k], I int64 [k])`` a query's picks give: the relevances and ids in selection order, -FLT_MAX / -1
    behind them."""
    D = np.full(int(k), -FLT_MAX, dtype=np.float32)
    I = np.full(int(k), -1, dtype=np.int64)
    D[: len(picks)] = np.asarray(rel, dtype=np.float32)[picks]
    I[: len(picks)] = np.asarray(ids, dtype=np.int64)[picks]
    return D, I


def step_valid(rel, S, picks, lam, tol, valid=None):
    """Every step of ``picks`` is a best choice up to ``tol``: the float64 objective of pick t given picks[:t] is at
    least the best objective among the valid candidates not picked before, minus ``tol``.  Checks every step (it does
    not stop at the first difference from the model); also that the picks are distinct, valid positions.  Returns the
    largest shortfall seen (<= tol)."""
    rel = np.asarray(rel, dtype=np.float64)
    C = rel.shape[0]
    free = np.ones(C, dtype=bool) if valid is None else np.asarray(valid, dtype=bool).copy()
    worst = 0.0
    for t, p in enumerate(picks):
        p = int(p)
        assert 0 <= p < C and free[p], f"step {t}: position {p} is not a free valid candidate"
        obj = _objective(rel, S, [int(x) for x in picks[:t]], lam)
        best = obj[free].max()
        short = float(best - obj[p])
        assert short <= tol, f"step {t}: objective {obj[p]!r} of pick {p} is {short:.3e} below the best {best!r}"
        worst = max(worst, short)
        free[p] = False
    return worst


def mmr_brute_force_step(rel, S, picked, lam, valid=None):
    """The definition, spelled out for tiny C: the best unpicked valid position by (objective desc, position asc)."""
    C = len(rel)
    best = None
    for i in range(C):
        if i in picked or (valid is not None and not valid[i]):
            continue
        if picked:
            o = lam * float(rel[i]) - (1.0 - lam) * max(float(S[i][j]) for j in picked)
        else:
            o = float(rel[i])
        if best is None or o > best[0]:
            best = (o, i)
    return None if best is None else best[1]


def mmr_brute_force(rel, S, k, lam, valid=None):
    picks = []
    for _ in range(k):
        p = mmr_brute_force_step(rel, S, picks, lam, valid)
        if p is None:
            break
        picks.append(p)
    return picks


def all_small_cases(max_c=6, seed=0):
    """(rel, S, valid) for every C <= max_c: small integers, so ties are frequent and every objective is exact."""
    rng = np.random.default_rng(seed)
    for C, rep in itertools.product(range(1, max_c + 1), range(40)):
        X = rng.integers(-2, 3, size=(C, 3)).astype(np.float64)
        S = X @ X.T
        rel = rng.integers(-3, 4, size=C).astype(np.float64)
        valid = rng.random(C) < 0.8 if rep % 2 else None
        yield rel, S, valid
