"""Exactly scored inputs for stage-2 MaxSim ("exact inputs for MaxSim").

Every token row, query or document, has entries in {0, +-1, +-2, +-4} and a sum of squares 4^j, j <= 5 (or is all-zero).
Then every product, partial dot product and partial sum of squares is a small integer, sqrt(4^j) = 2^j and its
reciprocal are exact, every cosine is a multiple of 2^-10 in [-1, 1], and the sum of Lq <= 192 maxima is exact in fp32
in any order: the only rounding of the ``maxsim`` score is the final division by Lq, one IEEE fp32 division of two
exact operands.  A correct kernel returns ``expected_maxsim`` bit for bit, in every store type (the values are exact in
f16, bf16, f32 and e4m3), and the tests compare with ``np.array_equal``.  ``colbert`` goes through expf and is
compared with float64 at COLBERT_ATOL.

Classes:
  plant  random rows, plus PLANTED rows in every candidate: copies (times 1, 2 or 4) of query tokens whose supports
         are disjoint, at row 0, row len-1, rows 31 and 32 and the last row of every full 32-row tile, each for a
         different query token.  Its cosine is exactly 1 and no other row reaches 1 for that token: a kernel that
         loses the row returns a different score.  One query token is all-zero (its maximum is exactly 0) and one
         has only negative entries where the documents have none below zero (its maximum is <= 0).
  kedge  as plant, the planted tokens hot only in the last 8 columns: the half k step of rows with
         row_bytes % 32 == 16 and the last real k step before the padded ones.
  neg    document entries >= 0, query entries <= 0, one column hot in every row: every cosine is < 0, except in
         the candidates that hold one all-zero row (their maxima are exactly 0).
  ones   every candidate holds a copy of every query token: all maxima are 1 (the stale-scratch test's first launch).

The mirrors of the dispatch (``m16_shape``) and of the slicing (``slice_facts``) only decide which case covers which
path; no expected value comes from them.  No GPU is needed here; tests/test_exact_maxsim_host.py checks all of it and
tests/test_exact_maxsim_gpu.py walks the same table.
"""
import functools
from collections import namedtuple

import numpy as np

COLBERT_ATOL = 2e-6                      # the project's fp32 bound (tests/test_stage1_gpu.py), for every store type here
STORES = ("f16", "bf16", "f32", "e4m3_f16", "e4m3_bf16")
SCALE_BITS = 10                          # cosines are multiples of 2^-10
M16_MAX_DOCS, M16_MAX_BATCH, M16_WAVES = 4096, 64, 4


def store_dtype(store):
    return "e4m3" if store.startswith("e4m3") else store


def elem_bytes(store):
    return {"f32": 4, "e4m3": 1}.get(store_dtype(store), 2)


# ------------------------------------------------------------------------------------------- mirror of the dispatch
Shape = namedtuple("Shape", "row_bytes ring s_pad nqt passes lq_pad full")


def m16_shape(H, store, max_lq):
    """ts_maxsim16.hip m16_shape: the launch shape, or None where the streaming kernel does not take the rows."""
    dt = store_dtype(store)
    ups = 2 if dt == "e4m3" else 1
    row_bytes = H * elem_bytes(store)
    if row_bytes % 16:
        return None
    s_real = (row_bytes + 31) // 32
    ring = 24 if (dt == "e4m3" and row_bytes % (32 * 24) == 0 and row_bytes % (32 * 16) != 0) else 16
    s_pad = (s_real + ring - 1) // ring * ring
    cap = 156 * 1024
    extra = M16_WAVES * 32 * 4 + 64 + (M16_MAX_DOCS + 1) * 4 + 12
    image = s_pad * ups * 1024
    nqt = 2 if (max_lq > 32 and image * 2 + extra <= cap) else 1
    if image * nqt + extra > cap:
        return None
    passes = (max_lq + nqt * 32 - 1) // (nqt * 32)
    return Shape(row_bytes, ring, s_pad, nqt, passes, passes * nqt * 32, row_bytes % (32 * ring) == 0)


def kernel_path(H, store, max_lq, form):
    """What runs: ("m16", store, nqt, full, ring, form), ("fallback", element type, "vec" | "scalar"), or None for an
    e4m3 store the streaming kernel refuses (there is no general kernel behind it)."""
    sh = m16_shape(H, store, max_lq)
    if sh is not None:
        return ("m16", store, sh.nqt, sh.full, sh.ring, form)
    if store_dtype(store) == "e4m3":
        return None
    return ("fallback", store, "vec" if H % 8 == 0 else "scalar")      # ts_maxsim.hip: one launch per query


# -------------------------------------------------------------------------------------------- mirror of the slicing
def tiles_of(lens):
    lens = np.asarray(lens, np.int64)
    return np.where(lens > 0, (lens + 31) // 32, 0)


def wave_slices(lens, grid, eq_slices):
    """[(lo, hi)] of the waves of one launch over candidates `lens` (<= 4096), and whether the equal-slice rule of the
    single-query launch was taken."""
    T = int(tiles_of(lens).sum())
    n_waves = grid * M16_WAVES
    out = [(gw * T // n_waves, (gw + 1) * T // n_waves) for gw in range(n_waves)]
    taken = False
    if eq_slices:
        t = (T + n_waves - 1) // n_waves
        w_eff = (T + t - 1) // t if t > 0 else 0
        if 0 < t <= 10 and 4 * w_eff >= 3 * n_waves:
            taken = True
            out = [(gw * t, min(gw * t + t, T)) for gw in range(w_eff)]
    return [(lo, hi) for lo, hi in out if lo < hi], taken


def launches(cand_lens, form, num_cus=256):
    """The launches of one call as (lens of the launch's candidates, grid, eq_slices) per query of the launch.
    `cand_lens`: one list of lengths per query.  form "single": ts_launch_maxsim16 (chunks of 4096 candidates);
    "batch": ts_launch_maxsim16_batch (per-query calls where a query has more than 4096 candidates)."""
    out = []
    if form == "batch" and all(len(c) <= M16_MAX_DOCS for c in cand_lens):
        nq = len(cand_lens)
        max_cand = max(len(c) for c in cand_lens)
        grid = num_cus if nq == 1 else min(num_cus, max(1, (max_cand + 15) // 16))
        return [(list(c), grid, nq == 1) for c in cand_lens if len(c)]
    for c in cand_lens:
        for c0 in range(0, len(c), M16_MAX_DOCS):
            out.append((list(c[c0: c0 + M16_MAX_DOCS]), num_cus, True))
    return out


def slice_facts(cand_lens, form, passes, num_cus=256):
    """Which slice shapes the launches of one call contain."""
    facts = dict(starts_inside=False, register_path=False, three_waves=False, steps_over_empty=False,
                 eq_taken=False, eq_not_taken=False)
    for lens, grid, eq in launches(cand_lens, form, num_cus):
        tiles = tiles_of(lens)
        prefix = np.concatenate([[0], np.cumsum(tiles)])
        sl, taken = wave_slices(lens, grid, eq)
        if eq:
            facts["eq_taken" if taken else "eq_not_taken"] = True
        lo = np.array([s[0] for s in sl], np.int64)
        hi = np.array([s[1] for s in sl], np.int64)
        if lo.size == 0:
            continue
        first = np.searchsorted(prefix[:-1], lo, side="right") - 1          # the last candidate with prefix <= lo
        facts["starts_inside"] |= bool((lo - prefix[first] > 0).any())
        for c in range(len(lens)):
            a, b = prefix[c], prefix[c + 1]
            if tiles[c] >= 2 and passes == 1 and ((lo <= a) & (b <= hi)).any():
                facts["register_path"] = True
            if tiles[c] and ((lo < b) & (a < hi)).sum() >= 3:
                facts["three_waves"] = True
            if tiles[c] == 0 and ((lo < a) & (a < hi)).any():
                facts["steps_over_empty"] = True
    return facts


# ------------------------------------------------------------------------------------------------------- generators
def _j_of(norm2):
    """j with norm2 = 4^j (0 for an all-zero row); -1 where it is neither."""
    n = np.asarray(norm2, np.float64)
    with np.errstate(divide="ignore"):
        l4 = np.where(n > 0, np.log2(np.maximum(n, 1e-300)) / 2.0, 0.0)
    ok = (n == 0) | ((l4 == np.rint(l4)) & (n >= 1))
    return np.where(ok, np.rint(l4), -1).astype(np.int64)


def _row(rng, cols, H, sign=0, must=None, jmax=5):
    """One row, hot on a subset of `cols` (and at column `must`), entries of sign `sign` (0: random), norm^2 = 4^j."""
    cols = np.asarray(cols)
    room = cols.size
    feasible = [j for j in range(jmax + 1) if max(1, 4 ** j // 16) <= room]
    j = int(rng.choice(feasible))
    n2 = 4 ** j
    parts = [4] * (n2 // 16) if n2 >= 16 else ([2] if n2 == 4 else [1])
    for _ in range(int(rng.integers(0, 7))):                    # split a 4 into four 2s, a 2 into four 1s
        big = [i for i, v in enumerate(parts) if v > 1]
        if not big or len(parts) + 3 > room:
            break
        i = big[int(rng.integers(len(big)))]
        v = parts.pop(i)
        parts += [v // 2] * 4
    where = rng.permutation(cols)[: len(parts)]
    if must is not None and must not in where:
        where[0] = must
    out = np.zeros(H, np.float32)
    s = rng.choice([-1.0, 1.0], size=len(parts)) if sign == 0 else float(sign)
    out[where] = np.asarray(parts, np.float32) * s
    return out


def _scaled_copy(rng, tok):
    """tok times 1, 2 or 4, as far as the entries stay <= 4 and the norm^2 <= 4^5."""
    j = int(_j_of(float(tok.astype(np.float64) @ tok.astype(np.float64))))
    top = float(np.abs(tok).max())
    ok = [s for s in (1, 2, 4) if top * s <= 4 and j + int(np.log2(s)) <= 5]
    return tok * np.float32(rng.choice(ok))


def plant_positions(length):
    """Where a candidate of `length` rows gets planted rows, most important first."""
    pos = [length - 1, 0, 32, 31] + [r for r in range(63, length, 32)]
    seen, out = set(), []
    for p in pos:
        if 0 <= p < length and p not in seen:
            seen.add(p)
            out.append(p)
    return out


def default_lens(n, rng, top=192):
    lens = np.minimum(rng.integers(0, top + 1, size=n), rng.integers(0, top + 1, size=n))    # more short ones than long
    edge = [0, 1, 31, 32, 33, 64, 65, 192, 0, 96, 2]
    lens[: min(n, len(edge))] = edge[:n]
    return rng.permutation(lens)


def _gen_plant(H, Lq, lens, rng, kedge):
    n_special = (1 if Lq >= 2 else 0) + (1 if Lq >= 12 else 0)
    n_plant = min(8 if kedge else 9, Lq - n_special)
    anti_cols = np.array([1, H // 2, H // 2 + 1, H - 9]) if H >= 64 else np.array([1])
    free = np.setdiff1d(np.arange(H), anti_cols)
    if kedge:
        blocks = [np.array([H - 8 + i]) for i in range(n_plant)]
    else:
        w = max(1, min(8, free.size // n_plant))
        perm = rng.permutation(free)
        blocks = [perm[i * w: (i + 1) * w] for i in range(n_plant)]
    # roles of the query tokens: the planted ones sit at the ends of the query and around its 32-token tiles
    want = [t for t in (0, Lq - 1, 31, 32, 63, 64, 65) if 0 <= t < Lq]
    rest = [t for t in rng.permutation(Lq).tolist() if t not in want]
    order = list(dict.fromkeys(want))[:n_plant]
    order += rest[: n_plant - len(order)]
    others = [t for t in range(Lq) if t not in order]
    q = np.zeros((Lq, H), np.float32)
    for i, t in enumerate(order):
        q[t] = _row(rng, blocks[i], H)
    special = rng.permutation(others)[:n_special].tolist()
    zero_tok = special[0] if n_special >= 1 else None
    anti_tok = special[1] if n_special >= 2 else None
    for t in others:
        if t == zero_tok:
            continue
        q[t] = _row(rng, anti_cols, H, sign=-1) if t == anti_tok else _row(rng, free, H)
        while t != anti_tok and (_cosines(q[order], q[t: t + 1]) >= 1.0).any():     # never parallel to a planted token
            q[t] = _row(rng, free, H)
    # a pool of random document rows: >= 0 where the "anti" token is hot, never parallel to a planted token
    pool = np.stack([_row(rng, np.arange(H), H) for _ in range(256)])
    pool[:, anti_cols] = np.abs(pool[:, anti_cols])
    pool[rng.random(256) < 0.03] = 0.0
    cos = _cosines(q[order], pool)
    pool[(cos >= 1.0).any(axis=0)] = 0.0
    docs, plants = [], []
    for c, L in enumerate(lens):
        d = pool[rng.integers(0, 256, size=L)].copy()
        pos = plant_positions(L)
        k = min(len(pos), n_plant)
        if pos:
            rot = c % len(pos)
            pos = (pos[rot:] + pos[:rot])[:k]
            if L > 32 and all(p < 32 for p in pos):           # every candidate of several tiles has one past the first
                pos[-1] = L - 1
        mine = []
        for i, p in enumerate(pos):
            tok = order[(i + c) % n_plant]
            if L == 1:      # without its only row the candidate scores 0.0: its own score must not be 0.0 by chance
                tok = next(order[(c + s) % n_plant] for s in range(n_plant)
                           if _cosines(q, q[order[(c + s) % n_plant]][None]).sum() != 0)
            d[p] = _scaled_copy(rng, q[tok])
            mine.append((p, tok))
        docs.append(d)
        plants.append(mine)
    return q, docs, plants


def _gen_neg(H, Lq, lens, rng):
    hot = H // 3
    q = np.stack([_row(rng, np.arange(H), H, sign=-1, must=hot) for _ in range(Lq)])
    pool = np.stack([_row(rng, np.arange(H), H, sign=1, must=hot) for _ in range(256)])
    docs = []
    for c, L in enumerate(lens):
        d = pool[rng.integers(0, 256, size=L)].copy()
        if L and c % 3 == 0:
            d[int(rng.integers(L))] = 0.0
        docs.append(d)
    return q, docs, [[] for _ in lens]


def _gen_ones(H, Lq, lens, rng):
    q = np.stack([_row(rng, np.arange(H), H) for _ in range(Lq)])
    pool = np.stack([_row(rng, np.arange(H), H) for _ in range(256)])
    docs = []
    for L in lens:
        assert L >= Lq, "a candidate of the ones class holds every query token"
        d = pool[rng.integers(0, 256, size=L)].copy()
        at = rng.permutation(L)[:Lq]
        for t in range(Lq):
            d[at[t]] = _scaled_copy(rng, q[t])
        docs.append(d)
    return q, docs, [[] for _ in lens]


Case = namedtuple("Case", "name cls H Lq n stores seed lens_kind")
Data = namedtuple("Data", "q docs plants lens")


def case_lens(case):
    rng = np.random.default_rng([case.seed, 7])
    if case.lens_kind == "default":
        return default_lens(case.n, rng)
    if case.lens_kind == "short":                     # ~1.8 tiles per candidate: 1000 of them take the equal slices
        return default_lens(case.n, rng, top=113)
    if case.lens_kind == "one":
        return np.ones(case.n, np.int64)
    if case.lens_kind == "long":                      # the ones class: every candidate holds the whole query
        return rng.integers(case.Lq, 193, size=case.n)
    raise ValueError(case.lens_kind)


@functools.lru_cache(maxsize=6)
def generate(case, cls=None, lens=None):
    """Data(q [Lq, H], docs: list of [len, H], plants: per candidate [(row, query token)], lens) of a case; float32,
    read-only, cached.  `cls` / `lens` (a tuple) override the case's own (the stale-scratch pairs)."""
    cls = cls or case.cls
    lens = np.asarray(lens if lens is not None else case_lens(case), np.int64)
    rng = np.random.default_rng([case.seed, len(cls), case.H, case.Lq])
    if cls in ("plant", "kedge"):
        q, docs, plants = _gen_plant(case.H, case.Lq, lens, rng, cls == "kedge")
    elif cls == "neg":
        q, docs, plants = _gen_neg(case.H, case.Lq, lens, rng)
    else:
        q, docs, plants = _gen_ones(case.H, case.Lq, lens, rng)
    q.setflags(write=False)
    for d in docs:
        d.setflags(write=False)
    return Data(q, docs, plants, lens)


# ------------------------------------------------------------------------------------------------ integer reference
def _cosines(q, rows):
    """float64 cosines [Lq, rows] with the kernel's clamp; exact for guarded rows."""
    q, r = np.asarray(q, np.float64), np.asarray(rows, np.float64)
    qn = np.maximum(np.sqrt((q * q).sum(1)), 1e-12)
    rn = np.maximum(np.sqrt((r * r).sum(1)), 1e-12)
    return (q @ r.T) / qn[:, None] / rn[None, :]


def integer_cosines(q, rows):
    """int64 [Lq, rows]: cos(q_i, d_j) in units of 2^-10, by integer arithmetic; zero rows give cosine 0."""
    qi = np.rint(np.asarray(q, np.float64)).astype(np.int64)
    ri = np.rint(np.asarray(rows, np.float64)).astype(np.int64)
    jq = _j_of((qi * qi).sum(1))
    jd = _j_of((ri * ri).sum(1))
    assert (jq >= 0).all() and (jd >= 0).all(), "a row norm^2 is not a power of four"
    shift = SCALE_BITS - jq[:, None] - jd[None, :]
    assert (shift >= 0).all()
    return (qi @ ri.T) << shift                                          # exact: int64


def integer_maxima(q, docs):
    """int64 [n, Lq]: max_j cos(q_i, d_j) in units of 2^-10; the rows of an empty candidate stay 0."""
    lens = np.array([d.shape[0] for d in docs], np.int64)
    out = np.zeros((len(docs), np.shape(q)[0]), np.int64)
    if lens.sum() == 0:
        return out
    v = integer_cosines(q, np.concatenate([d for d in docs if d.shape[0]]))
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    live = lens > 0
    out[live] = np.maximum.reduceat(v, starts[live], axis=1).T
    return out


def maxsim_from_maxima(m, empty=None):
    """float32 [n] from integer maxima [n, Lq]: an integer sum S, then float32(S * 2^-10) / float32(Lq), one IEEE
    fp32 division of two exact operands — the only rounding."""
    m = np.asarray(m, np.int64)
    S = m.sum(1)
    num = (S.astype(np.float64) * 2.0 ** -SCALE_BITS).astype(np.float32)
    assert np.array_equal(num.astype(np.float64) * 2.0 ** SCALE_BITS, S.astype(np.float64))     # S * scale is an fp32 number
    out = (num / np.float32(m.shape[1])).astype(np.float32)
    if empty is not None:
        out[empty] = 0.0
    return out


def expected_maxsim(q, docs):
    """float32 [n]: the bits a correct kernel returns in maxsim mode (0.0 for an empty candidate)."""
    return maxsim_from_maxima(integer_maxima(q, docs), np.array([d.shape[0] == 0 for d in docs], bool))


def expected_colbert(q, docs, dtype=np.float64):
    """sum_i softmax(m)_i m_i from the exact maxima, evaluated in `dtype`."""
    m = (integer_maxima(q, docs).astype(np.float64) * 2.0 ** -SCALE_BITS).astype(dtype)
    e = np.exp(m - m.max(axis=1, keepdims=True))
    num, den = (e * m).sum(axis=1, dtype=dtype), e.sum(axis=1, dtype=dtype)
    out = (num / den).astype(dtype)
    out[[d.shape[0] == 0 for d in docs]] = 0.0
    return out


# ------------------------------------------------------------------------------------------------------------ guard
def assert_exactly_scored(q, docs, plants=None):
    """float64 / integer check of the rule above; returns the largest |dot product|."""
    allowed = np.array([0.0, 1.0, 2.0, 4.0])
    Lq = np.shape(q)[0]
    assert 1 <= Lq <= 192
    top = 0.0
    q64 = np.asarray(q, np.float64)
    for x in [q64] + [np.asarray(d, np.float64) for d in docs]:
        assert np.isin(np.abs(x), allowed).all(), "an entry outside {0, +-1, +-2, +-4}"
        j = _j_of((x * x).sum(1))
        assert (j >= 0).all() and (j <= 5).all(), "a row norm^2 is neither zero nor 4^j, j <= 5"
        if x is not q64 and x.shape[0]:
            top = max(top, float(np.abs(q64 @ x.T).max()), float((np.abs(q64) @ np.abs(x).T).max()))
    assert top < 2.0 ** 24
    m = integer_maxima(q, docs)
    assert np.abs(m).max() <= 1 << SCALE_BITS                            # cosines in [-1, 1], multiples of 2^-10
    assert np.abs(m).sum(1).max() < 1 << 24, "the sum of maxima is not exact in fp32"
    # (every partial sum of the maxima, in any order, is a multiple of 2^-10 below 2^24 units: an fp32 number)
    for c, mine in enumerate(plants or []):
        if not mine:
            continue
        cos = _cosines(q64, docs[c])
        toks = [t for _, t in mine]
        assert len(set(toks)) == len(toks), "two planted rows serve one query token"
        for p, t in mine:
            assert cos[t, p] == 1.0, "a planted row is not a copy of its token"
            assert (np.delete(cos[t], p) < 1.0).all(), "another row reaches the planted maximum"
            assert (np.delete(cos[:, p], t) < 1.0).all(), "a planted row raises another token's maximum to 1"
    return top


# -------------------------------------------------------------------------------------------------------- mutations
def drop_row(docs, c, p):
    out = list(docs)
    out[c] = np.delete(docs[c], p, axis=0)
    return out


def zero_k_step(docs, c, g, store):
    """Candidate c without the 32 bytes of k step g of each of its rows."""
    per = 32 // elem_bytes(store)
    out = list(docs)
    d = docs[c].copy()
    d[:, g * per: (g + 1) * per] = 0.0
    out[c] = d
    return out


def last_k_step(H, store):
    return (H * elem_bytes(store) - 1) // 32


def first_tile_only(docs):
    return [d[:32] for d in docs]


# ------------------------------------------------------------------------------------------------------- case table
ALL = STORES
BITS16 = ("f16", "bf16")
E4M3 = ("e4m3_f16", "e4m3_bf16")
N_CAND, N_WIDE, N_MANY = 150, 40, 1000


def _cases():
    out, seed = [], [0]

    def add(cls, H, Lq, stores, n=N_CAND, lens_kind="default"):
        seed[0] += 1
        out.append(Case(f"{cls}-H{H}-Lq{Lq}-n{n}", cls, H, Lq, n, tuple(stores), seed[0], lens_kind))

    # H = 64: 16-bit rows of 128 bytes (full = false, 12 padded k steps), e4m3 rows of two k steps, f32 of eight
    for Lq in (1, 5, 32, 33, 65, 150):
        add("plant", 64, Lq, ALL)
    add("neg", 64, 5, ALL)
    add("neg", 64, 65, ALL)
    add("kedge", 64, 40, ALL)
    # 1000 candidates at the smallest H of each store type: the equal slices of the single-query launch
    add("plant", 64, 33, BITS16 + E4M3, n=N_MANY, lens_kind="short")
    add("plant", 32, 5, ("f32",), n=N_MANY, lens_kind="short")
    # H = 104: 208-byte rows at 16 bit, the half k step; 416 bytes in f32
    add("kedge", 104, 5, BITS16 + ("f32",))
    add("kedge", 104, 40, BITS16 + ("f32",))
    add("plant", 104, 64, BITS16 + ("f32",))
    # f32: H = 32 (full = false), H = 128 (full = true); 16-bit and e4m3 rows of 64 / 32 bytes on the same data
    add("plant", 32, 5, ALL)
    add("kedge", 32, 40, ALL)
    add("plant", 128, 5, ALL)
    add("plant", 128, 40, ALL)
    add("neg", 128, 33, ALL)
    # H = 256: full = true at 16 bit and f32, e4m3 ring 16 with full = false
    for Lq in (32, 64, 65):
        add("plant", 256, Lq, ALL)
    add("kedge", 256, 5, ALL)
    add("neg", 256, 150, ALL)
    # H = 512: e4m3 ring 16, full = true
    add("plant", 512, 5, ALL)
    add("kedge", 512, 40, ALL)
    # H = 768: e4m3 ring 24; f32 with nqt = 1, so Lq = 33 takes two passes
    add("plant", 768, 5, ALL)
    add("plant", 768, 33, ALL)
    add("kedge", 768, 150, ALL)
    add("neg", 768, 32, E4M3 + ("f32",))
    # H = 2048: nqt forced to 1 at 16 bit and e4m3 (Lq = 33: two passes); f32 rows go to the general kernel
    add("plant", 2048, 5, ALL, n=N_WIDE)
    add("plant", 2048, 33, ALL, n=N_WIDE)
    add("kedge", 2048, 65, BITS16 + E4M3, n=N_WIDE)
    # the general kernel: a query image beyond LDS (vectorised loop), rows that are no multiple of 16 bytes (scalar)
    add("plant", 4096, 5, BITS16, n=N_WIDE)
    add("kedge", 4096, 40, BITS16, n=N_WIDE)
    add("plant", 50, 33, ("f32",))
    add("kedge", 100, 40, BITS16)
    add("neg", 100, 5, BITS16)
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]
CASE_STORES = [(c, s) for c in CASES for s in c.stores]
CASE_STORE_IDS = [f"{c.name}-{s}" for c, s in CASE_STORES]

# the stale-scratch pairs: launch A of the ones class, then launch B of the neg class on the same cells
STALE = [Case(f"stale-H{H}", "ones", H, 65, 48, st, 900 + i, "long")
         for i, (H, st) in enumerate(((256, ("bf16",) + E4M3), (768, ("f16",) + E4M3)))]
STALE_B2 = (31, 40)             # the second B: fewer candidates, another Lq (lq_pad 64 instead of 128)

# more than one launch
BEYOND_H, BEYOND_N, BEYOND_LQ = 64, 4100, 21
BEYOND_QUERIES = 70


def batch_plan(case):
    """The ragged batch every case is also scored as: (token slice, candidate indices) per query — the whole query
    on 20..60 candidates, a part of it on an empty list, two more parts on 20..60 candidates each."""
    rng = np.random.default_rng([case.seed, 11])
    Lq, n = case.Lq, case.n
    a = max(1, Lq // 3)
    toks = [(0, Lq), (Lq // 2, Lq), (0, a), (Lq - a, Lq)]
    plan = []
    for j, (t0, t1) in enumerate(toks):
        k = (20, 0, 60, int(rng.integers(20, 61)))[j]
        pick = rng.permutation(n)[:k]
        if j == 0:
            pick[0] = int(np.argmax(case_lens(case)))        # a long candidate: one wave walks several tiles of it
        plan.append(((t0, t1), pick))
    return plan


def beyond_case():
    return Case("beyond-one-launch", "plant", BEYOND_H, BEYOND_LQ, BEYOND_N, ("bf16",), 777, "one")
