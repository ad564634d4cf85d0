"""Adversarial inputs for the step that turns scores into ids: `select_kernel` (csrc/ts_select.hip) in its three modes
and the merge built on it ("selection order").

Three things live here, none of which needs a GPU:
  canonical_topk   the reference for one query, built on an integer key of its own;
  score sets and id layouts, each aimed at one data-dependent branch of the kernel, and the case tables made of them;
  select_plan / merge_plan   a Python mirror of the decisions of launch_select_t, select_kernel and merge_impl, so
                   that tests/test_select_host.py can show which case reaches which branch.

tests/test_select_host.py checks all of it; tests/test_select_gpu.py feeds the same tables to the kernels."""
import functools

import numpy as np

import exact_inputs as ex

FLT_MAX = np.float32(np.finfo(np.float32).max)
I64_MAX = np.iinfo(np.int64).max
I64_MIN = np.iinfo(np.int64).min


# ------------------------------------------------------------------------------------------------------ reference
def score_rank(scores):
    """int64, larger = better: the sign-magnitude reading of the float32 bits (so -0 and +0 both give 0 and the order
    of the finite values and the infinities is the numeric one); NaN of either sign or payload ranks below -inf."""
    s = np.ascontiguousarray(scores, np.float32)
    u = s.view(np.uint32).astype(np.int64)
    mag = u & 0x7FFFFFFF
    r = np.where(u >> 31, -mag, mag)
    return np.where(np.isnan(s), np.int64(-(1 << 40)), r)


def canonical_topk(scores, ids, k):
    """The k best entries of one query: score descending (-0 == +0, NaN last), exact ties by ascending id, equal ids
    by position; entries with id < 0 are padding and never returned; (-FLT_MAX, -1) fills the tail.  A returned zero
    is +0 whatever its sign was."""
    s = np.ascontiguousarray(scores, np.float32).ravel()
    i = np.asarray(ids, np.int64).ravel()
    assert s.shape == i.shape
    valid = np.flatnonzero(i >= 0)
    order = valid[np.lexsort((valid, i[valid], -score_rank(s[valid])))][:k]
    D = np.full(k, -FLT_MAX, np.float32)
    I = np.full(k, -1, np.int64)
    with np.errstate(invalid="ignore"):                # a signalling NaN stays a NaN
        D[: order.size] = s[order] + np.float32(0.0)
    I[: order.size] = i[order]
    return D, I


def canonical_merge(scores, ids, k):
    """canonical_topk of every query of lists [R, B, k']."""
    R, B, kk = scores.shape
    out = [canonical_topk(scores[:, b, :].ravel(), ids[:, b, :].ravel(), k) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def same_result(got, want):
    """ids equal; scores equal bit for bit, except that a NaN matches any NaN."""
    (D, I), (D0, I0) = got, want
    D, D0 = np.ascontiguousarray(D, np.float32), np.ascontiguousarray(D0, np.float32)
    if D.shape != D0.shape or not np.array_equal(np.asarray(I, np.int64), np.asarray(I0, np.int64)):
        return False
    nan = np.isnan(D0)
    return np.array_equal(np.isnan(D), nan) and np.array_equal(D.view(np.uint32)[~nan], D0.view(np.uint32)[~nan])


def first_k_ties_by_position(scores, ids, k, cap=1024):
    """The defect the merge had: of the entries that tie with the k-th score only the first `cap` BY POSITION are
    considered (the luckiest outcome of its race), the smallest ids among those are taken."""
    s = np.ascontiguousarray(scores, np.float32).ravel()
    i = np.asarray(ids, np.int64).ravel()
    r = score_rank(s)
    valid = np.flatnonzero(i >= 0)
    if valid.size <= k:
        return canonical_topk(s, i, k)
    kth = np.sort(r[valid])[::-1][k - 1]
    ties = valid[r[valid] == kth]
    drop = np.ones(s.size, bool)
    drop[valid[r[valid] > kth]] = False
    drop[ties[:cap]] = False
    return canonical_topk(s, np.where(drop, -1, i), k)


# ------------------------------------------------------------------------------------------------------ score sets
# gen(n, k, rng) -> float32 [n], in no particular order.  "rank k" below is the k-th best of the n entries.
def _distinct_vals(n, rng, lo=-40, hi=40, signs=(-1.0, 1.0)):
    """n different finite values: mantissas without repetition inside each of the binades lo..hi, both signs."""
    e = np.arange(lo, hi + 1)
    per = -(-n // (e.size * len(signs)))
    out = [sg * np.ldexp(1.0 + rng.choice(1 << 23, size=per, replace=False) * 2.0 ** -23, x) for x in e for sg in signs]
    v = np.concatenate(out).astype(np.float32)
    assert np.unique(v).size == v.size
    return rng.permutation(v)[:n]


def s_distinct(n, k, rng):
    return _distinct_vals(n, rng)                      # 81 binades, both signs


def s_all_equal(n, k, rng):
    return np.full(n, 0.75, np.float32)


def s_all_negative(n, k, rng):
    return _distinct_vals(n, rng, lo=-30, hi=30, signs=(-1.0,))


def s_two_level(delta):
    def gen(n, k, rng):
        m = int(np.clip(k + delta, 0, n))              # k = m - delta: delta in {+1, 0, -1} gives k = m-1, m, m+1
        v = np.full(n, -3.0, np.float32)
        v[rng.permutation(n)[:m]] = 5.0
        return v
    return gen


def s_shared_bytes(b):
    """Keys whose orderable 32-bit form agrees on exactly the top b bytes: 1 + j * 2^-23 with j below 2^(8 (4 - b)),
    the extremes of the first differing byte present."""
    top = 1 << (8 * (4 - b) - (1 if b == 1 else 0))    # b = 1: j < 2^23 keeps the exponent, the second byte still varies
    def gen(n, k, rng):
        j = rng.integers(0, top, size=n)
        j[rng.permutation(n)[:2]] = (0, top - 1)[: min(n, 2)]
        return (np.float32(1.0) + j.astype(np.float64) * 2.0 ** -23).astype(np.float32)
    return gen


def s_boundary_ties(t):
    """`above` distinct scores, then a class of t equal scores that straddles rank k, then distinct lower ones.
    t = None: the whole input tied (s_all_equal at another value)."""
    def gen(n, k, rng):
        if t is None:
            return np.full(n, -1.5, np.float32)
        tt = min(t, n)
        above = int(np.clip(k - (tt + 1) // 2, 0, n - tt))
        v = np.empty(n, np.float32)
        v[:above] = 2.0 + np.arange(above, dtype=np.float32)
        v[above: above + tt] = 1.0
        v[above + tt:] = -np.arange(n - above - tt, dtype=np.float32)
        return rng.permutation(v)
    return gen


def s_signed_zeros(n, k, rng):
    v = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 2.0 ** -140], np.float32), size=n)
    return v.astype(np.float32)


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def s_specials(n, k, rng):
    """Merge only: NaN of both signs and two payloads, +-inf, denormals, +-FLT_MAX, zeros, among ordinary values."""
    pool = np.concatenate([_f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFABCDEF, 0x7F800000, 0xFF800000,
                                 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF,
                                 0x00000000, 0x80000000]), np.array([1.0, -1.0, 3.5, -2.25], np.float32)])
    v = pool[rng.integers(0, pool.size, size=n)]
    v[: min(n, pool.size)] = pool[: min(n, pool.size)]
    return rng.permutation(v)


def s_nan_heavy(n, k, rng):
    """Merge only: a few finite scores, NaN everywhere else.  With the `nan_padding` ids fewer than k entries are valid
    and more than 1024 of them are NaN: the k-th key is a padding key and every NaN entry is wanted."""
    v = np.full(n, np.nan, np.float32)
    m = min(300, n // 4)
    v[rng.permutation(n)[:m]] = rng.integers(-50, 50, size=m).astype(np.float32)
    return v


NAN_KEPT = 1500        # valid-id NaN entries of the `nan_padding` layout

SCORE_SETS = {
    "distinct": s_distinct, "all_equal": s_all_equal, "all_negative": s_all_negative,
    "two_level(k+1)": s_two_level(+1), "two_level(k)": s_two_level(0), "two_level(k-1)": s_two_level(-1),
    "shared_bytes(1)": s_shared_bytes(1), "shared_bytes(2)": s_shared_bytes(2), "shared_bytes(3)": s_shared_bytes(3),
    "ties(2)": s_boundary_ties(2), "ties(1023)": s_boundary_ties(1023), "ties(1024)": s_boundary_ties(1024),
    "ties(1025)": s_boundary_ties(1025), "ties(5000)": s_boundary_ties(5000), "ties(all)": s_boundary_ties(None),
    "signed_zeros": s_signed_zeros, "specials": s_specials, "nan_heavy": s_nan_heavy,
}
FINITE_SETS = tuple(s for s in SCORE_SETS if s not in ("specials", "nan_heavy"))


# ------------------------------------------------------------------------------------------------------ id layouts
# layout(R, k, rng) -> int64 [R, k]: the id of the entry at position j of list r
def i_contiguous(R, k, rng):
    return (np.arange(R)[:, None] * (k + 11) + np.arange(k)[None, :]).astype(np.int64)      # shard r owns a row range


def i_interleaved(R, k, rng):
    return (np.arange(k)[None, :] * R + np.arange(R)[:, None]).astype(np.int64)             # id = j * R + r


def i_descending(R, k, rng):
    return (R * k - 1 - (np.arange(R)[:, None] * k + np.arange(k)[None, :])).astype(np.int64)


def i_huge(R, k, rng):
    base = i_interleaved(R, k, rng)
    return np.where(base % 2 == 0, (1 << 32) + 5 + base, I64_MAX - base)      # above 2^32, and down from 2^63 - 1


def i_duplicate(R, k, rng):
    ids = i_interleaved(R, k, rng)
    if R > 1:
        ids[R - 1, :] = ids[0, :]                      # the last list repeats the ids of the first
    return ids


def i_negative(R, k, rng):
    ids = i_interleaved(R, k, rng)
    bad = rng.random((R, k)) < 0.3
    return np.where(bad, rng.choice(np.array([-1, -2, -7, I64_MIN]), size=(R, k)), ids)


def i_all_padding(R, k, rng):
    return rng.choice(np.array([-1, -2, I64_MIN]), size=(R, k)).astype(np.int64)


def i_nan_padding(R, k, rng):
    """Interleaved; merge_query then turns every NaN entry but the first NAN_KEPT (by position) into padding."""
    return i_interleaved(R, k, rng)


ID_LAYOUTS = {"nan_padding": i_nan_padding, "contiguous": i_contiguous, "interleaved": i_interleaved, "descending": i_descending, "huge": i_huge,
              "duplicate": i_duplicate, "negative": i_negative, "all_padding": i_all_padding}

# The ONE merge table: every score set on contiguous and on interleaved ids, the other layouts on the sets where the
# tie rule decides (and on the specials); a query of padding only.
MERGE_TABLE = tuple([(s, l) for s in SCORE_SETS for l in ("contiguous", "interleaved")] +
                    [(s, l) for s in ("all_equal", "ties(1025)", "ties(5000)", "two_level(k+1)", "specials", "distinct")
                     for l in ("descending", "huge", "duplicate", "negative")] +
                    [("distinct", "all_padding"), ("nan_heavy", "nan_padding")])
MERGE_SHAPES = ((1, 1), (2, 1), (3, 7), (2, 1024), (3, 1024), (8, 1000), (8, 2048), (7, 2049), (2, 8192), (3, 8192),
                (17, 1000), (5, 8192))
MERGE_K_UNSUPPORTED = 8193
MANY_TIES = ("all_equal", "ties(1025)", "ties(5000)", "ties(all)", "two_level(k+1)", "two_level(k-1)")


@functools.lru_cache(maxsize=None)
def _merge_query(score_set, layout, R, k):
    rng = np.random.default_rng([R, k, sorted(SCORE_SETS).index(score_set), sorted(ID_LAYOUTS).index(layout)])
    s = SCORE_SETS[score_set](R * k, k, rng).reshape(R, k)
    s = np.take_along_axis(s, np.argsort(-score_rank(s), axis=1, kind="stable"), axis=1)   # every list best first
    ids = ID_LAYOUTS[layout](R, k, rng)
    if layout == "nan_padding":
        ids = ids.copy()
        ids.ravel()[np.flatnonzero(np.isnan(s.ravel()))[NAN_KEPT:]] = -1
    s.setflags(write=False)
    ids.setflags(write=False)
    return s, ids


def merge_query(score_set, layout, R, k):
    """(scores float32 [R, k], ids int64 [R, k]) of one query: every list sorted by score, ids by position (so
    inside a tie class the ids come in the layout's order, not necessarily ascending).  Cached, read-only."""
    return _merge_query(score_set, layout, R, k)


def merge_batch(cases, R, k):
    """Lists [R, B, k] with one table entry per query."""
    qs = [merge_query(s, l, R, k) for s, l in cases]
    return (np.ascontiguousarray(np.stack([q[0] for q in qs], axis=1)),
            np.ascontiguousarray(np.stack([q[1] for q in qs], axis=1)))


def merge_batches(R, k):
    """The whole table at one shape as [(cases, B)]: B = 1 for every entry, then B = 3 in consecutive triples (a
    different score set per query)."""
    out = [((c,), 1) for c in MERGE_TABLE]
    step = 3
    out += [(tuple(MERGE_TABLE[(i + j) % len(MERGE_TABLE)] for j in range(step)), 3) for i in range(0, len(MERGE_TABLE), step)]
    return out


# --------------------------------------------------------------------------------------- planted (index-driven) cases
# Scores reach SEL_DENSE / SEL_PAIRS32 through an index: corpus [n, 40] in f16 or bf16 holds them, the queries are
# rows of the identity, so score[q][i] = corpus[i][q] exactly.  Everything is an integer number of UNIT below 2^24,
# with at most 8 significant bits per corpus value (bf16) — a distribution that needs more mantissa than that spreads
# its bytes over up to three more columns and its query is the sum of their identity rows (products of 1, added
# exactly: ex.assert_exactly_summable holds for the whole corpus).
PLANT_D = 40
UNIT = 2.0 ** -8
PLANT_N = (1, 33, 1061, 16384, 16385, 20011)
PLANT_K = (1, 2, 3, 1000, 1024, 1025, 2048, 2049, 5000, "n", "n+3")
MAX_KERNEL_K = 16384


def _p_distinct(n, rng, sign=None):
    """Integers of 8 significant bits below 2^23, both signs, as many different ones as there are (8446), repeated
    beyond that: ids break those ties."""
    m = np.concatenate([np.arange(1, 256)] + [np.arange(128, 256) << s for s in range(1, 16)])
    v = np.concatenate([m, -m]) if sign is None else sign * m
    v = rng.permutation(v)
    return np.resize(v, n)


def _p_two_level(m):
    def gen(n, rng):
        v = np.full(n, -768, np.int64)
        v[rng.permutation(n)[: min(m, n)]] = 1280
        return v
    return gen


def _p_ties(t, above):
    def gen(n, rng):
        tt = min(t, n)
        a = min(above, n - tt)
        v = np.empty(n, np.int64)
        v[:a] = 1 << 22                                # more than 255 different values are not needed above the class:
        v[:a] += (np.arange(a) % 128) << 15            # ids break the ties among them
        v[a: a + tt] = 1 << 21
        v[a + tt:] = -(np.arange(n - a - tt) % 255) - 1
        return rng.permutation(v)
    return gen


def _p_shared(b):
    def gen(n, rng):
        top = 1 << (8 * (4 - b) - (1 if b == 1 else 0))
        j = rng.integers(0, top, size=n)
        j[rng.permutation(n)[:2]] = (0, top - 1)[: min(n, 2)]
        return (1 << 23) + j                           # 2^23 .. 2^24 - 1 units: one binade, 24 bits
    return gen


def _p_signed_zeros(n, rng):
    return rng.choice(np.array([0, 0, 0, 1, -1]), size=n)


PLANTED = {
    "distinct": lambda n, rng: _p_distinct(n, rng),
    "all_equal": lambda n, rng: np.full(n, 192, np.int64),
    "all_negative": lambda n, rng: _p_distinct(n, rng, sign=-1),
    "two_level(2)": _p_two_level(2), "two_level(1001)": _p_two_level(1001), "two_level(1024)": _p_two_level(1024),
    "two_level(2048)": _p_two_level(2048), "two_level(5000)": _p_two_level(5000),
    "shared_bytes(1)": _p_shared(1), "shared_bytes(2)": _p_shared(2), "shared_bytes(3)": _p_shared(3),
    "ties(2)": _p_ties(2, 999), "ties(1023)": _p_ties(1023, 500), "ties(1024)": _p_ties(1024, 500),
    "ties(1025)": _p_ties(1025, 500), "ties(5000)": _p_ties(5000, 100),
    "signed_zeros": _p_signed_zeros,
}


def _byte_columns(v):
    """An integer below 2^24 as up to three columns of at most 8 significant bits each (all of one sign)."""
    a = np.abs(v)
    assert (a < (1 << 24)).all()
    if ((a // np.maximum(a & -a, 1)) < 256).all():     # 8 significant bits everywhere: one column
        return [v]
    cols = [np.sign(v) * (a & m) for m in (0xFF0000, 0xFF00, 0xFF)]
    return [c for c in cols if c.any()]


@functools.lru_cache(maxsize=4)
def planted(n, names=tuple(PLANTED), seed=0):
    """(corpus float32 [n, 40], queries float32 [len(names), 40], units int64 [len(names), n]) — units * UNIT are the
    planted scores, also what the queries score against the corpus.  Cached, read-only."""
    corpus = np.zeros((n, PLANT_D), np.float64)
    queries = np.zeros((len(names), PLANT_D), np.float32)
    units = np.zeros((len(names), n), np.int64)
    col = 0
    for q, name in enumerate(names):
        rng = np.random.default_rng([seed, n, sorted(PLANTED).index(name)])
        v = np.asarray(PLANTED[name](n, rng), np.int64)
        units[q] = v
        for c in _byte_columns(v):
            corpus[:, col] = c * UNIT
            queries[q, col] = 1.0
            col += 1
    assert col <= PLANT_D, col
    corpus = corpus.astype(np.float32)
    for a in (corpus, queries, units):
        a.setflags(write=False)
    return corpus, queries, units


def planted_scores(units):
    return (np.asarray(units, np.float64) * UNIT).astype(np.float32)


def fits_16bit(x):
    """True where every value survives float16 AND bfloat16 storage."""
    x = np.ascontiguousarray(x, np.float32)
    bf = (x.view(np.uint32) & np.uint32(0xFFFF)) == 0
    with np.errstate(over="ignore"):
        return bool(bf.all() and np.array_equal(x.astype(np.float16).astype(np.float32), x))


def plant_ks(n):
    """The k of PLANT_K the select kernels serve at n rows (k above 16384 on more rows than that is the slow path)."""
    out = []
    for k in PLANT_K:
        k = n if k == "n" else n + 3 if k == "n+3" else k
        if k > MAX_KERNEL_K and n > MAX_KERNEL_K:
            continue
        if k not in out:
            out.append(k)
    return out


def planted_topk(units, k, allowed=None, id_offset=0):
    """canonical_topk of the planted scores of every query; rows outside `allowed` (bool [n], or one per query) are
    padding."""
    S = planted_scores(units)
    n = S.shape[1]
    out = []
    for q in range(S.shape[0]):
        ids = np.arange(n, dtype=np.int64)
        a = allowed[q] if isinstance(allowed, (list, tuple)) else allowed
        if a is not None:
            ids = np.where(np.asarray(a, bool), ids, -1)
        D, I = canonical_topk(S[q], ids, k)
        out.append((D, np.where(I >= 0, I + id_offset, -1)))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# chunked dense: two chunks of the dense path (1 << 20 rows each), the second one 40 rows
CHUNK_ROWS = 1 << 20
N_CHUNKED = CHUNK_ROWS + 40
K_CHUNKED = 100


@functools.lru_cache(maxsize=1)
def chunked():
    """(corpus [N_CHUNKED, 40], queries [3, 40], units [3, N_CHUNKED]).  Query 0: low noise, top scores planted in both
    chunks and one tie class across the chunk boundary that straddles rank 100; query 1: every score negative (the
    padding of the short chunk's list, -FLT_MAX, must still lose); query 2: everything equal."""
    n = N_CHUNKED
    rng = np.random.default_rng(77)
    u = np.zeros((3, n), np.int64)
    u[0] = rng.integers(-200, 56, size=n)
    u[0, [5, 70_001, CHUNK_ROWS - 2, CHUNK_ROWS + 1, CHUNK_ROWS + 38]] = (240 << 8, 232 << 8, 224 << 8, 248 << 8, 216 << 8)
    tie = np.concatenate([rng.permutation(CHUNK_ROWS - 64)[:120] + 32, [CHUNK_ROWS - 1, CHUNK_ROWS, CHUNK_ROWS + 39],
                          CHUNK_ROWS + 10 + np.arange(12)])
    u[0, tie] = 128 << 8
    u[1] = -(rng.integers(1, 256, size=n) << rng.integers(0, 12, size=n))
    u[2] = 160
    corpus = np.zeros((n, PLANT_D), np.float32)
    queries = np.zeros((3, PLANT_D), np.float32)
    for q in range(3):
        corpus[:, q] = u[q] * UNIT
        queries[q, q] = 1.0
    return corpus, queries, u


# masked dense (SEL_PAIRS32 with -1 ids): allowed sets of 0, 5, k-1, k and k+1 rows out of 20011
N_MASKED, K_MASKED = 20011, 1000
MASKED_COUNTS = (0, 5, K_MASKED - 1, K_MASKED, K_MASKED + 1)


MASKED_DIRECT = (16384, 100)     # and one size that fits LDS: no global pass, the in-LDS select works among the -1 ids


def masked_direct_set():
    return np.random.default_rng(6).random(MASKED_DIRECT[0]) < 0.5


MASKED_NAMES = ("distinct", "ties(1025)", "all_equal", "two_level(1001)", "shared_bytes(3)")   # one per allowed set


def masked_sets():
    rng = np.random.default_rng(5)
    out = []
    for c in MASKED_COUNTS:
        m = np.zeros(N_MASKED, bool)
        m[rng.permutation(N_MASKED)[:c]] = True
        out.append(m)
    return out


# filter path: n = ex.N_FILTER; k = 2048 needs 32 k rows to stay on it (ts_index_filter_path), hence the second size
FILTER_K = (1, 10, 1000, 2048)
N_FILTER_2048 = 32 * 2048 + 37
FILTER_ON_PATH = ("distinct", "shared_bytes(3)")
FILTER_ANY_PATH = ("all_equal", "two_level(1001)")


def filter_path_expected(n, k):
    """ts_index.hip's rule for the filter path (kMaxFilterK, kMinFilterRows, 32 k rows)."""
    return k <= 2048 and n >= 32768 and n >= 32 * k


def sample_rank(n, k):
    """The rank tau_kernel is asked for on the five-launch filter path (ts_index.hip sample_geometry, corpora whose
    sample is smaller than one round of scan waves): <= 64 takes tau_kernel<1>, above that tau_kernel<4>."""
    nblk = -(-n // 32)
    nsb = min(nblk, max(8192, n // 128) // 32)
    S = nsb * 32
    over = 3 if k > 1024 else 4
    return max(24, -(-over * k * S // n))


# ---------------------------------------------------------------------------------------------- the kernel's decisions
SEL_DENSE, SEL_PAIRS32, SEL_MERGE64 = "dense", "pairs32", "merge64"
LDS_KEYS_CAP = 16384          # TS_SEL_LDS_KEYS
SEL_THREADS = 1024
SEL_OUT_CAP = 2048
SEL_TIE_CAP = 1024


def kernel_keys(mode, scores, ids=None, id_base=0):
    """load_key of ts_select.hip: orderable(score) << 32 | (0xFFFFFFFF - tiebreak); 0 for padding.  The tiebreak is
    the row (dense), the int32 id (pairs32) or the position (merge64)."""
    s = np.ascontiguousarray(scores, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        u = (s + np.float32(0.0)).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    key = np.where(np.isnan(s), np.uint32(0), key).astype(np.uint64)
    pos = np.arange(s.size, dtype=np.uint64)
    if mode == SEL_DENSE:
        tb, pad = pos + np.uint64(id_base), np.zeros(s.size, bool)
    elif mode == SEL_PAIRS32:
        i = np.asarray(ids, np.int64).ravel()
        tb, pad = (i & 0xFFFFFFFF).astype(np.uint64), i < 0
    else:
        tb, pad = pos, np.asarray(ids, np.int64).ravel() < 0
    out = (key << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - tb)
    return np.where(pad, np.uint64(0), out)


def _pow2_at_least(x, least=2):
    p = least
    while p < x:
        p <<= 1
    return p


def _radix(keys, krem, first_pass, stop_at_score_bits):
    """The MSB-first 8-bit radix select of both phases: (threshold T, passes run, bits decided, whole bin wanted)."""
    cand = keys
    prefix, bits, passes, whole = (int(keys.max()) >> (64 - 8 * first_pass)) if first_pass else 0, 8 * first_pass, 0, False
    if first_pass:
        cand = cand[(cand >> np.uint64(64 - bits)) == np.uint64(prefix)]
    for p in range(first_pass, 8):
        digit = ((cand >> np.uint64(56 - 8 * p)) & np.uint64(0xFF)).astype(np.int64)
        hist = np.bincount(digit, minlength=256)
        at_least = np.cumsum(hist[::-1])[::-1]                       # votes in bins >= b
        b = int(np.flatnonzero((at_least >= krem) & (at_least - hist < krem))[0])
        krem -= int(at_least[b] - hist[b])
        whole = int(hist[b]) == krem
        prefix, bits, passes = (prefix << 8) | b, bits + 8, passes + 1
        cand = cand[digit == b]
        if whole or (stop_at_score_bits and bits == 32):
            break
    return (prefix << (64 - bits)) if bits < 64 else prefix, passes, bits, whole


def select_plan(mode, n, k, keys, n_cap=None):
    """What one launch of select_kernel<mode> does with the n keys of one query (kernel_keys): a dict of
      lds_keys, phase1 ('direct' | 'global'), global_passes, global_early_exit,
      phase2 ('taken' | 'skipped: count <= 2 pk' | 'skipped: pk > 2048'), skip_raw, skip, ending ('whole bin' |
      'score bits' | 'all 64 bits'), tie_class, want, sort ('register' | 'lds'), P, k_above_n, unsupported."""
    keys = np.asarray(keys, np.uint64)
    assert keys.size == n
    nmax = n_cap if n_cap is not None else n
    plan = dict(mode=mode, n=n, k=k, unsupported=False, global_passes=0, global_early_exit=None, skip_raw=None, skip=None,
                ending=None, tie_class=0, want=0, every_tie_taken=False, k_above_n=k > n)
    lds_keys = _pow2_at_least(min(nmax, LDS_KEYS_CAP))
    if nmax > LDS_KEYS_CAP:
        if k > LDS_KEYS_CAP:
            plan["unsupported"] = True
            return plan
        lds_keys = _pow2_at_least(k)
    plan["lds_keys"] = lds_keys
    kk = min(k, n)
    if n > lds_keys:
        plan["phase1"] = "global"
        T, passes, bits, whole = _radix(keys, kk, 0, False)
        plan["global_passes"], plan["global_early_exit"] = passes, passes < 8
        keys = keys[(keys >= np.uint64(T)) & (keys != 0)][:lds_keys]
    else:
        plan["phase1"] = "direct"
    count = keys.size
    pk = _pow2_at_least(kk)
    if kk >= 1 and pk <= SEL_OUT_CAP and count > 2 * pk:
        plan["phase2"] = "taken"
        diff = int(np.bitwise_and.reduce(keys)) ^ int(np.bitwise_or.reduce(keys))
        raw = (64 - diff.bit_length()) >> 3 if diff else 7
        skip = min(raw, 3) if mode == SEL_MERGE64 else raw
        plan["skip_raw"], plan["skip"] = raw, skip
        T, passes, bits, whole = _radix(keys, kk, skip, mode == SEL_MERGE64)
        plan["ending"] = "all 64 bits" if bits == 64 else "whole bin" if whole else "score bits"
        if mode == SEL_MERGE64 and not whole:
            sk, sT = keys >> np.uint64(32), np.uint64(T >> 32)
            c1 = int(((sk > sT) & (keys != 0)).sum())
            plan["tie_class"], plan["want"] = int(((sk == sT) & (keys != 0)).sum()), kk - c1
            plan["every_tie_taken"] = plan["want"] >= plan["tie_class"]      # the k-th key is a padding key
            count = kk
        else:
            count = int(((keys >= np.uint64(T)) & (keys != 0)).sum())
        count = min(count, SEL_OUT_CAP)
    else:
        plan["phase2"] = "skipped: pk > 2048" if (kk >= 1 and pk > SEL_OUT_CAP) else "skipped: count <= 2 pk"
    plan["P"] = _pow2_at_least(count)
    plan["sort"] = "register" if plan["P"] <= SEL_THREADS else "lds"
    return plan


def merge_plan(scores, ids, k):
    """merge_impl for ONE query's lists [R, k]: dict(form 'once' | 'grouped', groups, last_group, depth, launches =
    [select_plan of every launch], unsupported)."""
    R = scores.shape[0]
    if k > LDS_KEYS_CAP // 2:
        return dict(form=None, unsupported=True, launches=[], depth=0, groups=0, last_group=0)
    def once(s, i):
        return select_plan(SEL_MERGE64, s.size, k, kernel_keys(SEL_MERGE64, s.ravel(), i.ravel()))
    if R * k <= LDS_KEYS_CAP:
        return dict(form="once", unsupported=False, launches=[once(scores, ids)], depth=0, groups=1, last_group=R)
    per = LDS_KEYS_CAP // k
    groups = [(g, min(g + per, R)) for g in range(0, R, per)]
    launches, ts, ti = [], [], []
    for a, b in groups:
        launches.append(once(scores[a:b], ids[a:b]))
        D, I = canonical_topk(scores[a:b].ravel(), ids[a:b].ravel(), k)
        ts.append(D)
        ti.append(I)
    inner = merge_plan(np.stack(ts), np.stack(ti), k)
    return dict(form="grouped", unsupported=False, launches=launches + inner["launches"], depth=1 + inner["depth"],
                groups=len(groups), last_group=groups[-1][1] - groups[-1][0])


# Branches the tables do not reach, with the reason (tests/test_select_host.py asserts that they stay unreached, so
# that this list cannot go stale):
UNREACHED = {
    ("merge64", "phase1", "global"): "merge_impl never hands one launch more than 16384 entries (it merges in groups)",
    ("dense", "skip", 4): "keys that agree on the score and differ in id bits 24..31: one launch never spans 2^24 rows "
                          "(dense chunks are 2^20 rows)",
    ("dense", "skip", 5): "needs tied rows 2^16 apart among more than 2 pk entries in LDS: a direct launch holds at "
                          "most 16384 rows and the survivors of a global pass are k entries, so phase 2 is not taken",
    ("pairs32", "skip", 4): "ids 2^24 apart with equal scores in one candidate list: corpora of more than 16 M rows, "
                            "out of a test's size",
    ("pairs32", "skip", 5): "ids 2^16 apart with equal scores among more than 2 pk candidates: the planted cases of "
                            "that size tie in thousands and leave the filter path",
    ("pairs32", "filter lists", "not planned"): "the candidate lists of the filter path (flat and IVF) depend on the "
                                               "sampled threshold tau, so their plan is not computed; the GPU tests "
                                               "assert the path and the sample rank instead",
    ("pairs32", "skip", 1): "a -1 id makes a zero key, so the masked lists share no byte (skip = 0); the lists without "
                            "padding are the filter path's (not planned); the template is the one SEL_DENSE reaches "
                            "skip 1, 2, 3, 6 and 7 with",
    ("pairs32", "sort", "lds"): "the masked cases end in at most 1024 survivors (k = 1000 and 100); the LDS sort of "
                                "this template runs in SEL_DENSE and in the filter searches at k = 2048",
    ("dense", "tie_class", "any"): "the tie list exists in SEL_MERGE64 only (keys of the other modes are unique)",
}
