"""Bit-level host model of what goes into a stage-1 index and into a query image.

Rows going in: ``row_den_kernel``, ``relayout_kernel`` and ``reconstruct_kernel`` (ts_scan.hip) with the host and device
drivers ``ts_index_add`` / ``ts_index_reconstruct`` (ts_index.hip).  Queries going in: ``qprep_kernel``,
``qprep_f32s_kernel`` and ``q_unit`` / ``build_qimage`` of ``fused_kernel``.

Everything here is numpy; tests/test_ingest_model_host.py checks the model itself (against a search over all 65 536
patterns of a storage type, against fp32 emulations of the kernel's reduction, and against planted defects) and
tests/test_ingest_gpu.py holds the kernels to it by bits.

Values travel as float32 arrays.  A 16-bit *input* is a float32 array whose every value is a number of that type
(``representable``); the GPU tests turn it into a tensor of the type without rounding.
"""
import functools
import math

import numpy as np

from oracle import oracle

F32 = np.float32
STORAGE = ("f16", "bf16", "f32")
INPUTS = ("f32", "f16", "bf16")
FLT_MAX = F32(np.finfo(np.float32).max)
EPS = F32(1e-8)                       # the epsilon of x / (|x| + 1e-8), as the kernel's float literal
INF_PATTERN = {"f16": 0x7C00, "bf16": 0x7F80}
TOP = {"f16": 2.0 ** 16, "bf16": 2.0 ** 128}          # the power of two above the largest finite value
STAGE_BYTES = 64 << 20                # the staging buffer of ts_index_add / ts_index_reconstruct


# ------------------------------------------------------------------------------------------------------- rounding
def round_to(x, T):
    """float32 -> storage type T -> float32, round to nearest even: ``oracle.quantize``; the identity for f32."""
    with np.errstate(over="ignore"):                    # beyond the largest finite value: inf, as intended
        return oracle.quantize(np.ascontiguousarray(x, dtype=F32), T)


def patterns(T):
    """The float32 value of each of the 65 536 bit patterns of T, by pattern."""
    p = np.arange(65536, dtype=np.uint32)
    if T == "f16":
        return p.astype(np.uint16).view(np.float16).astype(F32)
    return (p << 16).view(F32)


@functools.lru_cache(maxsize=None)
def _magnitudes(T):
    """float64 magnitudes of the patterns 0 .. inf pattern, ascending: every non-negative finite value of T, then the
    power of two that follows the largest one.  The index of a magnitude is its bit pattern, so an even index is an
    even mantissa, and the last index is the pattern of +inf."""
    m = patterns(T)[: INF_PATTERN[T] + 1].astype(np.float64)
    m[-1] = TOP[T]
    assert (np.diff(m) > 0).all()
    return m


def round_by_search(x, T):
    """The nearest value of T to each float32 x, found by a search over all patterns of T (exact float64 distances),
    ties to the even mantissa; what lies at or beyond the midpoint between the largest finite value and the next power
    of two becomes inf (IEEE 754 round to nearest even); NaN stays NaN; the sign of x is kept, also on zero."""
    x = np.ascontiguousarray(x, dtype=F32)
    m = _magnitudes(T)
    nan = np.isnan(x)
    a = np.abs(np.where(nan, F32(0), x).astype(np.float64))
    hi = np.clip(np.searchsorted(m, a, side="left"), 1, len(m) - 1)       # m[hi-1] < a <= m[hi], clipped
    lo = hi - 1
    dlo, dhi = a - m[lo], m[hi] - a
    pick = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    pick = np.where(np.isinf(a), len(m) - 1, pick)
    val = patterns(T)[pick]
    out = np.copysign(val, x).astype(F32)
    out[nan] = np.nan
    return out


def truncate_to(x, T):
    """A planted defect: round toward zero instead of to nearest (bf16: keep the upper 16 bits)."""
    x = np.ascontiguousarray(x, dtype=F32)
    if T == "bf16":
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    r = round_to(x, T)
    over = np.abs(r) > np.abs(x)
    return np.where(over, np.nextafter(r.astype(np.float16), np.float16(0)).astype(F32), r)


def round_sig(x, bits):
    """Normal float32 values rounded (nearest even) to ``bits`` significant bits: the intermediate of a planted
    double rounding."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    sh = np.uint64(24 - bits)
    one = np.uint64(1)
    r = ((u + ((one << sh >> one) - one) + ((u >> sh) & one)) >> sh) << sh
    return r.astype(np.uint32).view(F32)


def representable(x, T):
    """True where the float32 x is a number of T (NaN counts)."""
    x = np.ascontiguousarray(x, dtype=F32)
    r = round_to(x, T)
    return (r.view(np.uint32) == x.view(np.uint32)) | np.isnan(x)


def mismatches(got, want):
    """Flat indices at which two float32 arrays differ: NaN equals NaN whatever its payload, everything else is
    compared by bits, so -0 is not +0."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32)))
    return np.flatnonzero(bad.reshape(-1))


def assert_same_bits(got, want, what=""):
    bad = mismatches(got, want)
    if bad.size:
        g, w = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
        i = int(bad[0])
        cols = np.shape(want)[-1] if np.ndim(want) > 1 else 1
        raise AssertionError(f"{what}: {bad.size} of {w.size} values differ, first at flat {i} (row {i // cols}, col "
                             f"{i % cols}): got {g[i]!r} (0x{g[i:i + 1].view(np.uint32)[0]:08x}) want {w[i]!r} "
                             f"(0x{w[i:i + 1].view(np.uint32)[0]:08x})")


# ------------------------------------------------------------------------------------------------- edge catalogues
def _f32_exact(v64):
    v = v64.astype(F32)
    assert (v.astype(np.float64) == v64).all(), "a catalogue value is not a float32 number"
    return v


@functools.lru_cache(maxsize=None)
def edge_catalogue(T):
    """{name: float32 values} for a 16-bit storage type T.  Both signs everywhere.
      patterns    every finite pattern of T
      midpoints   the midpoint of each non-negative finite value and its successor in magnitude (the last successor is
                  the power of two beyond the largest finite value: that midpoint is the overflow threshold); exact
      mid_below   the float32 predecessor (toward zero) of each midpoint
      mid_above   the float32 successor (away from zero) of each midpoint
      specials    +-0, half the smallest subnormal with its float32 neighbours, the largest finite value, the overflow
                  threshold with its neighbours, FLT_MAX, +-inf, NaN, float32 subnormals"""
    m = _magnitudes(T)
    fin = patterns(T)
    fin = fin[np.isfinite(fin)]
    mid = _f32_exact((m[:-1] + m[1:]) / 2.0)
    below, above = np.nextafter(mid, F32(0)), np.nextafter(mid, F32(np.inf))
    tiny, top, thr = _f32_exact(m[1:2] / 2.0)[0], F32(m[-2]), mid[-1]
    sp = [F32(0.0), tiny, np.nextafter(tiny, F32(0)), np.nextafter(tiny, F32(1)), top, thr, np.nextafter(thr, F32(0)),
          np.nextafter(thr, F32(np.inf)), FLT_MAX, F32(np.inf), F32(2.0 ** -149), F32(2.0 ** -127), F32(3 * 2.0 ** -140),
          np.nextafter(F32(2.0 ** -126), F32(0))]
    sp = np.array(sp, dtype=F32)
    both = lambda v: np.concatenate([v, -v]).astype(F32)
    out = {"patterns": fin, "midpoints": both(mid), "mid_below": both(below), "mid_above": both(above),
           "specials": np.concatenate([both(sp), np.array([np.nan], dtype=F32)])}
    for v in out.values():
        v.setflags(write=False)
    return out


def catalogue_values(T):
    """The whole edge catalogue of T as one float32 vector (about 4 x 65 536 values)."""
    return np.concatenate(list(edge_catalogue(T).values()))


def cross_catalogue(in_dtype):
    """All 65 536 patterns of a 16-bit input type (inf and NaN included), for an index of the other 16-bit type."""
    return patterns(in_dtype)


def pack_rows(values, d):
    """A vector as rows of d, the tail padded with zeros."""
    v = np.ascontiguousarray(values, dtype=F32)
    n = -(-v.size // d)
    out = np.zeros(n * d, dtype=F32)
    out[: v.size] = v
    return out.reshape(n, d)


def rounding_input(in_dtype, T):
    """The values a rounding test feeds for (input type, storage type): the storage type's edge catalogue for float32
    input (both catalogues for float32 storage, where nothing may change), all patterns of a 16-bit input."""
    if in_dtype == "f32":
        return catalogue_values(T) if T != "f32" else np.concatenate([catalogue_values("f16"), catalogue_values("bf16")])
    return cross_catalogue(in_dtype)


def stored(rows, in_dtype, T, normalize=False):
    """What ``reconstruct_n`` must return for rows added without normalisation: the input widened exactly, rounded
    once to T; for f32 storage the input's bits."""
    assert not normalize, "normalised rows: stored_exact_norm / stored_bracket"
    rows = np.ascontiguousarray(rows, dtype=F32)
    assert representable(rows, in_dtype).all()
    return round_to(rows, T)


# ------------------------------------------------------------------------------ normalisation, class 1: exact rows
# (elements ; norm): Pythagorean triples and quadruples, every norm odd, so no product of them is a power of two
BASE_TUPLES = (((3, 4), 5), ((5, 12), 13), ((8, 15), 17), ((1, 2, 2), 3), ((2, 3, 6), 7), ((1, 4, 8), 9),
               ((2, 6, 9), 11), ((6, 6, 7), 11), ((4, 4, 7), 9), ((2, 10, 11), 15))
N_LIMIT = 4096                         # N < 2^12, so N^2 < 2^24
EXPONENTS = {"f32": (0, 20, -31, -53), "bf16": (0, 20, -31, -53), "f16": (0, 3, -24)}


def _compose(rng, cap):
    """One integer tuple with a perfect-square sum of squares: an outer tuple (c_i ; n) whose element i is replaced,
    sometimes, by c_i times an inner tuple scaled to the common norm L: sum = n^2 L^2.  At most ``cap`` elements."""
    while True:
        outer, n = BASE_TUPLES[rng.integers(len(BASE_TUPLES))]
        inner = [BASE_TUPLES[rng.integers(len(BASE_TUPLES))] if rng.random() < 0.6 else ((1,), 1) for _ in outer]
        L = 1
        for _, m in inner:
            L = L * m // math.gcd(L, m)
        s = int(rng.integers(1, 4))
        N = n * L * s
        elems = [c * (L // m) * s * b for c, (bs, m) in zip(outer, inner) for b in bs]
        if N < N_LIMIT and len(elems) <= cap:
            assert sum(e * e for e in elems) == N * N
            return elems, N


def exact_norm_rows(n, d, in_dtype="f32", seed=0):
    """Class 1: ``(rows float32 [n, d], N int64 [n], e int64 [n])``.  Row i holds integers with sum of squares N_i^2 <
    2^24 (N_i not a power of two) at shuffled positions with shuffled signs, times 2^e_i; every element is a number of
    ``in_dtype``.  The exponents cycle through EXPONENTS[in_dtype]: 0 (the epsilon is absorbed: den == N), a large
    one, about 2^-20 / N (the epsilon changes den), and, for the types that reach it, 2^-53 (den is nearly the
    epsilon, the quotients land in f16's subnormal range)."""
    rng = np.random.default_rng([seed, n, d, INPUTS.index(in_dtype)])
    rows = np.zeros((n, d), dtype=F32)
    Ns, es = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    exps = EXPONENTS[in_dtype]
    for i in range(n):
        e = exps[i % len(exps)]
        while True:
            elems, N = _compose(rng, d)
            v = np.ldexp(np.array(elems, dtype=np.float64), e).astype(F32)
            if representable(v, in_dtype).all() and (np.ldexp(np.array(elems, np.float64), e) == v).all():
                break
        v = v * rng.choice(np.array([-1.0, 1.0], dtype=F32), size=v.size)
        rows[i, rng.permutation(d)[: v.size]] = v
        Ns[i], es[i] = N, e
    return rows, Ns, es


def exact_den(N, e):
    """den = fl32(N * 2^e + fl32(1e-8)): N * 2^e is the exact square root of an exact fp32 sum, so the kernel's
    denominator is this one fp32 addition."""
    root = np.ldexp(np.asarray(N, dtype=np.float64), np.asarray(e)).astype(F32)
    return (root + EPS).astype(F32)


def degenerate_rows(d, in_dtype="f32"):
    """``(rows, den)``: a zero row (den = 1e-8, stored as zeros), rows with every |v| < 2^-75 (the sum of squares
    underflows to 0: den = fl32(1e-8)), rows at 2^70 (the sum is inf: every element is stored as a zero) -- those of
    them that ``in_dtype`` can express."""
    k = np.arange(d)
    rows = [np.zeros(d)]
    den = [EPS]
    if in_dtype != "f16":
        small = (1 + k % (31 if in_dtype == "f32" else 15)) * 2.0 ** -80 * np.where(k % 3 == 0, -1.0, 1.0)
        rows += [small, small[::-1] * 2.0 ** -40]
        den += [EPS, EPS]
        big = np.where(k % 2 == 0, 1.0, -1.5) * 2.0 ** 70
        rows += [big, np.where(k == d // 2, 2.0 ** 70, 0.0)]
        den += [F32(np.inf), F32(np.inf)]
    rows = np.array(rows, dtype=np.float64).astype(F32)
    assert representable(rows, in_dtype).all()
    return rows, np.array(den, dtype=F32)


def stored_exact_norm(rows, den, T, epsilon=True, reciprocal=False):
    """round_to(fl32(v / den), T), bit for bit.  ``epsilon=False`` and ``reciprocal=True`` are planted defects (the
    caller passes den without the epsilon; v * fl32(1 / den) instead of the division)."""
    rows = np.ascontiguousarray(rows, dtype=F32)
    den = np.asarray(den, dtype=F32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        q = (rows * (F32(1.0) / den).astype(F32)).astype(F32) if reciprocal else (rows / den).astype(F32)
    return round_to(q, T)


# --------------------------------------------------------------------- fp32 emulations of row_den_kernel's reduction
def _mul_add(s, v, fma):
    """s + v * v in fp32: fused (the exact float64 product, one rounding of the sum) or as two fp32 operations."""
    if fma:
        return (s.astype(np.float64) + v.astype(np.float64) * v.astype(np.float64)).astype(F32)
    return (s + (v * v).astype(F32)).astype(F32)


def sumsq_lane_strided(rows, fma=True):
    """The kernel's order: lane l adds k = l, l + 64, ...; then six butterfly steps (xor 32, 16, ... 1); lane 0."""
    rows = np.ascontiguousarray(rows, dtype=F32)
    n, d = rows.shape
    pad = np.zeros((n, -(-d // 64) * 64), dtype=F32)
    pad[:, :d] = rows
    s = np.zeros((n, 64), dtype=F32)
    with np.errstate(all="ignore"):
        for t in range(pad.shape[1] // 64):
            live = min(64, d - 64 * t)                      # lanes with k < dim take the step, the others do not
            s[:, :live] = _mul_add(s[:, :live], pad[:, 64 * t: 64 * t + live], fma)
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            s = (s + s[:, lanes ^ off]).astype(F32)
    return s[:, 0]


def sumsq_sequential(rows, fma=True, reverse=False):
    rows = np.ascontiguousarray(rows, dtype=F32)
    if reverse:
        rows = rows[:, ::-1]
    s = np.zeros(rows.shape[0], dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(rows.shape[1]):
            s = _mul_add(s, rows[:, k], fma)
    return s


def emulated_den(rows, fma=True):
    with np.errstate(all="ignore"):
        return (np.sqrt(sumsq_lane_strided(rows, fma)).astype(F32) + EPS).astype(F32)


# ---------------------------------------------------------------------------- normalisation, class 2: general rows
def beta(d):
    """Relative bound of the kernel's denominator against the float64 |x| + 1e-8 (derivation: DESIGN.md 4.16 and
    test_ingest_model_host.py): ceil(d / 64) + 6 roundings of the sum, halved by the root, one for the root, one for
    the addition, all doubled."""
    return (-(-d // 64) + 10) * 2.0 ** -24


def general_rows(n, d, in_dtype="f32", seed=0):
    """Class 2: standard normal times 3, rounded to the input type."""
    rng = np.random.default_rng([seed, n, d, 77])
    return round_to((rng.standard_normal((n, d)) * 3).astype(F32), in_dtype)


def den64(rows):
    return np.sqrt((np.asarray(rows, np.float64) ** 2).sum(axis=1)) + 1e-8


def _f32_down(x64):
    f = x64.astype(F32)
    return np.where(f.astype(np.float64) > x64, np.nextafter(f, F32(-np.inf)), f).astype(F32)


def _f32_up(x64):
    f = x64.astype(F32)
    return np.where(f.astype(np.float64) < x64, np.nextafter(f, F32(np.inf)), f).astype(F32)


def den_bracket(rows):
    """(den_lo, den_hi): the fp32 numbers bracketing den64 * (1 -+ beta(d))."""
    d64, b = den64(rows), beta(np.shape(rows)[1])
    return _f32_down(d64 * (1 - b)), _f32_up(d64 * (1 + b))


def stored_bracket(rows, T):
    """(lo, hi) float32 [n, d]: division and rounding are monotone, so each stored element lies between
    round_to(fl32(v / den_lo), T) and round_to(fl32(v / den_hi), T) (ordered here by value)."""
    dl, dh = den_bracket(rows)
    a, b = stored_exact_norm(rows, dl, T), stored_exact_norm(rows, dh, T)
    return np.minimum(a, b), np.maximum(a, b)


def undecided_share(rows, T):
    lo, hi = stored_bracket(rows, T)
    return float((lo != hi).mean())


def assert_in_bracket(got, rows, T, what=""):
    lo, hi = stored_bracket(rows, T)
    got = np.asarray(got, dtype=F32)
    bad = np.argwhere(~((got >= lo) & (got <= hi)))
    assert bad.size == 0, (f"{what}: {bad.shape[0]} elements outside the bracket, first at {bad[0].tolist()}: got "
                           f"{got[tuple(bad[0])]!r}, bracket [{lo[tuple(bad[0])]!r}, {hi[tuple(bad[0])]!r}]")


# ------------------------------------------------------------------------------------- the layout, for planted defects
def layout_roundtrip(rows, defect=None):
    """relayout_kernel followed by reconstruct_kernel for 16-bit storage, element by element: the value that k of a row
    comes back with sits in group g = k // 16, lane half h = (k // 8) % 2, element e = k % 8 (frag_k: k = 16 g + 8 h +
    e); elements 2j and 2j + 1 share a 32-bit word, low half first.  Defects: "swap16" writes the pair's halves the
    other way round; "k+8" maps the second lane half 8 further when writing."""
    rows = np.ascontiguousarray(rows, dtype=F32)
    n, d = rows.shape
    k = np.arange(d)
    g, h, e = k // 16, (k // 8) % 2, k % 8
    if defect == "swap16":
        e = e ^ 1
    src = 16 * g + 8 * h + e + (8 * h if defect == "k+8" else 0)
    out = np.zeros_like(rows)
    ok = src < d
    out[:, k[ok]] = rows[:, src[ok]]
    return out


# --------------------------------------------------------------------------------------------- host chunk loops
# The dimensions of the chunk-loop test: 4096 where the flat index takes it; 16-bit storage keeps 32 queries of d
# elements in LDS beside its staging area, in groups of 16 k that come eight at a time (ts_make_layout), which ends at
# 2176 on the MI355X's 160 KiB.
CHUNK_D = (4096, 2176)


def chunk_rows(d, elem_bytes=4):
    """Rows per staging chunk of ts_index_add / ts_index_reconstruct: max(1, 64 MiB // row bytes)."""
    return max(1, STAGE_BYTES // (d * elem_bytes))


def chunked_copy(n, chunk, ignore_r0=False):
    """Source row of every destination row after the drivers' loop ``for r0 in range(0, n, chunk)``; the planted
    defect reads every chunk from the start of the source."""
    src = np.empty(n, dtype=np.int64)
    for r0 in range(0, n, chunk):
        c = min(chunk, n - r0)
        src[r0: r0 + c] = np.arange(c) + (0 if ignore_r0 else r0)
    return src


# ------------------------------------------------------------------------------------------------- probe corpora
def probe_corpus(n, d):
    """Row i = e_(i mod d) * 2^-((i div d) mod 8): exact in every storage type.  Returns (rows, k, scale)."""
    i = np.arange(n)
    k, scale = i % d, 2.0 ** -((i // d) % 8)
    rows = np.zeros((n, d), dtype=F32)
    rows[i, k] = scale
    return rows, k, scale


def in_query_range(q, T):
    """Finite after rounding to T, and zero or with a magnitude in [2^-60, 2^60] (where the three truncated terms of
    the bf16x3 split add up to q exactly and no product with a row scale leaves the normal range)."""
    q = np.ascontiguousarray(q, dtype=F32)
    a = np.abs(q)
    return np.isfinite(round_to(q, T)) & ((a == 0) | ((a >= 2.0 ** -60) & (a <= 2.0 ** 60)))


def probe_queries(B, d, in_dtype, T, seed=0):
    """[B, d] queries drawn from the edge catalogue (of T; of both 16-bit types for f32 storage), numbers of
    ``in_dtype``, in range.  The first values of each row walk the catalogue in order, so every kind of entry occurs."""
    rng = np.random.default_rng([seed, B, d, INPUTS.index(in_dtype), STORAGE.index(T)])
    pool = rounding_input(in_dtype, T)
    pool = pool[in_query_range(pool, T) & representable(pool, in_dtype)]
    q = pool[rng.integers(0, pool.size, size=(B, d))]
    q.setflags(write=False)
    return q


def probe_scores(q, T, k, scale):
    """float64 scores [B, n] of the probe corpus: round_to(q[b, k_i], T) * scale_i, exactly -- one product is non-zero
    and the accumulator starts at +0, so a zero score is +0 whatever the sign of the query element."""
    rq = round_to(q, T).astype(np.float64)
    s = rq[:, k] * scale[None, :]
    return np.where(s == 0, 0.0, s)


def probe_topk(q, T, k_of_row, scale, k, allowed=None):
    """(D float32 [B, k], I int64 [B, k]) by score descending, then id ascending; -FLT_MAX / -1 padding."""
    s = probe_scores(q, T, k_of_row, scale)
    if allowed is not None:
        s = np.where(np.asarray(allowed, bool)[None, :], s, -np.inf)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    top = np.take_along_axis(s, order, axis=1)
    got = np.isfinite(top)
    D = np.full((s.shape[0], k), -FLT_MAX, dtype=F32)
    I = np.full((s.shape[0], k), -1, dtype=np.int64)
    D[:, : order.shape[1]] = np.where(got, top, -FLT_MAX).astype(F32)
    I[:, : order.shape[1]] = np.where(got, order, -1)
    return D, I


def max_tie_multiplicity(q, T, k_of_row, scale, k):
    """The largest number of rows that share one score among each query's k best scores."""
    s = probe_scores(q, T, k_of_row, scale)
    worst = 0
    for row in s:
        kth = np.sort(row)[::-1][min(k, row.size) - 1]
        vals, counts = np.unique(row[row >= kth], return_counts=True)
        worst = max(worst, int(counts.max()))
    return worst
