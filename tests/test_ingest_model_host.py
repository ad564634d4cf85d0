"""The ingest model checked on its own, without a GPU: its rounding against a search over all
patterns, every catalogue entry against the property its name claims, the exact rows against fp32 emulations of the
kernel's reduction in three orders, the bound beta(d) against the emulation of the kernel's own order, the probe
corpora against a float32 matmul, the chunk sizes, and each planted defect against the entries that catch it."""
import numpy as np
import pytest

import exact_inputs as ex
import ingest_model as im
from oracle import oracle

F32 = np.float32
BRACKET_D = (40, 100, 768, 1536)


# ----------------------------------------------------------------------------------------------------- rounding
@pytest.mark.parametrize("T", ["f16", "bf16"])
def test_round_to_is_the_nearest_pattern_with_ties_to_even(T):
    """round_to (numpy's cast for f16, integer arithmetic for bf16) against the search over all patterns of T, on the
    whole edge catalogue and on both cross-type catalogues."""
    for name, v in list(im.edge_catalogue(T).items()) + [("all f16 patterns", im.cross_catalogue("f16")),
                                                          ("all bf16 patterns", im.cross_catalogue("bf16"))]:
        with np.errstate(over="ignore"):
            im.assert_same_bits(im.round_to(v, T), im.round_by_search(v, T), f"{T} {name}")
    assert im.catalogue_values(T).size > 3.8 * 65536


@pytest.mark.parametrize("T", ["f16", "bf16"])
def test_catalogue_entries_are_what_their_names_claim(T):
    cat = im.edge_catalogue(T)
    pat = cat["patterns"]
    assert pat.size == 2 * im.INF_PATTERN[T] and np.isfinite(pat).all()
    assert im.mismatches(im.round_to(pat, T), pat).size == 0                 # patterns are fixed points, -0 included
    assert np.signbit(pat).sum() == pat.size // 2
    with np.errstate(over="ignore"):
        mid, below, above = (im.round_to(cat[n], T) for n in ("midpoints", "mid_below", "mid_above"))
    m = cat["midpoints"]
    half = m.size // 2
    mag = im._magnitudes(T)
    lo, hi = mag[:-1], mag[1:]                                               # the neighbours of each midpoint
    # a tie: both neighbours are equally far (exact in float64), and the model picks the even one
    assert ((m[:half].astype(np.float64) - lo) == (hi - m[:half].astype(np.float64))).all()
    even = np.where(np.arange(lo.size) % 2 == 0, lo, hi)
    even[-1] = np.inf                                                        # the overflow threshold goes to inf
    assert np.array_equal(mid[:half].astype(np.float64), even)
    assert np.array_equal(mid[half:].astype(np.float64), -even)
    # the float32 neighbours of a tie round apart: to the value below and to the value above
    hi_inf = hi.copy()
    hi_inf[-1] = np.inf
    assert np.array_equal(below[:half].astype(np.float64), lo) and np.array_equal(above[:half].astype(np.float64), hi_inf)
    assert np.array_equal(below[half:].astype(np.float64), -lo) and np.array_equal(above[half:].astype(np.float64), -hi_inf)
    assert (np.signbit(below[half:])).all()                                  # -(half the smallest subnormal)- -> -0
    # the specials land where stated
    top = F32(mag[-2])
    r = lambda v: im.round_to(np.array([v], dtype=F32), T)[0]
    tiny = F32(mag[1] / 2)
    assert r(tiny) == 0 and r(np.nextafter(tiny, F32(0))) == 0 and r(np.nextafter(tiny, F32(1))) == F32(mag[1])
    thr = m[half - 1]
    with np.errstate(over="ignore"):
        assert r(top) == top and r(np.nextafter(thr, F32(0))) == top and np.isinf(r(thr)) and np.isinf(r(np.nextafter(thr, F32(np.inf))))
        assert np.isinf(r(im.FLT_MAX)) and np.isinf(r(F32(np.inf))) and np.isnan(r(F32(np.nan)))
    if T == "f16":
        assert top == 65504 and thr == 65520
        assert r(F32(2.0 ** -149)) == 0 and r(F32(2.0 ** -127)) == 0          # float32 subnormals vanish in f16
    else:
        assert r(F32(2.0 ** -127)) == F32(2.0 ** -127)                        # ... and are bf16 subnormals where they fit
        assert r(F32(2.0 ** -149)) == 0 and r(np.nextafter(F32(2.0 ** -126), F32(0))) == F32(2.0 ** -126)
    sp = cat["specials"]
    assert np.isnan(sp).sum() == 1 and np.isinf(sp).sum() == 2 and (sp == 0).sum() == 2


def test_cross_type_catalogues_round_overflow_and_underflow():
    f16, bf16 = im.cross_catalogue("f16"), im.cross_catalogue("bf16")
    assert f16.size == bf16.size == 65536
    to_bf = im.round_to(f16, "bf16")
    fin = np.isfinite(f16)
    assert (to_bf[fin] != f16[fin]).mean() > 0.8                              # 11 -> 8 significant bits: real rounding
    ties = fin & ((f16.view(np.uint32) & 0xFFFF) == 0x8000)                   # exactly half a bf16 step
    assert ties.sum() > 3000 and ((to_bf[ties].view(np.uint32) >> 16) & 1 == 0).all()
    assert (to_bf[fin & (f16 != 0)] != 0).all()                               # every f16 subnormal is a bf16 normal
    with np.errstate(over="ignore"):
        to_h = im.round_to(bf16, "f16")
    finb = np.isfinite(bf16)
    assert np.isinf(to_h[finb & (np.abs(bf16) >= 65520)]).all() and (np.abs(bf16[finb]) >= 65520).sum() > 28000
    assert (to_h[finb & (np.abs(bf16) <= 2.0 ** -25)] == 0).all() and (to_h[finb & (np.abs(bf16) > 2.0 ** -25)] != 0).all()
    sub = finb & (np.abs(bf16) > 2.0 ** -25) & (np.abs(bf16) < 2.0 ** -14)
    assert sub.sum() > 2000 and (np.abs(to_h[sub]) < 2.0 ** -14).mean() > 0.99   # f16 subnormals
    assert np.array_equal(np.signbit(to_h[finb]), np.signbit(bf16[finb]))     # -0 on underflow


def test_stored_is_one_rounding_of_the_exact_widening():
    for in_dtype in im.INPUTS:
        for T in im.STORAGE:
            v = im.rounding_input(in_dtype, T)
            assert im.representable(v, in_dtype).all()
            with np.errstate(over="ignore"):
                s = im.stored(im.pack_rows(v, 40), in_dtype, T)
            if T == "f32" or T == in_dtype:
                assert im.mismatches(s, im.pack_rows(v, 40)).size == 0        # the input's bits
    sub = im.patterns("f16")[1:0x400]                                         # f16 subnormals widen exactly
    assert (sub > 0).all() and (sub < 2.0 ** -14).all() and np.array_equal(sub.astype(np.float64), np.arange(1, 0x400) * 2.0 ** -24)


# --------------------------------------------------------------------------------------------------- class 1 rows
@pytest.mark.parametrize("in_dtype", im.INPUTS)
@pytest.mark.parametrize("d", [8, 40, 99, 768])
def test_exact_rows_have_an_exact_norm_in_every_order(in_dtype, d):
    rows, N, e = im.exact_norm_rows(96, d, in_dtype, seed=1)
    assert im.representable(rows, in_dtype).all()
    ints = np.ldexp(rows.astype(np.float64), -e[:, None])
    assert np.array_equal(ints, np.rint(ints))
    assert np.array_equal((ints ** 2).sum(axis=1), (N * N).astype(np.float64)) and (N * N < 2 ** 24).all()
    assert ((N & (N - 1)) != 0).all()                                         # no power of two
    assert set(e) == set(im.EXPONENTS[in_dtype])
    want = np.ldexp((N * N).astype(np.float64), 2 * e)
    for fma in (True, False):
        for got in (im.sumsq_lane_strided(rows, fma), im.sumsq_sequential(rows, fma),
                    im.sumsq_sequential(rows, fma, reverse=True)):
            assert np.array_equal(got.astype(np.float64), want)
    root = np.sqrt(im.sumsq_lane_strided(rows)).astype(F32)
    assert np.array_equal(root.astype(np.float64), np.ldexp(N.astype(np.float64), e))     # the root is exact
    den = im.exact_den(N, e)
    assert np.array_equal(den, im.emulated_den(rows)) and np.array_equal(den, im.emulated_den(rows, fma=False))
    assert (den[e == 0] == N[e == 0]).all() and (den[e == 20].astype(np.float64) == np.ldexp(N[e == 20].astype(np.float64), 20)).all()
    small = e < -20
    assert (den[small].astype(np.float64) != np.ldexp(N[small].astype(np.float64), e[small])).all()   # the epsilon counts
    if in_dtype != "f16":
        q = im.stored_exact_norm(rows[e == -53], den[e == -53], "f16")
        nz = q[rows[e == -53] != 0]
        assert (np.abs(nz) < 2.0 ** -14).all() and (nz != 0).mean() > 0.5     # quotients in f16's subnormal range


def test_degenerate_rows_agree_with_the_oracle():
    for in_dtype in im.INPUTS:
        rows, den = im.degenerate_rows(40, in_dtype)
        assert len(rows) == (1 if in_dtype == "f16" else 5)
        with np.errstate(all="ignore"):
            assert im.mismatches(im.emulated_den(rows), den).size == 0
            assert im.mismatches(im.emulated_den(rows, fma=False), den).size == 0
            want = oracle.normalize_embeddings(rows)
        assert want.dtype == np.float32
        got = im.stored_exact_norm(rows, den, "f32")
        assert im.mismatches(got, want).size == 0
        assert (got[0] == 0).all()
        if in_dtype != "f16":
            assert (np.abs(rows[1:3]) < 2.0 ** -75).all() and (rows[1:3] != 0).all() and (got[1:3] != 0).all()
            assert (got[3:] == 0).all() and np.array_equal(np.signbit(got[3:]), np.signbit(rows[3:]))


# --------------------------------------------------------------------------------------------------- class 2 rows
@pytest.mark.parametrize("d", [40, 99, 100, 768, 1536, 4096])
def test_beta_bounds_the_emulated_denominator(d):
    """den = fl32(fl32(sqrt(S)) + eps), S the lane-strided fp32 sum.  Every partial sum is a sum of non-negative
    terms, so each of the r roundings on the way to lane 0 moves it by at most u = 2^-24 relatively: lane 0's chain
    has ceil(d / 64) additions (fused with their products; unfused, the product's rounding adds one more per step
    and stays inside the doubling) and the butterfly 6, |S / S64 - 1| <= (1 + u)^r - 1 ~ r u.  The root halves a
    relative error and rounds once, the addition of 1e-8 (positive) rounds once more:
    (ceil(d / 64) + 6) / 2 + 2 = ceil(d / 64) / 2 + 5 units, doubled as margin: beta(d) = (ceil(d / 64) + 10) u."""
    assert im.beta(d) == (-(-d // 64) + 10) * 2.0 ** -24
    worst = 0.0
    for in_dtype in im.INPUTS:
        rows = im.general_rows(200, d, in_dtype, seed=3)
        d64 = im.den64(rows)
        for fma in (True, False):
            worst = max(worst, float(np.abs(im.emulated_den(rows, fma).astype(np.float64) / d64 - 1).max()))
        lo, hi = im.den_bracket(rows)
        den = im.emulated_den(rows)
        assert ((lo <= den) & (den <= hi)).all()
    print(f"\nd={d}: emulated |den / den64 - 1| <= {worst / 2.0 ** -24:.2f} x 2^-24, beta = {im.beta(d) / 2.0 ** -24:.0f} x 2^-24")
    assert worst <= im.beta(d) / 2                                            # the margin is there


@pytest.mark.parametrize("T", ["f16", "bf16"])
def test_the_bracket_leaves_at_most_one_percent_undecided(T):
    """The condition of the issue: at most 1 % of the elements have two different ends.  Measured: f16 0.16 %, 0.22 %,
    0.40 %, 0.60 % at d = 40, 100, 768, 1536; bf16 under 0.1 %."""
    for d in BRACKET_D:
        for in_dtype in im.INPUTS:
            rows = im.general_rows(300, d, in_dtype)
            share = im.undecided_share(rows, T)
            print(f"\n{T} d={d} {in_dtype} rows: {100 * share:.2f} % undecided")
            assert share <= 0.01
            got = im.stored_exact_norm(rows, im.emulated_den(rows), T)
            im.assert_in_bracket(got, rows, T)                                # the emulated kernel passes its own check


# ------------------------------------------------------------------------------------------------- probe corpora
@pytest.mark.parametrize("T,d", [("f16", 40), ("bf16", 99), ("f32", 100), ("f32", 600)])
def test_probe_corpus_reads_back_the_rounded_queries(T, d):
    n = d + 37
    rows, k, scale = im.probe_corpus(n, d)
    assert (im.round_to(rows, "f16") == rows).all() and (im.round_to(rows, "bf16") == rows).all()
    assert ((rows != 0).sum(axis=1) == 1).all() and (scale[:d] == 1).all() and (scale[d:] == 0.5).all()
    for in_dtype in im.INPUTS:
        q = im.probe_queries(33, d, in_dtype, T)
        assert im.representable(q, in_dtype).all() and im.in_query_range(q, T).all()
        rq = im.round_to(q, T)
        assert np.isfinite(rq).all()
        got = rq @ rows.T                                                     # float32 matmul: one product per score
        want = im.probe_scores(q, T, k, scale)
        assert np.array_equal(got.astype(np.float64), want)
        assert np.array_equal(want[:, :d], rq.astype(np.float64))             # scores == round_to(q)
        if T == "f32":                                                        # the three truncated terms add to q exactly
            s3 = ex.split3(q)
            assert np.array_equal(s3["h"] + s3["m"] + s3["l"], q.astype(np.float64))
        if in_dtype == "f32" and T != "f32":
            assert (rq != q).mean() > 0.5                                     # the queries really are rounded


@pytest.mark.parametrize("d", [128, 99])
def test_probe_topk_has_the_stated_tie_multiplicity(d):
    """Rows that share a dimension and a scale tie exactly: ceil(n / (8 d)) of them; scores equal through a power of
    two add a few more.  A few dozen at most, far below any candidate list."""
    n = ex.N_FILTER
    rows, k, scale = im.probe_corpus(n, d)
    per = -(-n // (8 * d))
    for T in im.STORAGE:
        q = im.probe_queries(8, d, "f32", T, seed=5)
        m = im.max_tie_multiplicity(q, T, k, scale, 100)
        assert per - 1 <= m <= 3 * per, (m, per)
        D, I = im.probe_topk(q, T, k, scale, 100)
        assert (np.diff(D.astype(np.float64), axis=1) <= 0).all()
        same = np.diff(D, axis=1) == 0
        assert (np.diff(I, axis=1)[same] > 0).all()                          # ties by ascending id


# ---------------------------------------------------------------------------------------------------- chunk sizes
def test_chunk_rule_gives_two_chunks_with_a_partial_one():
    """The shapes of test_ingest_gpu.py's chunk-loop test, at both dimensions it may run (ingest_model.CHUNK_D)."""
    for d in im.CHUNK_D:
        chunk = im.chunk_rows(d)
        assert chunk == (64 << 20) // (4 * d) and chunk >= 1
        n = chunk + 33
        starts = list(range(0, n, chunk))
        assert len(starts) == 2 and n - starts[-1] == 33                     # a second chunk, and a partial one
        assert n % 32 != 0                                                    # the index ends inside a row block
    assert im.chunk_rows(4096) % 32 == 0 and im.chunk_rows(2176) % 32 == 30   # the second chunk starts on / inside a block
    assert im.chunk_rows(1 << 30) == 1


# ------------------------------------------------------------------------------------------------ planted defects
def _names_hit(T, faulty):
    """The catalogue entries of T on which a faulty rounding differs from the model."""
    hit = {}
    for name, v in im.edge_catalogue(T).items():
        with np.errstate(all="ignore"):
            hit[name] = im.mismatches(faulty(v), im.round_to(v, T)).size
    return hit


def test_planted_truncation_is_caught_by_the_upper_neighbours():
    hit = _names_hit("bf16", lambda v: im.truncate_to(v, "bf16"))
    assert hit["patterns"] == 0 and hit["mid_above"] >= 2 * 0x7F7F and hit["midpoints"] >= 0x7F00
    hit = _names_hit("f16", lambda v: im.truncate_to(v, "f16"))
    assert hit["patterns"] == 0 and hit["mid_above"] >= 2 * 0x7BFF


def test_planted_double_rounding_is_caught():
    """f32 rows into a bf16 index through f16: the float32 successor of a bf16 tie is an f16 tie or rounds onto the
    bf16 tie, which then goes to the even side; and f16's range is lost.  f16 rows into a bf16 index through a
    10-bit intermediate: caught by the f16 patterns one step beside a bf16 tie."""
    with np.errstate(over="ignore"):
        hit = _names_hit("bf16", lambda v: im.round_to(im.round_to(v, "f16"), "bf16"))
    assert hit["mid_above"] > 1000 and hit["mid_below"] > 1000 and hit["specials"] > 0
    f16 = im.cross_catalogue("f16")
    normal = np.isfinite(f16) & (np.abs(f16) >= 2.0 ** -14)
    v = f16[normal]
    bad = im.mismatches(im.round_to(im.round_sig(v, 10), "bf16"), im.round_to(v, "bf16"))
    assert bad.size > 1000
    assert np.isin((v[bad].view(np.uint32) >> 13) & 7, (3, 5)).all()         # mantissa tails 011 and 101: beside the tie


def test_planted_normalisation_defects_are_caught_by_class_one():
    rows, N, e = im.exact_norm_rows(96, 100, "f32", seed=1)
    den = im.exact_den(N, e)
    for T in im.STORAGE:
        good = im.stored_exact_norm(rows, den, T)
        no_eps = im.stored_exact_norm(rows, np.ldexp(N.astype(np.float64), e).astype(F32), T)
        bad_rows = np.unique(im.mismatches(no_eps, good) // 100)
        assert set(bad_rows) <= set(np.flatnonzero(e < -20)) and bad_rows.size >= 0.9 * (e < -20).sum(), T
    # v * (1 / den) is not v / den: caught in f32 storage (a 16-bit rounding hides it on these rows)
    good, recip = im.stored_exact_norm(rows, den, "f32"), im.stored_exact_norm(rows, den, "f32", reciprocal=True)
    assert np.unique(im.mismatches(recip, good) // 100).size >= 10
    # a dropped epsilon on the degenerate rows: 0 / 0
    z, zden = im.degenerate_rows(40)
    with np.errstate(all="ignore"):
        assert np.isnan(im.stored_exact_norm(z[:1], np.zeros(1, F32), "f16")).all()
    assert (im.stored_exact_norm(z[:1], zden[:1], "f16") == 0).all()


@pytest.mark.parametrize("d", [8, 40, 99, 100])
def test_planted_layout_defects_are_caught_by_the_catalogue_rows(d):
    rows = im.pack_rows(im.catalogue_values("f16"), d)[:64]
    assert im.mismatches(im.layout_roundtrip(rows), rows).size == 0
    assert im.mismatches(im.layout_roundtrip(rows, "swap16"), rows).size > rows.size // 2
    if d > 8:
        assert im.mismatches(im.layout_roundtrip(rows, "k+8"), rows).size > rows.size // 4
    # the same two defects in a query image: the probe corpus reads element k of the query in row k
    c, k, scale = im.probe_corpus(d + 5, d)
    q = im.probe_queries(3, d, "f16", "f16")
    want = im.probe_scores(q, "f16", k, scale)
    for defect in ("swap16", "k+8") if d > 8 else ("swap16",):
        assert not np.array_equal(im.probe_scores(im.layout_roundtrip(q, defect), "f16", k, scale), want)


def test_planted_chunk_loop_defect_is_caught_by_the_second_chunk():
    for d in im.CHUNK_D:
        chunk = im.chunk_rows(d)
        n = chunk + 33
        assert np.array_equal(im.chunked_copy(n, chunk), np.arange(n))
        bad = im.chunked_copy(n, chunk, ignore_r0=True)
        assert np.array_equal(np.flatnonzero(bad != np.arange(n)), np.arange(chunk, n))     # the last 33 rows
