"""tests/select_cases.py without a GPU: the reference against the two older oracles, the branches of select_kernel and
merge_impl that the case tables reach (through the Python mirror select_plan), the proof that the tables can see the
"first 1024 boundary ties" defect, and the exact-input guard of every index-driven case."""
import functools

import numpy as np
import pytest

import exact_inputs as ex
import select_cases as sc
from oracle import oracle


# ------------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("R,k", [(3, 7), (8, 1000), (3, 8192)])
def test_reference_equals_the_merge_oracle_on_finite_inputs(R, k):
    for s, l in sc.MERGE_TABLE:
        if s not in sc.FINITE_SETS:
            continue
        scores, ids = sc.merge_batch(((s, l),), R, k)
        D, I = sc.canonical_merge(scores, ids, k)
        D0, I0 = oracle.merge_topk(scores, ids, k)
        I0 = np.where(I0 < 0, -1, I0)                    # the oracle hands a padding id back as it came: -2, INT64_MIN
        assert np.array_equal(I, I0), (s, l)
        assert np.array_equal(D, D0), (s, l)             # by value: -0 == +0


def test_reference_equals_expected_topk_on_planted_scores():
    n = 1061
    corpus, queries, units = sc.planted(n)
    for k in (1, 100, n, n + 3):
        D0, I0 = ex.expected_topk(corpus, queries, k)
        D, I = sc.planted_topk(units, k)
        assert np.array_equal(I, I0) and np.array_equal(D, D0), k
    allowed = sc.masked_sets()
    corpus, queries, units = sc.planted(sc.N_MASKED, sc.MASKED_NAMES)
    D0, I0 = ex.expected_topk(corpus, queries, sc.K_MASKED, allowed=allowed)
    D, I = sc.planted_topk(units, sc.K_MASKED, allowed=allowed)
    assert np.array_equal(I, I0) and np.array_equal(D, D0)


def test_reference_order_on_special_values():
    f = sc._f32
    s = np.concatenate([f([0x7FC00000, 0xFF800000, 0x80000000, 0x00000000, 0xFFABCDEF, 0x7F800000, 0x00000001, 0xFF7FFFFF]),
                        np.array([1.0, 1.0, 1.0], np.float32)])
    ids = np.array([3, 4, 9, 8, 1, 5, 6, 7, 20, 10, -5], np.int64)
    D, I = sc.canonical_topk(s, ids, 12)
    # +inf, 1.0 (id 10 before 20; id -5 is padding), denormal, the zeros by id (8 before 9), -FLT_MAX, -inf, NaNs by id
    assert I.tolist() == [5, 10, 20, 6, 8, 9, 7, 4, 1, 3, -1, -1]
    assert D.view(np.uint32)[4] == 0 and D.view(np.uint32)[5] == 0           # -0 comes back as +0
    assert np.isnan(D[8:10]).all() and (D[10:] == -sc.FLT_MAX).all()
    # equal ids: by position — visible in which of two different-looking zeros is kept at the boundary
    D, I = sc.canonical_topk(np.array([2.0, 2.0], np.float32), np.array([7, 7]), 1)
    assert I.tolist() == [7]


def test_same_result_is_strict():
    D = np.array([[1.0, np.nan, 0.0]], np.float32)
    I = np.array([[1, 2, 3]])
    assert sc.same_result((D, I), (D.copy(), I.copy()))
    assert not sc.same_result((np.array([[1.0, np.nan, -0.0]], np.float32), I), (D, I))       # bit pattern
    assert not sc.same_result((np.array([[1.0, 5.0, 0.0]], np.float32), I), (D, I))
    assert not sc.same_result((D, np.array([[1, 3, 2]])), (D, I))


# ------------------------------------------------------------------------------------------ generators do what they say
def test_score_sets_have_the_advertised_shape():
    rng = np.random.default_rng(0)
    n, k = 8000, 1000
    v = sc.SCORE_SETS["distinct"](n, k, rng)
    assert np.unique(v).size == n and (v > 0).any() and (v < 0).any()
    assert np.unique(np.frexp(v)[1]).size > 60
    for b in (1, 2, 3):
        key = sc.kernel_keys(sc.SEL_DENSE, sc.SCORE_SETS[f"shared_bytes({b})"](n, k, rng)) >> np.uint64(32)
        diff = int(np.bitwise_and.reduce(key)) ^ int(np.bitwise_or.reduce(key))
        assert (32 - diff.bit_length()) >> 3 == b
    for t in (2, 1023, 1024, 1025, 5000):
        v = np.sort(sc.SCORE_SETS[f"ties({t})"](n, k, rng))[::-1]
        cls = np.flatnonzero(v == v[k - 1])
        assert cls.size == t and cls[0] < k - 1 + (t == 2) and cls[-1] >= k       # straddles rank k
    assert (sc.SCORE_SETS["all_negative"](n, k, rng) < 0).all()
    v = sc.SCORE_SETS["specials"](n, k, rng)
    bits = set(v.view(np.uint32).tolist())
    assert {0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFABCDEF, 0x7F800000, 0xFF800000, 1, 0x80000001, 0x7F7FFFFF,
            0xFF7FFFFF, 0x80000000} <= bits
    for delta in (1, 0, -1):
        v = sc.s_two_level(delta)(n, k, rng)
        assert (v == 5.0).sum() == k + delta and np.unique(v).size == 2


def test_id_layouts():
    rng = np.random.default_rng(0)
    R, k = 8, 1000
    assert np.array_equal(np.sort(sc.i_interleaved(R, k, rng).ravel()), np.arange(R * k))
    assert (np.diff(sc.i_descending(R, k, rng).ravel()) == -1).all()
    h = sc.i_huge(R, k, rng)
    assert (h > 1 << 32).all() and h.max() == sc.I64_MAX - 1 and np.unique(h).size == h.size
    d = sc.i_duplicate(R, k, rng)
    assert np.array_equal(d[0], d[-1])
    neg = sc.i_negative(R, k, rng)
    assert {-1, -2, -7, sc.I64_MIN} <= set(neg[neg < 0].tolist())
    assert (sc.i_all_padding(R, k, rng) < 0).all()


# ---------------------------------------------------------------------------------------------------------- the plan
def _bucket(t):
    return 0 if t == 0 else "1..1023" if t < 1024 else t if t <= 1025 else ">1025"


def _facts(plan):
    m = plan["mode"]
    out = {(m, "phase1", plan["phase1"]), (m, "phase2", plan["phase2"]), (m, "sort", plan["sort"]), (m, "P", plan["P"])}
    if plan["phase1"] == "global":
        out.add((m, "global_early_exit", plan["global_early_exit"]))
    if plan["phase2"] == "taken":
        out |= {(m, "skip", plan["skip"]), (m, "ending", plan["ending"])}
        if m == sc.SEL_MERGE64:
            out.add((m, "tie_class", _bucket(plan["tie_class"])))
            if plan["skip_raw"] > 3:
                out.add((m, "skip", "clamped"))
            if plan["tie_class"] > sc.SEL_TIE_CAP:
                out.add((m, "every_tie_taken", plan["every_tie_taken"]))
    if plan["k_above_n"]:
        out.add((m, "k_above_n", True))
    return out


@functools.lru_cache(maxsize=1)
def _reached():
    facts, witness = set(), {}
    def note(fs, who):
        for f in fs:
            witness.setdefault(f, who)
        facts.update(fs)
    for R, k in sc.MERGE_SHAPES:
        for s, l in sc.MERGE_TABLE:
            scores, ids = sc.merge_query(s, l, R, k)
            mp = sc.merge_plan(scores, ids, k)
            who = f"merge R={R} k={k} {s}/{l}"
            note({("merge", "form", mp["form"]), ("merge", "depth", mp["depth"])}, who)
            if mp["form"] == "grouped":
                note({("merge", "last_group", mp["last_group"])}, who)
            if l == "all_padding":
                note({("merge", "padding_only", True)}, who)
            for p in mp["launches"]:
                note(_facts(p), who)
    for n in sc.PLANT_N:
        corpus, queries, units = sc.planted(n)
        S = sc.planted_scores(units)
        for q, name in enumerate(sc.PLANTED):
            keys = sc.kernel_keys(sc.SEL_DENSE, S[q])
            for k in sc.plant_ks(n):
                note(_facts(sc.select_plan(sc.SEL_DENSE, n, k, keys)), f"dense n={n} k={k} {name}")
    # masked dense: SEL_PAIRS32 over the whole corpus with -1 ids
    _, _, units = sc.planted(sc.N_MASKED, sc.MASKED_NAMES)
    S = sc.planted_scores(units)
    for q, allowed in enumerate(sc.masked_sets()):
        ids = np.where(allowed, np.arange(sc.N_MASKED), -1)
        note(_facts(sc.select_plan(sc.SEL_PAIRS32, sc.N_MASKED, sc.K_MASKED, sc.kernel_keys(sc.SEL_PAIRS32, S[q], ids))),
             f"masked {int(allowed.sum())} rows")
        if not allowed.any():
            note({(sc.SEL_PAIRS32, "padding_only", True)}, "masked 0 rows")
    n, k = sc.MASKED_DIRECT
    S = sc.planted_scores(sc.planted(n)[2])
    ids = np.where(sc.masked_direct_set(), np.arange(n), -1)
    for q, name in enumerate(sc.PLANTED):
        note(_facts(sc.select_plan(sc.SEL_PAIRS32, n, k, sc.kernel_keys(sc.SEL_PAIRS32, S[q], ids))), f"masked half of {n} {name}")
    return facts, witness


REQUIRED = (
    [("merge", "form", "once"), ("merge", "form", "grouped"), ("merge", "last_group", 1), ("merge", "depth", 2),
     ("merge", "padding_only", True)] +
    [(sc.SEL_MERGE64, "phase1", "direct"), (sc.SEL_MERGE64, "phase2", "taken"),
     (sc.SEL_MERGE64, "phase2", "skipped: count <= 2 pk"), (sc.SEL_MERGE64, "phase2", "skipped: pk > 2048")] +
    [(sc.SEL_MERGE64, "skip", s) for s in (0, 1, 2, 3, "clamped")] +
    [(sc.SEL_MERGE64, "ending", e) for e in ("whole bin", "score bits")] +
    [(sc.SEL_MERGE64, "tie_class", t) for t in (0, "1..1023", 1024, 1025, ">1025")] +
    [(sc.SEL_MERGE64, "every_tie_taken", v) for v in (False, True)] +
    [(sc.SEL_MERGE64, "sort", s) for s in ("register", "lds")] +
    [(sc.SEL_MERGE64, "P", p) for p in (2, 1024, 2048, 16384)] +
    [(sc.SEL_DENSE, "phase1", "direct"), (sc.SEL_DENSE, "phase1", "global"),
     (sc.SEL_DENSE, "global_early_exit", True), (sc.SEL_DENSE, "global_early_exit", False),
     (sc.SEL_DENSE, "phase2", "taken"), (sc.SEL_DENSE, "phase2", "skipped: count <= 2 pk"),
     (sc.SEL_DENSE, "phase2", "skipped: pk > 2048"), (sc.SEL_DENSE, "k_above_n", True)] +
    [(sc.SEL_DENSE, "skip", s) for s in (0, 1, 2, 3, 6, 7)] +
    [(sc.SEL_DENSE, "ending", e) for e in ("whole bin", "all 64 bits")] +
    [(sc.SEL_DENSE, "sort", s) for s in ("register", "lds")] +
    [(sc.SEL_DENSE, "P", p) for p in (2, 1024, 2048, 16384)] +
    [(sc.SEL_PAIRS32, "phase1", "global"), (sc.SEL_PAIRS32, "phase1", "direct"), (sc.SEL_PAIRS32, "phase2", "taken"),
     (sc.SEL_PAIRS32, "padding_only", True), (sc.SEL_PAIRS32, "phase2", "skipped: count <= 2 pk"),
     (sc.SEL_PAIRS32, "global_early_exit", True), (sc.SEL_PAIRS32, "global_early_exit", False)] +
    [(sc.SEL_PAIRS32, "skip", 0)] +                    # (a -1 id is a zero key: no common byte where a list is padded)
    [(sc.SEL_PAIRS32, "ending", e) for e in ("whole bin", "all 64 bits")] +
    [(sc.SEL_PAIRS32, "sort", "register")] +
    [(sc.SEL_PAIRS32, "P", p) for p in (2, 128, 1024)]
)


def test_case_tables_reach_every_branch_of_the_plan():
    facts, witness = _reached()
    missing = [f for f in REQUIRED if f not in facts]
    assert not missing, missing
    for f in REQUIRED:
        print(f, "<-", witness[f])


def test_unreached_branches_are_really_unreached():
    facts, _ = _reached()
    for (mode, what, value), reason in sc.UNREACHED.items():
        assert reason
        if value == "not planned":
            continue
        if value == "any":
            assert not any(f[0] == mode and f[1] == what for f in facts), (mode, what)
        else:
            assert (mode, what, value) not in facts, (mode, what, value)
    assert not any(f[1] == "ending" and f[2] == "all 64 bits" for f in facts if f[0] == sc.SEL_MERGE64)


def test_merge_shapes_and_the_unsupported_k():
    one = sc.merge_query("distinct", "contiguous", 2, 8192)
    assert sc.merge_plan(one[0], one[1], 8192)["launches"][0]["P"] == 16384
    s = np.zeros((2, sc.MERGE_K_UNSUPPORTED), np.float32)
    assert sc.merge_plan(s, np.zeros(s.shape, np.int64), sc.MERGE_K_UNSUPPORTED)["unsupported"]
    big = sc.merge_query("distinct", "contiguous", 5, 8192)
    mp = sc.merge_plan(big[0], big[1], 8192)
    assert (mp["form"], mp["groups"], mp["last_group"], mp["depth"]) == ("grouped", 3, 1, 2) and len(mp["launches"]) == 6


def test_plan_mirrors_the_launch_sizes():
    keys = sc.kernel_keys(sc.SEL_DENSE, np.zeros(20011, np.float32))
    assert sc.select_plan(sc.SEL_DENSE, 20011, 1000, keys)["lds_keys"] == 1024
    assert sc.select_plan(sc.SEL_DENSE, 20011, 16385, keys)["unsupported"]
    assert sc.select_plan(sc.SEL_DENSE, 16384, 5, keys[:16384])["lds_keys"] == 16384
    assert sc.select_plan(sc.SEL_DENSE, 1, 4, keys[:1])["lds_keys"] == 2
    assert sc.select_plan(sc.SEL_PAIRS32, 300, 10, keys[:300], n_cap=16384)["lds_keys"] == 16384


# ------------------------------------------------------------------------------------------------- the mutation proof
@pytest.mark.parametrize("R,k", [(8, 1000), (8, 2048), (17, 1000)])
def test_tables_see_a_tie_list_of_1024(R, k):
    """"Keep the first 1024 boundary ties by position" — the kindest outcome of the old tie list's race — differs from
    the reference wherever more than 1024 entries tie at rank k and small ids sit late: the interleaved layouts."""
    seen = []
    for s in sc.MANY_TIES:
        for l in ("interleaved", "descending", "huge"):
            scores, ids = sc.merge_query(s, l, R, k)
            per = sc.LDS_KEYS_CAP // k
            bad = False
            for g in range(0, R, per):                                   # the defect acts inside every group's launch
                a, b = scores[g: g + per].ravel(), ids[g: g + per].ravel()
                bad |= not sc.same_result(sc.first_k_ties_by_position(a, b, k), sc.canonical_topk(a, b, k))
            if bad:
                seen.append((s, l))
    assert ("all_equal", "interleaved") in seen and ("ties(5000)", "interleaved") in seen, seen
    if R == 8:                                           # (of 17 lists the first group of 16 holds under 1025 of them)
        assert ("ties(1025)", "interleaved") in seen or ("ties(1025)", "descending") in seen, seen
    # and not where at most 1024 entries tie
    for s in ("ties(1024)", "ties(1023)", "distinct"):
        scores, ids = sc.merge_query(s, "interleaved", 8, 1000)
        assert sc.same_result(sc.first_k_ties_by_position(scores.ravel(), ids.ravel(), 1000),
                              sc.canonical_topk(scores.ravel(), ids.ravel(), 1000))


def test_the_issue_example():
    """Eight lists of k = 1000 with one repeated score and ids j * R + r: the result is ids 0..999."""
    scores, ids = sc.merge_query("all_equal", "interleaved", 8, 1000)
    D, I = sc.canonical_topk(scores.ravel(), ids.ravel(), 1000)
    assert np.array_equal(I, np.arange(1000))
    p = sc.merge_plan(scores, ids, 1000)["launches"][0]
    assert p["tie_class"] == 8000 and p["want"] == 1000 and p["ending"] == "score bits"


# ---------------------------------------------------------------------------------------------- index-driven cases
@pytest.mark.parametrize("n", sc.PLANT_N + (ex.N_FILTER, sc.N_FILTER_2048))
def test_planted_cases_are_exactly_summable_and_fit_16_bits(n):
    corpus, queries, units = sc.planted(n)
    ex.assert_exactly_summable(corpus, queries, sc.UNIT)
    assert sc.fits_16bit(corpus) and sc.fits_16bit(queries)
    assert np.array_equal(ex.exact_scores(corpus, queries), units * sc.UNIT)
    S = sc.planted_scores(units)
    assert np.array_equal(S.astype(np.float64), units * sc.UNIT)           # every planted score is an fp32 number


def test_chunked_case():
    corpus, queries, units = sc.chunked()
    ex.assert_exactly_summable(corpus, queries, sc.UNIT)
    assert sc.fits_16bit(corpus)
    assert np.array_equal(ex.exact_scores(corpus, queries), units * sc.UNIT)
    D, I = sc.planted_topk(units[:1], sc.K_CHUNKED)
    assert (I[0, :5] >= sc.CHUNK_ROWS).sum() == 2 and I[0, 0] == sc.CHUNK_ROWS + 1     # top scores from both chunks
    tie = D[0] == D[0, sc.K_CHUNKED - 1]
    assert tie.sum() > 50 and (units[0] == units[0, I[0, -1]]).sum() > tie.sum()        # the class straddles rank 100 ...
    assert (units[0, sc.CHUNK_ROWS:] == units[0, I[0, -1]]).any() and I[0, tie].max() < sc.CHUNK_ROWS   # ... and the boundary
    # the dense select of the first chunk radix-selects in global memory; the merge of the two lists is SEL_PAIRS32
    S = sc.planted_scores(units)
    p = sc.select_plan(sc.SEL_DENSE, sc.CHUNK_ROWS, sc.K_CHUNKED, sc.kernel_keys(sc.SEL_DENSE, S[0, : sc.CHUNK_ROWS]))
    assert p["phase1"] == "global" and p["lds_keys"] == 128
    p = sc.select_plan(sc.SEL_DENSE, 40, sc.K_CHUNKED, sc.kernel_keys(sc.SEL_DENSE, S[0, sc.CHUNK_ROWS:], id_base=sc.CHUNK_ROWS))
    assert p["k_above_n"] and p["phase1"] == "direct"


def test_filter_cases_cover_both_threshold_kernels():
    ranks = {k: sc.sample_rank(ex.N_FILTER, k) for k in sc.FILTER_K if sc.filter_path_expected(ex.N_FILTER, k)}
    assert min(ranks.values()) <= 64 < max(ranks.values()), ranks
    assert [sc.filter_path_expected(ex.N_FILTER, k) for k in sc.FILTER_K] == [True, True, True, False]
    assert sc.filter_path_expected(sc.N_FILTER_2048, 2048) and sc.sample_rank(sc.N_FILTER_2048, 2048) > 64
