"""The exactly scored MaxSim inputs (tests/exact_maxsim_inputs.py), proved without a GPU: every case of the table
passes the guard, the C oracle returns the integer reference bit for bit, losing a planted row / the last k step / all
tiles but the first changes the reference, the maxima have real dynamic range, and the table reaches every kernel
instantiation and slice shape the dispatch can produce (through the mirrors of m16_shape and of the slicing)."""
import itertools

import numpy as np
import pytest

import exact_maxsim_inputs as em
from oracle import oracle

ALL_CASES = em.CASES + em.STALE + [em.beyond_case()]


_WORST = [0.0, 0]     # largest float32 numpy colbert deviation seen, cases seen


def _data(case):
    return em.generate(case)


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_every_case_is_exactly_scored_and_the_oracle_returns_the_integer_reference(case):
    d = _data(case)
    assert d.q.shape == (case.Lq, case.H) and d.q.dtype == np.float32
    assert len(d.docs) == case.n and all(x.dtype == np.float32 and x.shape[1] == case.H for x in d.docs)
    assert em.assert_exactly_scored(d.q, d.docs, d.plants) < 2.0 ** 24
    want = em.expected_maxsim(d.q, d.docs)
    assert want.dtype == np.float32
    assert np.array_equal(oracle.maxsim_scores(d.q, d.docs, "maxsim"), want)
    c64 = em.expected_colbert(d.q, d.docs)
    assert np.abs(oracle.maxsim_scores(d.q, d.docs, "colbert").astype(np.float64) - c64).max() <= 6e-8   # its float32 rounding
    c32 = em.expected_colbert(d.q, d.docs, np.float32)
    assert c32.dtype == np.float32
    dev = float(np.abs(c32.astype(np.float64) - c64).max())
    print(f"\n{case.name}: float32 numpy colbert deviates from float64 by {dev:.3e}")
    assert dev < em.COLBERT_ATOL
    _WORST[:] = [max(_WORST[0], dev), _WORST[1] + 1]
    assert (want[d.lens == 0] == 0.0).all() and (c64[d.lens == 0] == 0.0).all()
    for store in case.stores:                        # the values survive every store type the case is run in
        dt = em.store_dtype(store)
        if dt != "e4m3":
            assert np.array_equal(oracle.quantize(d.q, dt), d.q)
            assert all(np.array_equal(oracle.quantize(x, dt), x) for x in d.docs[:8])
        else:
            qt = store.split("_")[1]
            assert np.array_equal(oracle.quantize(d.q, qt), d.q)     # entries up to 4: three bits of e4m3's range


def test_largest_float32_colbert_deviation_over_the_table():
    """The figure DESIGN.md 4.4 quotes (1.1e-7): numpy float32 against float64 on the exact maxima, the largest over
    the cases the test above has walked."""
    print(f"\nlargest float32 numpy colbert deviation over {_WORST[1]} cases: {_WORST[0]:.3e}")
    assert _WORST[0] < em.COLBERT_ATOL


def test_the_guard_refuses_inputs_that_are_not_exactly_scored():
    case = em.CASES[1]
    d = _data(case)
    em.assert_exactly_scored(d.q, d.docs, d.plants)
    c = next(i for i, x in enumerate(d.docs) if x.shape[0] >= 40)
    bad = list(d.docs)
    bad[c] = d.docs[c].copy()
    bad[c][3] = 0.0
    bad[c][3, :2] = 1.0                                    # norm^2 = 2
    with pytest.raises(AssertionError):
        em.assert_exactly_scored(d.q, bad, d.plants)
    bad[c] = d.docs[c] * np.float32(0.5)                   # entries outside the set
    with pytest.raises(AssertionError):
        em.assert_exactly_scored(d.q, bad, d.plants)
    p, t = d.plants[c][0]
    other = next(r for r in range(d.docs[c].shape[0]) if r not in [pp for pp, _ in d.plants[c]])
    bad[c] = d.docs[c].copy()
    bad[c][other] = d.q[t]                                 # a second row reaches the planted maximum
    with pytest.raises(AssertionError):
        em.assert_exactly_scored(d.q, bad, d.plants)
    with pytest.raises(AssertionError):                    # a planted row that is no copy of its token
        em.assert_exactly_scored(d.q, d.docs, [[(other, t)] if i == c else [] for i in range(case.n)])
    q2 = np.repeat(d.q[t: t + 1], 2, axis=0)               # two equal query tokens: the plant serves both
    with pytest.raises(AssertionError):
        em.assert_exactly_scored(q2, [d.docs[c]], [[(p, 0)]])


# ----------------------------------------------------------------------------------------------------- discrimination
PLANTED = [c for c in em.CASES if c.cls in ("plant", "kedge")] + [em.beyond_case()]


@pytest.mark.parametrize("case", PLANTED, ids=[c.name for c in PLANTED])
def test_losing_any_planted_row_changes_that_candidates_score(case):
    d = _data(case)
    want = em.expected_maxsim(d.q, d.docs)
    seen = set()
    for c, mine in enumerate(d.plants):
        L = int(d.lens[c])
        assert (L == 0) == (not mine)
        if not mine:
            continue
        rows = {p for p, _ in mine}
        assert len(mine) == min(len(em.plant_positions(L)), min(8 if case.cls == "kedge" else 9,
                                                                 case.Lq - (case.Lq >= 2) - (case.Lq >= 12)))
        if len(mine) == len(em.plant_positions(L)):
            assert rows == set(em.plant_positions(L))
        if L > 32:
            assert max(rows) >= 32
        seen |= {("first", 0 in rows), ("last", L - 1 in rows), ("31", 31 in rows), ("32", 32 in rows),
                 ("tile end", any(p % 32 == 31 and p > 31 for p in rows))}
        v = em.integer_cosines(d.q, d.docs[c])
        assert em.maxsim_from_maxima(v.max(axis=1)[None])[0] == want[c]
        for p, t in mine:
            assert v[t, p] == 1 << em.SCALE_BITS
            rest = np.delete(v, p, axis=1)
            lost = em.maxsim_from_maxima(rest.max(axis=1)[None])[0] if L > 1 else np.float32(0.0)
            assert lost != want[c], (c, p, t)
    if case.lens_kind != "one":
        assert {("first", True), ("last", True), ("31", True), ("32", True), ("tile end", True)} <= seen
    # the helper the GPU-side reasoning refers to does the same thing
    c = next(i for i, mine in enumerate(d.plants) if mine)
    p = d.plants[c][0][0]
    got = em.expected_maxsim(d.q, em.drop_row(d.docs, c, p))
    assert got[c] != want[c] and np.array_equal(np.delete(got, c), np.delete(want, c))


def _last_step_holds_the_last_8_columns(case, store):
    return case.H - 8 >= em.last_k_step(case.H, store) * (32 // em.elem_bytes(store))


KEDGE = [(c, s) for c, s in em.CASE_STORES if c.cls == "kedge" and _last_step_holds_the_last_8_columns(c, s)]


@pytest.mark.parametrize("case,store", KEDGE, ids=[f"{c.name}-{s}" for c, s in KEDGE])
def test_zeroing_the_last_k_step_changes_every_kedge_candidate(case, store):
    d = _data(case)
    want = em.expected_maxsim(d.q, d.docs)
    g = em.last_k_step(case.H, store)
    # (all kedge cases but the 200-byte rows of H = 100, which the general kernel takes: its last k step is 4 wide)
    assert {c.H for c in em.CASES if c.cls == "kedge"} - {c.H for c, _ in KEDGE} == {100}
    for _, toks in zip(d.docs, d.plants):
        for _, t in toks:
            assert np.flatnonzero(d.q[t]).min() >= case.H - 8
    # (the rows that remain are no longer exactly scored: the float64 oracle scores them)
    lost = oracle.maxsim_scores(d.q, [em.zero_k_step(d.docs, c, g, store)[c] for c in range(case.n)])
    live = d.lens > 0
    assert (lost[live] != want[live]).all()
    assert np.array_equal(lost[~live], want[~live])


@pytest.mark.parametrize("case", PLANTED, ids=[c.name for c in PLANTED])
def test_first_tile_only_changes_every_candidate_of_several_tiles(case):
    d = _data(case)
    want = em.expected_maxsim(d.q, d.docs)
    lost = em.expected_maxsim(d.q, em.first_tile_only(d.docs))
    several = d.lens > 32
    assert (lost[several] != want[several]).all()
    assert np.array_equal(lost[~several], want[~several])
    if case.n >= em.N_CAND and case.lens_kind == "default":
        assert several.sum() >= 20


# ------------------------------------------------------------------------------------------------------ dynamic range
@pytest.mark.parametrize("case", em.CASES, ids=em.CASE_IDS)
def test_maxima_have_dynamic_range(case):
    d = _data(case)
    m = em.integer_maxima(d.q, d.docs)[d.lens > 0]
    one = 1 << em.SCALE_BITS
    if case.cls == "neg":
        assert m.max() == 0 and (m.max(axis=1) == 0).any()           # an all-zero row above negatives
        strictly = m.max(axis=1) < 0
        assert strictly.sum() >= m.shape[0] // 2                      # no zero row: every maximum below zero
        assert (m[strictly] < 0).all() and np.unique(m).size > 8
        return
    assert (m.max(axis=1) == one).all()
    if case.Lq > 1:
        assert (m.min(axis=1) <= 0).all()                             # every candidate spans [<= 0, 1]
        diff = np.abs(em.expected_colbert(d.q, d.docs) - em.expected_maxsim(d.q, d.docs).astype(np.float64))
        assert (diff > 1e-3).sum() >= case.n / 2
    if case.Lq >= 32:
        assert np.unique(m).size > 8


def test_some_planted_case_has_negative_maxima_too():
    """The token that is negative where the documents are not: at small H every row of a candidate is hot there."""
    assert any((em.integer_maxima(*_data(c)[:2]) < 0).any() for c in em.CASES if c.cls == "plant" and c.H <= 64)


# ------------------------------------------------------------------------------------------------------ path coverage
def test_the_mirror_of_m16_shape_at_the_shapes_the_issue_names():
    s = em.m16_shape
    assert s(64, "bf16", 5) == em.Shape(128, 16, 16, 1, 1, 32, False)          # 4 real k steps, 12 padded
    assert s(104, "f16", 40) == em.Shape(208, 16, 16, 2, 1, 64, False) and 208 % 32 == 16
    assert s(256, "f16", 65) == em.Shape(512, 16, 16, 2, 2, 128, True)
    assert s(2048, "bf16", 33) == em.Shape(4096, 16, 128, 1, 2, 64, True)
    assert s(4096, "bf16", 5) is None and s(100, "f16", 5) is None and s(50, "f32", 5) is None
    assert s(32, "f32", 40) == em.Shape(128, 16, 16, 2, 1, 64, False)
    assert s(128, "f32", 40) == em.Shape(512, 16, 16, 2, 1, 64, True)
    assert s(768, "f32", 33) == em.Shape(3072, 16, 96, 1, 2, 64, True)
    assert s(2048, "f32", 5) is None
    assert s(256, "e4m3_f16", 40) == em.Shape(256, 16, 16, 2, 1, 64, False)
    assert s(512, "e4m3_bf16", 40) == em.Shape(512, 16, 16, 2, 1, 64, True)
    assert s(768, "e4m3_bf16", 33) == em.Shape(768, 24, 24, 2, 1, 64, True)
    assert s(2048, "e4m3_f16", 33) == em.Shape(2048, 16, 64, 1, 2, 64, True)
    assert s(104, "e4m3_f16", 5) is None
    assert em.kernel_path(4096, "f16", 5, "single") == ("fallback", "f16", "vec")
    assert em.kernel_path(100, "f16", 5, "single") == ("fallback", "f16", "scalar")
    assert em.kernel_path(50, "f32", 5, "single") == ("fallback", "f32", "scalar")


def _paths():
    """Every (path, passes) the GPU file reaches: the single form with the case's Lq, the batch form with the longest
    query of its plan."""
    out = set()
    for case, store in em.CASE_STORES:
        for form, lq in (("single", case.Lq), ("batch", max(b - a for (a, b), _ in em.batch_plan(case)))):
            path = em.kernel_path(case.H, store, lq, form)
            assert path is not None, (case.name, store)               # no e4m3 case the kernel refuses
            sh = em.m16_shape(case.H, store, lq)
            out.add((path, min(sh.passes, 2) if sh else 0))
    return out


def test_the_table_reaches_every_instantiation_the_dispatch_can_select():
    paths = {p for p, _ in _paths()}
    for store, nqt, full, form in itertools.product(em.STORES, (1, 2), (True, False), ("single", "batch")):
        assert ("m16", store, nqt, full, 16, form) in paths, (store, nqt, full, form)
    for store, nqt, form in itertools.product(em.E4M3, (1, 2), ("single", "batch")):
        assert ("m16", store, nqt, True, 24, form) in paths, (store, nqt, form)
    assert not any(p[0] == "m16" and p[4] == 24 and not p[3] for p in paths)      # m16_go_t: RING != M16_RING is FULL
    assert not any(p[0] == "m16" and p[4] == 24 and not p[1].startswith("e4m3") for p in paths)
    assert {("fallback", "f16", "vec"), ("fallback", "bf16", "vec"), ("fallback", "f32", "vec"),
            ("fallback", "f16", "scalar"), ("fallback", "bf16", "scalar"), ("fallback", "f32", "scalar")} <= paths
    # passes = 1 and >= 2 with each nqt, in every store type
    got = {(p[1], p[2], n) for p, n in _paths() if p[0] == "m16"}
    for store, nqt, n in itertools.product(em.STORES, (1, 2), (1, 2)):
        assert (store, nqt, n) in got, (store, nqt, n)
    assert any(em.m16_shape(c.H, s, c.Lq) and em.m16_shape(c.H, s, c.Lq).passes == 3 for c, s in em.CASE_STORES)
    assert {c.Lq for c in em.CASES} >= {1, 5, 32, 33, 64, 65, 150}
    for case in em.CASES:
        if case.lens_kind == "default":
            assert {0, 1, 31, 32, 33, 64, 65, 192} <= set(em.case_lens(case).tolist())


def test_the_table_reaches_every_slice_shape():
    single, batch = {}, {}
    for case in em.CASES:
        lens = em.case_lens(case)
        passes = {em.m16_shape(case.H, s, case.Lq).passes for s in case.stores if em.m16_shape(case.H, s, case.Lq)}
        for p in passes:
            for k, v in em.slice_facts([lens.tolist()], "single", p).items():
                single[k] = single.get(k, False) or v
        plan = em.batch_plan(case)
        lq = max(b - a for (a, b), _ in plan)
        for s in case.stores:
            sh = em.m16_shape(case.H, s, lq)
            if sh:
                for k, v in em.slice_facts([lens[pick].tolist() for _, pick in plan], "batch", sh.passes).items():
                    batch[k] = batch.get(k, False) or v
    for k in ("starts_inside", "register_path", "three_waves", "steps_over_empty", "eq_taken", "eq_not_taken"):
        assert single[k], k
    for k in ("starts_inside", "register_path", "three_waves", "steps_over_empty"):
        assert batch[k], k
    # the 1000-candidate cases take the equal slices (T >= 768 tiles on 1024 waves), the 150-candidate ones do not
    for case in em.CASES:
        f = em.slice_facts([em.case_lens(case).tolist()], "single", 1)
        assert f["eq_taken"] == (case.n == em.N_MANY), case.name
    # the batch form walks about ten tiles per wave
    case = em.CASES[3]
    for lens, grid, eq in em.launches([em.case_lens(case)[pick].tolist() for _, pick in em.batch_plan(case)], "batch"):
        sl, taken = em.wave_slices(lens, grid, eq)
        assert not taken and grid <= 4 and max(hi - lo for lo, hi in sl) >= 3


def test_the_slice_mirror_on_small_examples():
    sl, taken = em.wave_slices([64, 0, 96], 1, False)           # tiles 2, 0, 3 on 4 waves
    assert sl == [(0, 1), (1, 2), (2, 3), (3, 5)] and not taken
    f = em.slice_facts([[64, 0, 96], [3]], "batch", 1)          # two queries: one workgroup each, no equal slices
    assert f["starts_inside"] and not f["three_waves"] and not f["register_path"]
    assert not f["eq_taken"] and not f["eq_not_taken"] and not f["steps_over_empty"]
    f = em.slice_facts([[32] * 3 + [0] + [64] * 3, [5]], "batch", 1)     # grid 1: 9 tiles on 4 waves
    assert f["steps_over_empty"] and f["register_path"]
    assert em.slice_facts([[192]], "single", 1)["three_waves"]
    assert not em.slice_facts([[192]], "single", 2)["register_path"]
    assert [len(l) for l, _, _ in em.launches([[1] * 4100], "single")] == [4096, 4]
    assert [len(l) for l, _, _ in em.launches([[1] * 4100], "batch")] == [4096, 4]        # per-query fallback
    sl, taken = em.wave_slices([32] * 1800, 256, True)          # t = 2, 900 waves of 1024
    assert taken and len(sl) == 900 and sl[-1] == (1798, 1800)
    sl, taken = em.wave_slices([32] * 1200, 256, True)          # t = 2, 600 waves: below three quarters
    assert not taken


def test_the_stale_scratch_pairs():
    for case in em.STALE:
        a = _data(case)
        assert em.m16_shape(case.H, case.stores[0], case.Lq).passes >= 2          # every candidate through the scratch
        assert all(em.m16_shape(case.H, s, case.Lq).passes >= 2 for s in case.stores)
        assert (em.integer_maxima(a.q, a.docs) == 1 << em.SCALE_BITS).all()
        assert (em.expected_maxsim(a.q, a.docs) == 1.0).all()
        b = em.generate(case, "neg", tuple(a.lens.tolist()))
        em.assert_exactly_scored(b.q, b.docs)
        assert (em.integer_maxima(b.q, b.docs) <= 0).all() and (em.expected_maxsim(b.q, b.docs) < 0).any()
        n2, lq2 = em.STALE_B2
        assert em.m16_shape(case.H, case.stores[0], lq2).lq_pad != em.m16_shape(case.H, case.stores[0], case.Lq).lq_pad
        b2 = em.generate(case._replace(Lq=lq2, n=n2), "neg", tuple(a.lens[:n2].tolist()))
        em.assert_exactly_scored(b2.q, b2.docs)
        assert b2.q.shape[0] == lq2 and len(b2.docs) == n2
