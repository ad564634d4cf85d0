"""The k-means training model of tests/ivf_train_model.py, checked on its own (no GPU): the generator against its
published vectors, the shuffle's invariants, the one-step model on hand-made lists, and the two conditions that keep the
GPU test (tests/test_ivf_train_gpu.py) from going vacuous: the crafted input really empties several lists at once,
and the bound really is far below the effect of one dropped member."""
import numpy as np
import pytest

import ivf_train_model as tm

F32 = np.float32


# ------------------------------------------------------------------ the sample
def test_splitmix64_published_vectors():
    state, out = 1234567, []
    for _ in range(3):
        state, z = tm.splitmix64(state)
        out.append(z)
    assert out == [6457827717110365317, 3203168211198807973, 9817491932198370423]
    assert 0 <= state < 1 << 64


def test_splitmix64_wraps_at_64_bits():
    state, z = tm.splitmix64((1 << 64) - 1)                 # the increment overflows
    assert state == 0x9E3779B97F4A7C15 - 1 and 0 <= z < 1 << 64
    assert tm.splitmix64(-1 & tm.MASK64) == (state, z)       # a negative seed is its two's complement


@pytest.mark.parametrize("n,nlist", [(4596, 16), (3000, 40), (33, 33), (170, 6), (257, 1), (5, 5)])
def test_shuffle_is_a_permutation_prefix(n, nlist):
    nt = tm.sample_size(n, nlist)
    assert nt == min(n, 256 * nlist)
    moduli = []
    ids = tm.sample_ids(n, nlist, tm.SEED, moduli)
    assert ids.dtype == np.int64 and ids.shape == (nt,)
    assert ids.min() >= 0 and ids.max() < n and len(set(ids.tolist())) == nt
    assert moduli == [n - i for i in range(nt)]              # one draw per position, never modulo zero
    if nt == n:
        assert moduli[-1] == 1                               # the last position can only stay
        assert sorted(ids.tolist()) == list(range(n))
    # a prefix: the sample of a smaller cap is the head of this one (position i depends on draws 0..i only)
    if nlist > 1 and 256 * (nlist - 1) < nt:
        assert np.array_equal(tm.sample_ids(n, nlist - 1, tm.SEED), ids[:256 * (nlist - 1)])
    assert np.array_equal(tm.sample_ids(n, nlist, tm.SEED), ids)


def test_shuffle_by_hand():
    # n = 4, all four positions, from the draws themselves
    state, draws = 9, []
    for _ in range(4):
        state, z = tm.splitmix64(state)
        draws.append(z)
    ids = [0, 1, 2, 3]
    for i in range(4):
        j = i + draws[i] % (4 - i)
        ids[i], ids[j] = ids[j], ids[i]
    assert tm.sample_ids(4, 1, 9).tolist() == ids


def test_the_other_seed_gives_another_sample():
    c = tm.CASE["sampled"]
    a, b = tm.sample_ids(c.n, c.nlist, tm.SEED), tm.sample_ids(c.n, c.nlist, tm.OTHER_SEED)
    assert len(a) == len(b) == 4096 and not np.array_equal(a, b)
    assert set(a.tolist()) != set(b.tolist()) and not np.array_equal(a[:c.nlist], b[:c.nlist])


def test_cases_are_the_ones_stated():
    got = [(c.name, c.n, c.d, c.nlist, c.dtype) for c in tm.CASES]
    assert got == [("sampled", 4596, 300, 16, "f16"), ("whole", 3000, 64, 40, "bf16"),
                   ("split-quantizer", 1500, 768, 8, "f32"), ("long-rows", 700, 1030, 5, "f16"),
                   ("n-equals-nlist", 33, 40, 33, "f16"), ("empties", 170, 128, 6, "f16")]
    assert [tm.sample_size(c.n, c.nlist) for c in tm.CASES] == [4096, 3000, 1500, 700, 33, 170]
    assert all(c.steps == tuple(range(25)) for c in tm.CASES[:2])
    assert all(c.steps == (0, 1, 2, 24) for c in tm.CASES[2:])
    for c in tm.CASES:
        x = tm.case_input(c)
        assert x.dtype == F32 and x.shape == (c.n, c.d)
        assert np.array_equal(x, tm.oracle.quantize(x, c.dtype))          # already rounded to the input dtype


# ------------------------------------------------------------------ one step, members known by construction
def test_step_two_lists_by_hand():
    X = np.array([[1, 0, 0, 0], [0, 0, 2, 0], [0, 1, 0, 0], [3, 0, 0, 4]], F32)
    C = np.array([[1, 0, 0, 0], [0, 0, 0, 1]], F32)
    got, pairs = tm.step(C, X, [0, 1, 0, 1])
    assert pairs == []
    want = np.array([[1, 1, 0, 0], [3, 0, 2, 4]], np.float64)
    want /= np.sqrt([[2.0], [29.0]])
    assert np.array_equal(got, want)
    assert np.array_equal(tm.initial(X, 2), np.array([[1, 0, 0, 0], [0, 0, 1, 0]], np.float64))


def test_sums_are_sequential_fp32_in_ascending_position():
    big = F32(2.0 ** 24)
    X = np.array([[big, 1], [7, 7], [1, 1], [1, big]], F32)             # list 0: rows 0, 2, 3 in that order
    S, cnt = tm.list_sums(np.zeros((2, 2), F32), X, [0, 1, 0, 0])
    # first column: 2^24 + 1 rounds back to 2^24 (ties to even) and so does the next + 1; the second column holds the
    # same three values in the opposite order and gives 2^24 + 2
    assert S.dtype == F32 and S[0].tolist() == [2.0 ** 24, 2.0 ** 24 + 2] and S[1].tolist() == [7, 7]
    assert cnt.tolist() == [3, 1]


def test_step_three_lists_one_empty_by_hand():
    X = np.array([[2, 4, 0, 0], [2, 4, 0, 0], [0, 0, 1, 0]], F32)
    C = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F32)
    S, cnt = tm.list_sums(C, X, [0, 0, 2])
    assert S.tolist() == [[4, 8, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]] and cnt.tolist() == [2, 0, 1]
    S2, pairs = tm.split_empty(S, cnt)
    assert pairs == [(1, 0)]
    up, down = 1 + 1 / 1024, 1 - 1 / 1024                                # exact in fp32, and so are the products
    assert S2.tolist() == [[4 * down, 8 * up, 0, 0], [4 * up, 8 * down, 0, 0], [0, 0, 1, 0]]
    got, pairs = tm.step(C, X, [0, 0, 2])
    assert pairs == [(1, 0)]
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-15) and got[1, 0] > got[0, 0] and got[1, 1] < got[0, 1]


def test_split_bookkeeping_by_hand():
    d = 4
    S = np.arange(1, 6 * d + 1, dtype=F32).reshape(6, d)
    # counts 100 / 0 / 60 / 0 / 0 / 10: list 1 halves list 0 (50 / 50), list 3 halves list 2 (60 > 50: 30 / 30),
    # list 4 takes the lowest of the two lists with 50, which is list 0 again (25 / 25)
    S2, pairs = tm.split_empty(S, [100, 0, 60, 0, 0, 10])
    assert pairs == [(1, 0), (3, 2), (4, 0)]
    up, down = F32(1) + tm.SPLIT_EPS, F32(1) - tm.SPLIT_EPS
    a, b = np.array([down, up, down, up], F32), np.array([up, down, up, down], F32)
    assert np.array_equal(S2[1], S[0] * b) and np.array_equal(S2[3], S[2] * b) and np.array_equal(S2[2], S[2] * a)
    assert np.array_equal(S2[4], (S[0] * a) * b) and np.array_equal(S2[0], (S[0] * a) * a)
    assert np.array_equal(S2[5], S[5])
    # without the bookkeeping every empty list would have split list 0
    assert len({big for _, big in pairs}) == 2


def test_a_zero_row_stays_zero_and_a_list_without_members_keeps_its_row():
    C = np.array([[0, 3, 4], [1, 0, 0]], F32)
    got, pairs = tm.step(C, np.array([[0, 0, 0]], F32), [1])
    assert pairs == [(0, 1)] and np.array_equal(got, np.zeros((2, 3)))   # split of a zero row: still zero, no NaN
    S, cnt = tm.list_sums(C, np.array([[0, 0, 2]], F32), [1])
    assert S.tolist() == [[0, 3, 4], [0, 0, 2]] and cnt.tolist() == [0, 1]


# ------------------------------------------------------------------ what keeps the GPU test from going vacuous
def test_the_crafted_input_empties_several_lists_that_split_different_big_lists():
    c = tm.CASE["empties"]
    x = tm.case_input(c)
    assert len(np.unique(x, axis=0)) == 3
    X = x[tm.sample_ids(c.n, c.nlist, tm.SEED)]
    C0 = tm.initial(X, c.nlist).astype(F32)
    assert len(np.unique(C0, axis=0)) < c.nlist                          # duplicate initial centroids
    asg = tm.assign64(C0, X)                                             # identical rows: exact ties, lowest list
    S, cnt = tm.list_sums(C0, X, asg)
    assert (cnt == 0).sum() >= 2
    C1, pairs = tm.step(C0, X, asg)
    assert len(pairs) == (cnt == 0).sum() and len({big for _, big in pairs}) >= 2
    # the split lists differ from what they were split from, and every row is a unit vector
    for e, big in pairs:
        assert not np.array_equal(C1[e], C1[big])
    assert np.allclose(np.linalg.norm(C1, axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("case", [c for c in tm.CASES if c.name != "empties"], ids=lambda c: c.name)
@pytest.mark.parametrize("drop", ["first", "last"])
def test_the_bound_is_far_below_one_dropped_member(case, drop):
    """In every list of the first iteration, leaving one member out moves some component by more than 64 bounds.
    (The members of the "empties" case are copies of one another, so there a dropped copy cancels in the
    normalisation: that case is about the split, and its lists are not part of this check.)"""
    x = tm.case_input(case)
    X = x[tm.sample_ids(case.n, case.nlist, tm.SEED)]
    C0 = tm.initial(X, case.nlist).astype(F32)
    asg = tm.assign64(C0, X)
    want, pairs = tm.step(C0, X, asg)
    bad, bad_pairs = tm.step(C0, X, asg, drop=drop)
    assert pairs == bad_pairs
    touched = np.setdiff1d(np.unique(asg), [i for p in pairs for i in p])
    assert len(touched) >= min(case.nlist, 5)
    ratio = tm.excess(bad.astype(F32), want, case.d).max(axis=1)
    assert ratio[touched].min() > 64, (case.name, drop, ratio[touched].min())
    assert tm.excess(want.astype(F32), want, case.d).max() <= 1          # fp32 rounding of the model itself passes


def test_bound_formula():
    w = np.array([1.0, -0.5, 0.0])
    assert np.array_equal(tm.bound(w, 64), 17 * 2.0 ** -24 * np.abs(w) + 2.0 ** -149)
    assert tm.bound(1.0, 256) == 17 * 2.0 ** -24 + 2.0 ** -149 and tm.bound(1.0, 257) == 18 * 2.0 ** -24 + 2.0 ** -149
    assert tm.bound(1.0, 768) == 19 * 2.0 ** -24 + 2.0 ** -149 and tm.bound(1.0, 1030) == 21 * 2.0 ** -24 + 2.0 ** -149
    assert tm.excess(F32([0.0]), [0.0], 8).max() == 0
