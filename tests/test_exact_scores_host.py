"""The exact-input generators, their guard and the numpy model of the bf16x3 split (tests/exact_inputs.py): what
tests/test_exact_scores_gpu.py relies on, proved without a GPU."""
import numpy as np
import pytest

import exact_inputs as ex
from oracle import oracle


@pytest.mark.parametrize("cls,n,d,B", ex.gpu_shapes())
def test_every_gpu_shape_is_exactly_summable(cls, n, d, B):
    corpus, queries, unit = ex.case(cls, n, d, B)
    assert corpus.shape == (n, d) and queries.shape == (B, d)
    assert corpus.dtype == np.float32 and queries.dtype == np.float32
    assert ex.assert_exactly_summable(corpus, queries, unit) < 24.0
    s = ex.exact_scores(corpus, queries)
    if cls == "neg":
        assert s.max() <= 0.0 and s.min() < 0.0
    if cls in ("A", "C"):                        # the edge queries: hot only at k = 0 / only at k = d - 1
        assert np.flatnonzero(queries[0]).tolist() == [0] and np.flatnonzero(queries[1]).tolist() == [d - 1]
        assert (np.count_nonzero(queries, axis=1) <= 4).all() and (np.count_nonzero(queries, axis=1) >= 1).all()
        for row in queries:                      # non-zeros in different 16-wide k steps
            steps = np.flatnonzero(row) // 16
            assert len(set(steps.tolist())) == steps.size
    if cls == "B":
        assert np.flatnonzero(corpus[0]).tolist() == [0] and np.flatnonzero(corpus[1]).tolist() == [d - 1]
        assert (np.count_nonzero(corpus, axis=1) <= 4).all() and (np.count_nonzero(corpus, axis=1) >= 1).all()


def test_the_guard_refuses_inputs_that_are_not_exactly_summable():
    c, q, unit = ex.gen_ints(50, 64, 3)
    ex.assert_exactly_summable(c, q, unit)
    with pytest.raises(AssertionError):          # sums beyond 2^24 units
        ex.assert_exactly_summable(c * 4096.0, q, unit)
    with pytest.raises(AssertionError):          # a score between two multiples of the unit
        ex.assert_exactly_summable(c + np.float32(0.25), q, unit)
    c2 = np.zeros((2, 16), np.float32)
    q2 = np.zeros((1, 16), np.float32)
    c2[:, 0], c2[:, 1], q2[0, 0], q2[0, 1] = 0.5, 0.5, 1.0, 1.0
    with pytest.raises(AssertionError):          # every score is a multiple of 1, the products are not
        ex.assert_exactly_summable(c2, q2, 1.0)


def test_expected_topk_order_padding_and_masks():
    corpus = np.array([[1.0], [3.0], [3.0], [-2.0], [3.0]], np.float32)
    queries = np.array([[1.0], [-1.0]], np.float32)
    D, I = ex.expected_topk(corpus, queries, 7)
    assert I.tolist() == [[1, 2, 4, 0, 3, -1, -1], [3, 0, 1, 2, 4, -1, -1]]      # ties by ascending id
    assert D[0].tolist() == [3.0, 3.0, 3.0, 1.0, -2.0, -ex.FLT_MAX, -ex.FLT_MAX]
    live = np.array([True, False, True, True, True])
    only = np.array([False, True, True, False, True])
    D, I = ex.expected_topk(corpus, queries, 3, live=live, allowed=[only, None])
    assert I.tolist() == [[2, 4, -1], [3, 0, 2]] and D[0, 2] == -ex.FLT_MAX
    # and it agrees with the C oracle (float64 accumulation, the same canonical order) on an exact case
    c, q, _ = ex.case("ints", ex.N_DENSE, 40, 65)
    D, I = ex.expected_topk(c, q, ex.N_DENSE + 3)
    D0, I0 = oracle.ip_topk(c, q, ex.N_DENSE + 3)
    assert np.array_equal(I, I0) and np.array_equal(D, D0)


def test_split3_is_exact_and_truncates():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(100_000) * 10.0 ** rng.integers(-6, 6, 100_000)).astype(np.float32)
    t = ex.split3(x)
    assert np.array_equal(t["h"] + t["m"] + t["l"], x.astype(np.float64))
    for part in t.values():                      # each term fits bf16 and carries the sign of x (truncation)
        assert np.array_equal(oracle.quantize(part.astype(np.float32), "bf16"), part.astype(np.float32))
        assert (part * x >= 0).all()
    assert (np.abs(t["h"]) <= np.abs(x)).all()


LIVE = {"A": {"hh", "mh", "lh"}, "B": {"hh", "hm", "hl"}, "C": {"hh", "hm", "mh", "mm"}}


@pytest.mark.parametrize("cls", ["A", "B", "C"])
@pytest.mark.parametrize("d", ex.SPLIT_D)
def test_split_model_reproduces_the_exact_product(cls, d):
    corpus, queries, _ = ex.case(cls, ex.N_SPLIT, d, ex.B_SPLIT)
    ref = ex.exact_scores(corpus, queries)
    assert np.array_equal(ex.split_model(corpus, queries), ref)
    for t in ex.DROPPED_TERMS:                   # what the kernel drops is identically zero here
        assert not ex.split_model(corpus, queries, keep=[t]).any()
    live = {t for t in ex.KEPT_TERMS if ex.split_model(corpus, queries, keep=[t]).any()}
    assert live == LIVE[cls]
    for b in range(queries.shape[0]):            # scores within a query are essentially all distinct
        assert np.unique(ref[b]).size >= (0.9 if cls != "B" else 0.2) * ref.shape[1]


@pytest.mark.parametrize("term,cls", [("hh", "A"), ("mh", "A"), ("lh", "A"), ("hm", "B"), ("hl", "B"), ("mm", "C")])
@pytest.mark.parametrize("d", ex.SPLIT_D)
def test_losing_one_kept_term_changes_a_score(term, cls, d):
    """For each of the six partial products the kernel keeps there is a class whose exact result a kernel without that
    product cannot return: the bit-for-bit GPU comparison fails on a single lost term."""
    corpus, queries, _ = ex.case(cls, ex.N_SPLIT, d, ex.B_SPLIT)
    ref = ex.exact_scores(corpus, queries)
    lost = ex.split_model(corpus, queries, keep=[t for t in ex.KEPT_TERMS if t != term])
    wrong = lost.astype(np.float32) != ref.astype(np.float32)
    assert wrong.any()
    assert wrong.any(axis=1).sum() >= queries.shape[0] // 2      # not one lucky query: most of them


def test_all_six_kept_terms_are_covered():
    assert set().union(*LIVE.values()) == set(ex.KEPT_TERMS)


@pytest.mark.parametrize("cls", list(ex.GENERATORS))
def test_values_survive_the_storage_rounding(cls):
    corpus, queries, _ = ex.case(cls, ex.N_SPLIT, 520, ex.B_SPLIT)
    for x in (corpus, queries):
        assert np.array_equal(oracle.quantize(x, "f32"), x)
        if cls in ("ints", "neg"):
            assert np.array_equal(oracle.quantize(x, "f16"), x)
            assert np.array_equal(oracle.quantize(x, "bf16"), x)
    if cls == "A":                               # the 16-bit query types of 3b
        assert np.array_equal(oracle.quantize(queries, "f16"), queries)
        assert np.array_equal(oracle.quantize(queries, "bf16"), queries)
    if cls == "C":
        assert np.array_equal(oracle.quantize(queries, "f16"), queries)
        assert not np.array_equal(oracle.quantize(queries, "bf16"), queries)


def test_single_term_loss_on_unit_rows_fixes_the_accuracy_threshold():
    """On the unit-norm data of the other stage-1 tests a correct split (exact accumulation) is within 1e-8 rms of
    float64 and every single lost term costs more than 3e-7 rms: the threshold of the GPU accuracy test, a third of the
    smallest such loss, comes from this model and not from the kernel."""
    corpus, queries = ex.accuracy_case()
    losses = ex.single_loss_rms(corpus, queries)
    print({t: f"{v:.3g}" for t, v in losses.items()})
    assert losses["none"] < 1e-8
    for t in ex.KEPT_TERMS:
        assert losses[t] > 3e-7, (t, losses[t])
    thr = ex.split_rms_threshold(losses)
    assert 1e-7 < thr < 2e-7
    assert thr > 10 * losses["none"]
    full = ex.split_model(corpus, queries) - ex.exact_scores(corpus, queries)
    assert np.abs(full).max() < 2e-7             # the "< 2e-7 for unit rows" of DESIGN.md 4.1b, for the dropped terms
