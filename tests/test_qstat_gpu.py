"""Query-stationary coalesced passes (scan_qstat_kernel): forced on at small corpora, they give exactly what one scan
per batch (coalesce = False) and the synchronous search give, bit for bit, at every group count of a pass, with walks
shorter and longer than the LDS ring; layouts without the kernel and indexes with removed rows keep their passes."""
import numpy as np
import pytest

import exact_inputs as ex
from helpers import make_corpus
from qstat_helpers import (N_LONG, N_SHORT, batches_of as _batches, index_of as _index, run as _run, same as _same,
                           scan_launches as _scan_launches, sync_search as _sync, tq as _tq)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [768, 700, 640])
@pytest.mark.parametrize("n", [N_SHORT, N_LONG])
def test_stationary_passes_equal_one_scan_per_batch(torch_mod, n, d, dtype):
    torch = torch_mod
    idx = _index(torch, d, dtype, n=n)

    def held(batches, launches):
        """Held passes against one scan per batch and against the synchronous search; the filter scans they took."""
        sync = _sync(idx, batches)
        want, _ = _run(torch, idx, batches, False)
        got, n_scan = _scan_launches(torch, idx, batches)
        _same(torch, got, want)
        _same(torch, got, sync)
        assert n_scan == launches

    pool = _batches(torch, d, dtype, (64,) * 9, 100, 100)
    # 1..9 batches of 64: passes of 8 groups, partial ones of 2, 4 and 6 at finish(); with 9 two passes of 8 and one of
    # 2, the fifth batch .. the eighth in the second
    for nb, launches in ((1, 1), (2, 1), (3, 1), (4, 1), (5, 2), (9, 3)):
        held(pool[:nb], launches)
    # eight one-group batches, mixed k, fill ONE pass: every held-batch entry and every workspace set of the handle is
    # in use when the eighth is submitted.  Then a batch of 33 (a full group and a group of one query): a pass of 2.
    sizes8, ks8 = (32, 1, 8, 17, 5, 31, 2, 32), (1, 7, 100, 257, 1000, 7, 100, 1)
    eight = _batches(torch, d, dtype, sizes8 + (33,), ks8 + (257,), 200)
    held(eight[:8], 1)
    held(eight, 2)
    # seven one-group batches and the 33 as the eighth batch of the pass: its first group fills the pass of 8, its second
    # waits, with the batch, for the next one, which the batch of 64 joins (3 groups)
    split = _batches(torch, d, dtype, sizes8[:7] + (33, 64), ks8[:7] + (1000, 100), 220)
    held(split, 2)
    # single-group batches with the 33 in the middle: nine groups, so the last batch of 64 straddles a pass of 8 and a
    # partial one
    held(_batches(torch, d, dtype, (32, 1, 8, 33, 17, 5, 64), (1, 7, 100, 257, 1000, 7, 100), 240), 2)
    # seven groups: one wave of the workgroup owns no group
    held(_batches(torch, d, dtype, (32, 32, 20, 32, 1, 32, 31), 100, 300), 1)
    idx.close()


def test_pass_counts(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    idx = _index(torch, d, dtype)
    b16 = _batches(torch, d, dtype, (64,) * 8, 100, 400)
    want, n0 = _scan_launches(torch, idx, b16, False)
    got, n1 = _scan_launches(torch, idx, b16)
    assert (n0, n1) == (8, 2)   # 16 groups: two stationary passes
    _same(torch, got, want)
    b7 = _batches(torch, d, dtype, (32,) * 7, 100, 420)
    _, n7 = _scan_launches(torch, idx, b7)
    assert n7 == 1
    # forced off: today's widths (3 resident, 6 wide; "auto" keeps the resident ones at 154 MB)
    idx.stationary_passes = False
    for wide, launches in ((False, 6), (True, 3), ("auto", 6)):
        idx.wide_passes = wide
        got, n2 = _scan_launches(torch, idx, b16)
        assert n2 == launches, wide
        _same(torch, got, want)
    # "auto" at 154 MB: the policy picks no wide pass, so no stationary one either
    idx.stationary_passes, idx.wide_passes = "auto", "auto"
    _, n3 = _scan_launches(torch, idx, b16)
    assert n3 == 6
    # a forced wide-pass flag keeps its widths under "auto"
    idx.wide_passes = True
    _, n4 = _scan_launches(torch, idx, b16)
    assert n4 == 3
    idx.close()


def test_auto_policy_above_the_infinity_cache(torch_mod):
    """180 k x 768 (276 MB): where "auto" picked wide passes of 6 it now picks stationary passes of 8; a partial pass
    of 6 groups is a wide one, one of 7 a stationary one; a forced wide-pass flag keeps its widths."""
    torch = torch_mod
    d, dtype, n = 768, "f16", 180_000
    idx = _index(torch, d, dtype, n=n, stat="auto")
    assert idx.stationary_passes == "auto" and idx.wide_passes == "auto"
    b16 = _batches(torch, d, dtype, (64,) * 8, 100, 900)
    want, n0 = _scan_launches(torch, idx, b16, False)
    got, n1 = _scan_launches(torch, idx, b16)
    assert (n0, n1) == (8, 2)
    _same(torch, got, want)
    for groups in (6, 7):
        part = _batches(torch, d, dtype, (32,) * groups, 100, 920)
        want_p, _ = _scan_launches(torch, idx, part, False)
        got_p, n2 = _scan_launches(torch, idx, part)
        assert n2 == 1
        _same(torch, got_p, want_p)
    idx.stationary_passes = False
    got, n3 = _scan_launches(torch, idx, b16)
    assert n3 == 3   # wide passes of 6, as before
    _same(torch, got, want)
    idx.stationary_passes = "auto"
    for wide, launches in ((True, 3), (False, 6)):
        idx.wide_passes = wide
        got, n4 = _scan_launches(torch, idx, b16)
        assert n4 == launches, wide
        _same(torch, got, want)
    idx.close()


@pytest.mark.parametrize("d", [1024, 384])
def test_layouts_without_the_kernel_keep_their_passes(torch_mod, d):
    torch = torch_mod
    dtype = "f16"
    idx = _index(torch, d, dtype, stat=False)
    batches = _batches(torch, d, dtype, (64,) * 4, 100, 500)
    for wide in (True, False):
        idx.wide_passes = wide
        idx.stationary_passes = False
        want, n0 = _scan_launches(torch, idx, batches)
        idx.stationary_passes = True
        got, n1 = _scan_launches(torch, idx, batches)
        assert n0 == n1
        _same(torch, got, want)
    idx.close()


def test_failed_batch_inside_a_stationary_pass_is_redone_alone(torch_mod):
    """The half-identical-rows corpus of test_coalesce_wide_gpu.py: the tie batch shares a pass of 8 with four others."""
    torch = torch_mod
    d, dtype, n = 768, "f16", 100_000
    row = make_corpus(1, d, seed=500, dtype=dtype)
    corpus = np.concatenate([make_corpus(n // 2, d, seed=501, dtype=dtype), np.repeat(row, n // 2, axis=0)])
    idx = _index(torch, d, dtype, corpus=corpus)
    ties = _tq(torch, np.repeat(row, 8, axis=0), dtype)
    qa = make_corpus(64, d, seed=502, dtype=dtype)
    qa *= -np.sign(qa.astype(np.float64) @ row[0].astype(np.float64))[:, None].astype(qa.dtype)
    qa = _tq(torch, qa, dtype)
    qs = (qa, ties, qa, qa, qa[:32])   # 2 + 1 + 2 + 2 + 1 groups
    want = [idx.search(q, 30) for q in qs]
    idx.coalesce = True
    outs = [idx.search(q, 30, async_=True) for q in qs]
    last = int(idx._lib.ts_index_last_ticket(idx._h))
    tickets = [last - len(qs) + 1 + i for i in range(len(qs))]
    redone = idx.finish()
    assert redone == [tickets[1]]
    _same(torch, outs, want)
    idx.close()


def test_add_sync_search_and_policy_changes_between_held_batches(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    idx = _index(torch, d, dtype)
    q0 = _tq(torch, make_corpus(64, d, seed=600, dtype=dtype), dtype)
    q1 = _tq(torch, make_corpus(40, d, seed=601, dtype=dtype), dtype)
    before, before_1 = idx.search(q0, 100), idx.search(q1, 50)
    extra = _tq(torch, make_corpus(30_000, d, seed=602, dtype=dtype), dtype)
    idx.coalesce = True
    a = idx.search(q0, 100, async_=True)
    b = idx.search(q1, 50, async_=True)
    idx.add(extra)   # held batches search the rows they were submitted against
    after, after_1 = idx.search(q0, 100), idx.search(q1, 50)
    c = idx.search(q0, 100, async_=True)
    s = idx.search(q1, 50)   # a synchronous search between held batches
    e = idx.search(q1, 50, async_=True)
    f = idx.search(q0, 100, async_=True)
    assert idx.finish() == []
    _same(torch, [a, b, c, s, e, f], [before, before_1, after, after_1, after_1, after])
    # the policy changes between submissions: the pending groups are flushed, results stay the same
    batches = _batches(torch, d, dtype, (64,) * 6, 100, 610)
    want = [idx.search(q, k) for q, k in batches]
    outs = []
    for i, (q, k) in enumerate(batches):
        idx.stationary_passes = (True, False, "auto", True, True, True)[i]
        idx.wide_passes = ("auto", "auto", True, True, False, "auto")[i]
        outs.append(idx.search(q, k, async_=True))
    assert idx.finish() == []
    _same(torch, outs, want)
    idx.close()


def test_removed_rows_keep_the_tombstone_passes(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    idx = _index(torch, d, dtype)
    batches = _batches(torch, d, dtype, (64,) * 4, 100, 700)
    _, n0 = _scan_launches(torch, idx, batches)
    assert n0 == 1
    gone = np.arange(0, N_LONG, 3)
    assert idx.remove_ids(gone) == gone.size
    want = [idx.search(q, k) for q, k in batches]
    for wide, launches in ((True, 2), (False, 3)):   # 8 groups: wide passes of 6, resident ones of 3
        idx.wide_passes = wide
        got, n1 = _scan_launches(torch, idx, batches)
        assert n1 == launches
        _same(torch, got, want)
    idx.close()


@pytest.mark.parametrize("cls", ["ints", "neg"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_stationary_scans_are_exact(torch_mod, dtype, cls):
    """tests/exact_inputs.py: every product and partial sum is an fp32 number, so the scores must be the float64 ones
    bit for bit.  Seven batches of 64 are a pass of 8 groups and one of 6."""
    torch = torch_mod
    n, d = ex.N_FILTER, 768
    corpus, queries, unit = ex.case(cls, n, d, ex.COALESCE_BATCHES * ex.COALESCE_B)
    ex.assert_exactly_summable(corpus, queries, unit)
    idx = _index(torch, d, dtype, corpus=np.asarray(corpus))
    tq = _tq(torch, np.asarray(queries), dtype)
    batches = [(tq[i * 64: (i + 1) * 64], 100) for i in range(ex.COALESCE_BATCHES)]
    want = ex.expected_topk(corpus, queries, 100)
    outs, n_scan = _scan_launches(torch, idx, batches)
    assert n_scan == 2
    assert idx.last_search_info()["path"] == "filter"
    for i, (D, I) in enumerate(outs):
        assert np.array_equal(I.cpu().numpy(), want[1][i * 64: (i + 1) * 64]), i
        assert np.array_equal(D.cpu().numpy(), want[0][i * 64: (i + 1) * 64]), i
    idx.close()
