"""Wide coalesced passes (scan_wide_kernel): forced on at a small corpus, they give exactly what one scan per batch
(coalesce = False) and the synchronous search give, bit for bit; the auto policy takes them above the Infinity Cache."""
import numpy as np
import pytest

from helpers import make_corpus

pytestmark = pytest.mark.gpu

N = 100_000   # above the filter path's floor; classic_filter puts it on the five-launch path that coalesces
WIDE = 6      # ts_coalesce_groups_wide for f16 / bf16


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _tq(torch, a, dtype):
    t = torch.from_numpy(a).cuda()
    return t.half() if dtype == "f16" else t.bfloat16()


def _index(torch, d, dtype, n=N, seed=7, wide=True):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_tq(torch, make_corpus(n, d, seed=seed, dtype=dtype), dtype))
    idx.classic_filter = True
    idx.wide_passes = wide
    return idx


def _run(torch, idx, batches, coalesce):
    idx.coalesce = coalesce
    outs = [idx.search(q, k, async_=True) for q, k in batches]
    redone = idx.finish()
    torch.cuda.synchronize()
    return outs, redone


def _same(torch, a, b):
    for (D, I), (D0, I0) in zip(a, b):
        assert torch.equal(I, I0) and torch.equal(D, D0)


def _scan_launches(torch, idx, batches, coalesce):
    idx.set_profiling(True, every=1)
    idx.timings(reset=True)
    outs, redone = _run(torch, idx, batches, coalesce)
    n = idx.timings(reset=True)["filter_scan"][1]
    idx.set_profiling(False)
    assert redone == []
    return outs, n


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [384, 700, 768, 1024])
def test_wide_passes_equal_one_scan_per_batch(torch_mod, dtype, d):
    torch = torch_mod
    idx = _index(torch, d, dtype)
    # 1..13 batches of 64: passes of 6 groups and partial ones of 2 and 4 at finish()
    for nb in (1, 2, 3, 4, 5, 13):
        batches = [(_tq(torch, make_corpus(64, d, seed=100 + i, dtype=dtype), dtype), 100) for i in range(nb)]
        want, _ = _run(torch, idx, batches, False)
        got, redone = _run(torch, idx, batches, True)
        assert redone == []
        _same(torch, got, want)
    # mixed sizes and k: 19 groups of one- and two-group batches, passes of 6 that batches straddle and one of 1
    sizes, ks = (1, 8, 33, 64, 64, 33, 1, 8, 64, 33, 1, 64), (10, 1000, 100, 7, 257, 100, 64, 1, 1000, 33, 5, 100)
    batches = [(_tq(torch, make_corpus(b, d, seed=200 + i, dtype=dtype), dtype), k)
               for i, (b, k) in enumerate(zip(sizes, ks))]
    want, _ = _run(torch, idx, batches, False)
    got, redone = _run(torch, idx, batches, True)
    assert redone == []
    _same(torch, got, want)
    for (q, k), (D, I) in zip(batches, got):
        Ds, Is = idx.search(q, k)
        assert torch.equal(Is, I) and torch.equal(Ds, D)
    idx.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d,groups", [(768, 3), (768, 4), (768, 5), (1024, 3), (1536, 1), (1536, 2), (1536, 6)])
def test_partial_wide_passes(torch_mod, dtype, d, groups):
    """Single-group batches flushed at finish() as one pass: LDS-resident where the images fit (3 groups at d = 768,
    1 at d = 1536), wide otherwise (4 and 5 at d = 768, 3 at d = 1024, 2 and 6 at d = 1536)."""
    torch = torch_mod
    idx = _index(torch, d, dtype)
    batches = [(_tq(torch, make_corpus(32, d, seed=250 + i, dtype=dtype), dtype), 100) for i in range(groups)]
    want, n0 = _scan_launches(torch, idx, batches, False)
    got, n1 = _scan_launches(torch, idx, batches, True)
    assert (n0, n1) == (groups, 1)
    _same(torch, got, want)
    for (q, k), (D, I) in zip(batches, got):
        Ds, Is = idx.search(q, k)
        assert torch.equal(Is, I) and torch.equal(Ds, D)
    idx.close()


def test_wide_scans_are_shared(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    idx = _index(torch, d, dtype)
    batches = [(_tq(torch, make_corpus(64, d, seed=700 + i, dtype=dtype), dtype), 100) for i in range(6)]
    want, n0 = _scan_launches(torch, idx, batches, False)
    got, n1 = _scan_launches(torch, idx, batches, True)
    assert (n0, n1) == (6, 2)   # 12 groups: two wide passes
    _same(torch, got, want)
    # forced off: the LDS-resident passes of 3 groups
    idx.wide_passes = False
    got, n2 = _scan_launches(torch, idx, batches, True)
    assert n2 == 4
    _same(torch, got, want)
    # the width changes between submissions: the pending groups are flushed, results stay the same
    idx.coalesce = True
    outs = []
    for i, (q, k) in enumerate(batches):
        idx.wide_passes = (True, False, "auto")[i % 3]
        outs.append(idx.search(q, k, async_=True))
    assert idx.finish() == []
    _same(torch, outs, want)
    idx.close()


def test_auto_policy_above_the_infinity_cache(torch_mod):
    """200 k x 1024 (410 MB): no LDS-resident coalescing at d = 1024, wide passes with the auto policy."""
    torch = torch_mod
    d, dtype = 1024, "bf16"
    idx = _index(torch, d, dtype, n=200_000, wide="auto")
    batches = [(_tq(torch, make_corpus(64, d, seed=800 + i, dtype=dtype), dtype), 100) for i in range(5)]
    want, n0 = _scan_launches(torch, idx, batches, False)
    got, n1 = _scan_launches(torch, idx, batches, True)
    assert (n0, n1) == (5, -(-10 // WIDE))
    _same(torch, got, want)
    idx.wide_passes = False
    got, n2 = _scan_launches(torch, idx, batches, True)
    assert n2 == 5   # two groups per LDS-resident pass: nothing coalesced
    _same(torch, got, want)
    idx.close()
    # 100 k x 768 (154 MB) keeps the LDS-resident passes of 3 groups
    idx = _index(torch, 768, "f16", wide="auto")
    batches = [(_tq(torch, make_corpus(64, 768, seed=810 + i, dtype="f16"), "f16"), 100) for i in range(3)]
    _, n3 = _scan_launches(torch, idx, batches, True)
    assert n3 == 2
    idx.close()
    # and so does 400 k x 384 (307 MB): its LDS-resident passes take 4 groups
    idx = _index(torch, 384, "f16", n=400_000, wide="auto")
    batches = [(_tq(torch, make_corpus(64, 384, seed=820 + i, dtype="f16"), "f16"), 100) for i in range(3)]
    want, _ = _scan_launches(torch, idx, batches, False)
    got, n4 = _scan_launches(torch, idx, batches, True)
    assert n4 == 2
    _same(torch, got, want)
    idx.close()


def test_default_policy_and_flags(torch_mod):
    from tristage_rag_amd import _lib
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(768, dtype="f16")
    assert idx.wide_passes == "auto" and idx.coalesce
    idx.close()
    assert _lib.TS_FLAG_WIDE_PASSES & _lib.TS_FLAG_NO_WIDE_PASSES == 0


def test_queries_overwritten_right_after_submission(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    idx = _index(torch, d, dtype)
    qs = [_tq(torch, make_corpus(64, d, seed=300 + i, dtype=dtype), dtype) for i in range(5)]
    want = [idx.search(q, 100) for q in qs]
    buf = torch.empty_like(qs[0])
    outs = []
    for i, q in enumerate(qs):
        buf.copy_(q)
        outs.append(idx.search(buf, 100, async_=True))
        buf.copy_(qs[(i + 1) % 5] * 0.5)   # on the same stream, before the held scan runs
    assert idx.finish() == []
    _same(torch, outs, want)
    idx.close()


def test_add_and_sync_search_between_held_batches(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    idx = _index(torch, d, dtype)
    q0 = _tq(torch, make_corpus(64, d, seed=400, dtype=dtype), dtype)
    q1 = _tq(torch, make_corpus(40, d, seed=401, dtype=dtype), dtype)
    before = idx.search(q0, 100)
    before_1 = idx.search(q1, 50)
    extra = _tq(torch, make_corpus(30_000, d, seed=402, dtype=dtype), dtype)
    a = idx.search(q0, 100, async_=True)
    b = idx.search(q1, 50, async_=True)
    idx.add(extra)   # held batches search the rows they were submitted against
    after = idx.search(q0, 100)
    after_1 = idx.search(q1, 50)
    c = idx.search(q0, 100, async_=True)
    s = idx.search(q1, 50)   # a synchronous search between held batches
    e = idx.search(q1, 50, async_=True)
    f = idx.search(q0, 100, async_=True)
    assert idx.finish() == []
    _same(torch, [a, b, c, s, e, f], [before, before_1, after, after_1, after_1, after])
    idx.close()


def test_failed_batch_inside_a_wide_pass_is_redone_alone(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    row = make_corpus(1, d, seed=500, dtype=dtype)
    corpus = np.concatenate([make_corpus(N // 2, d, seed=501, dtype=dtype), np.repeat(row, N // 2, axis=0)])
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_tq(torch, corpus, dtype))
    idx.classic_filter = True
    idx.wide_passes = True
    ties = _tq(torch, np.repeat(row, 8, axis=0), dtype)
    qa = make_corpus(64, d, seed=502, dtype=dtype)
    qa *= -np.sign(qa.astype(np.float64) @ row[0].astype(np.float64))[:, None].astype(qa.dtype)
    qa = _tq(torch, qa, dtype)
    # 2 + 1 + 2 groups: the tie batch shares one wide pass of 5 with two others
    qs = (qa, ties, qa)
    want = [idx.search(q, 30) for q in qs]
    idx.coalesce = True
    outs = [idx.search(q, 30, async_=True) for q in qs]
    tickets = [int(idx._lib.ts_index_last_ticket(idx._h)) - 2 + i for i in range(3)]
    redone = idx.finish()
    assert redone == [tickets[1]]
    _same(torch, outs, want)
    idx.close()


def test_unfinished_pass_limit(torch_mod):
    """test_coalesce_gpu.py's limit test with wide passes forced on."""
    torch = torch_mod
    d, dtype = 384, "f16"
    idx = _index(torch, d, dtype)
    qs = [_tq(torch, make_corpus(64, d, seed=600 + i, dtype=dtype), dtype) for i in range(4)]
    want = [idx.search(q, 100) for q in qs]
    # 130 batches of 64 exceed the 240 passes of 32 that may wait: an internal finish() runs in between
    outs = [idx.search(qs[i % 4], 100, async_=True) for i in range(130)]
    assert idx.finish() == []
    for i, o in enumerate(outs):
        _same(torch, [o], [want[i % 4]])
    idx.close()
