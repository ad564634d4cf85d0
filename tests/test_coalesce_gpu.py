"""Coalesced passes (TS_FLAG_COALESCE): asynchronous batches that share one corpus scan give exactly what one scan
per batch gives (coalesce = False), bit for bit, whatever shares their pass and whatever happens between them."""
import numpy as np
import pytest

from helpers import make_corpus

pytestmark = pytest.mark.gpu

N = 100_000   # above the filter path's floor; classic_filter puts it on the five-launch path that coalesces


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _tq(torch, a, dtype):
    t = torch.from_numpy(a).cuda()
    return t.half() if dtype == "f16" else t.bfloat16()


def _index(torch, d, dtype, n=N, seed=7):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_tq(torch, make_corpus(n, d, seed=seed, dtype=dtype), dtype))
    idx.classic_filter = True
    return idx


def _run(torch, idx, batches, coalesce):
    """batches: [(queries, k)] submitted back to back; returns [(D, I)] after finish() and the redone tickets"""
    idx.coalesce = coalesce
    outs = [idx.search(q, k, async_=True) for q, k in batches]
    redone = idx.finish()
    torch.cuda.synchronize()
    return outs, redone


def _same(torch, a, b):
    for (D, I), (D0, I0) in zip(a, b):
        assert torch.equal(I, I0) and torch.equal(D, D0)


def test_groups_per_pass_on_device():
    from tristage_rag_amd import _lib
    lib = _lib.load()
    assert [lib.ts_coalesce_groups(d, 1) for d in (384, 768, 1024)] == [4, 3, 2]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [384, 768, 1024])
def test_pending_batches_and_mixed_sizes(torch_mod, dtype, d):
    torch = torch_mod
    idx = _index(torch, d, dtype)
    for nb in (1, 2, 3, 5, 7):
        batches = [(_tq(torch, make_corpus(64, d, seed=100 + i, dtype=dtype), dtype), 100) for i in range(nb)]
        want, _ = _run(torch, idx, batches, False)
        got, redone = _run(torch, idx, batches, True)
        assert redone == []
        _same(torch, got, want)
    # mixed sizes and k: groups of 1, 8, 32 + 1, 32 + 8 and 2 x 32 queries; the 64s straddle passes
    sizes, ks = (1, 8, 33, 40, 64, 64, 33, 1), (10, 1000, 100, 7, 257, 100, 64, 1)
    batches = [(_tq(torch, make_corpus(b, d, seed=200 + i, dtype=dtype), dtype), k)
               for i, (b, k) in enumerate(zip(sizes, ks))]
    want, _ = _run(torch, idx, batches, False)
    got, redone = _run(torch, idx, batches, True)
    assert redone == []
    _same(torch, got, want)
    # and against the synchronous search
    for (q, k), (D, I) in zip(batches, got):
        Ds, Is = idx.search(q, k)
        assert torch.equal(Is, I) and torch.equal(Ds, D)
    idx.close()


@pytest.mark.parametrize("d,groups", [(384, 4), (768, 3), (1024, 2)])
def test_scans_are_shared(torch_mod, d, groups):
    """The equality tests would also pass if nothing were coalesced: count the filter-scan launches."""
    torch = torch_mod
    dtype = "f16"
    idx = _index(torch, d, dtype)
    batches = [(_tq(torch, make_corpus(64, d, seed=700 + i, dtype=dtype), dtype), 100) for i in range(3)]
    launches = {}
    for co in (False, True):
        idx.set_profiling(True, every=1)
        idx.timings(reset=True)
        outs, redone = _run(torch, idx, batches, co)
        launches[co] = idx.timings(reset=True)["filter_scan"][1]
        idx.set_profiling(False)
        assert redone == []
        if co:
            _same(torch, outs, want)
        else:
            want = outs
    # 3 batches of 64 are 6 groups: one scan per batch without coalescing, ceil(6 / G) scans with it
    # (at d = 1024 two groups per pass is what the plain scan does: nothing is coalesced)
    assert launches[False] == 3
    assert launches[True] == (-(-6 // groups) if groups >= 3 else 3)
    idx.close()


def test_queries_overwritten_right_after_submission(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    idx = _index(torch, d, dtype)
    qs = [_tq(torch, make_corpus(64, d, seed=300 + i, dtype=dtype), dtype) for i in range(4)]
    want = [idx.search(q, 100) for q in qs]
    buf = torch.empty_like(qs[0])
    outs = []
    for i, q in enumerate(qs):
        buf.copy_(q)
        outs.append(idx.search(buf, 100, async_=True))
        buf.copy_(qs[(i + 1) % 4] * 0.5)   # on the same stream, before the held scan runs
    assert idx.finish() == []
    _same(torch, outs, want)
    idx.close()


def test_add_sync_and_filtered_searches_between(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    idx = _index(torch, d, dtype)
    q0 = _tq(torch, make_corpus(64, d, seed=400, dtype=dtype), dtype)
    q1 = _tq(torch, make_corpus(40, d, seed=401, dtype=dtype), dtype)
    before = idx.search(q0, 100)
    extra = _tq(torch, make_corpus(30_000, d, seed=402, dtype=dtype), dtype)
    # a batch held across add() searches the rows it was submitted against
    a = idx.search(q0, 100, async_=True)
    idx.add(extra)
    after = idx.search(q0, 100)
    b = idx.search(q0, 100, async_=True)
    assert idx.finish() == []
    _same(torch, [a, b], [before, after])
    # a synchronous and a filtered search between held batches
    allowed = np.zeros(idx.ntotal, dtype=bool)
    allowed[::3] = True
    want_f = idx.search(q1, 50, allowed=allowed)
    want_1 = idx.search(q1, 50)
    x = idx.search(q0, 100, async_=True)
    s = idx.search(q1, 50)
    y = idx.search(q1, 50, async_=True)
    f = idx.search(q1, 50, async_=True, allowed=allowed)
    z = idx.search(q0, 100, async_=True)
    assert idx.finish() == []
    _same(torch, [x, s, y, f, z], [after, want_1, want_1, want_f, after])
    # another stream: the held work is flushed on the first one and the result stays right
    side = torch.cuda.Stream()
    u = idx.search(q1, 50, async_=True)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v = idx.search(q1, 50, async_=True)
        idx.flush()
    torch.cuda.current_stream().wait_stream(side)
    assert idx.finish() == []
    _same(torch, [u, v], [want_1, want_1])
    # held on stream A, then B.wait_stream(A), a search on B and finish() on B: B's sync must cover A's held scan
    # and select, which are only enqueued when the search on B flushes the queue
    main = torch.cuda.current_stream()
    for coalesced_on_b in (False, True):
        w = idx.search(q0, 100, async_=True)              # held on the main stream
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if coalesced_on_b:
                x = idx.search(q1, 50, async_=True)        # joins the queue on B: the queue moves there
            else:
                x = idx.search(q1, 50)                     # cannot join: runs after the held batch
            redone = idx.finish()                          # syncs B only
            assert redone == []
            got = (w[0].clone(), w[1].clone(), x[0].clone(), x[1].clone())   # B reads A's outputs
        torch.cuda.synchronize()
        assert torch.equal(got[1], after[1]) and torch.equal(got[0], after[0])
        assert torch.equal(got[3], want_1[1]) and torch.equal(got[2], want_1[0])
    idx.close()


def test_failed_batch_inside_a_shared_pass_is_redone_alone(torch_mod):
    torch = torch_mod
    d, dtype = 768, "f16"
    # half the corpus is one repeated row: a query along it ties on 50 000 rows and overflows its candidate lists
    row = make_corpus(1, d, seed=500, dtype=dtype)
    corpus = np.concatenate([make_corpus(N // 2, d, seed=501, dtype=dtype), np.repeat(row, N // 2, axis=0)])
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_tq(torch, corpus, dtype))
    idx.classic_filter = True
    ties = _tq(torch, np.repeat(row, 8, axis=0), dtype)
    # the other batches score the repeated row below zero, far under their thresholds: only `ties` can overflow
    qa = make_corpus(64, d, seed=502, dtype=dtype)
    qa *= -np.sign(qa.astype(np.float64) @ row[0].astype(np.float64))[:, None].astype(qa.dtype)
    qa = _tq(torch, qa, dtype)
    want = [idx.search(q, 30) for q in (qa, ties, qa)]
    idx.coalesce = True
    outs = [idx.search(q, 30, async_=True) for q in (qa, ties, qa)]
    tickets = [int(idx._lib.ts_index_last_ticket(idx._h)) - 2 + i for i in range(3)]
    redone = idx.finish()
    assert redone == [tickets[1]]
    _same(torch, outs, want)
    idx.close()


def test_unfinished_pass_limit(torch_mod):
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
