"""The survivor epilogue of the coalesced scans (epilogue_multi: wave-uniform ballots per group and per accumulator
register): the corpus's partial last row block, a row block in which every lane and register of one group hits, a row
that survives in several groups of one pass, and a staging area that overflows.  The check is the wide tests' own: equal to
one scan per batch (coalesce = False) and to the synchronous search, bit for bit in scores and ids."""
import numpy as np
import pytest

from helpers import make_corpus
from oracle import oracle

pytestmark = pytest.mark.gpu

N = 100_013          # 3125 row blocks of 32 and one of 13
TAIL = N - N % 32    # first row of the partial block
RUN6, RUN1 = 32 * 1234, 32 * 2000   # block-aligned runs of 32 equal rows
SUM6, SUM1 = 77_777, 55_555         # rows along the sum of one query per group
K = 100


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _tq(torch, a, dtype):
    t = torch.from_numpy(a).cuda()
    return t.half() if dtype == "f16" else t.bfloat16()


def _unit(x, dtype):
    x = x.astype(np.float64)
    return oracle.quantize((x / np.linalg.norm(x)).astype(np.float32)[None], dtype)[0]


def _planted(d, dtype):
    """corpus, the three 64-query batches of the 6-group pass, the five 32-query batches of the partial passes, and
    per batch list the planted (query, row) pairs"""
    corpus = make_corpus(N, d, seed=7, dtype=dtype)
    six = [make_corpus(64, d, seed=100 + i, dtype=dtype) for i in range(3)]
    one = [make_corpus(32, d, seed=250 + i, dtype=dtype) for i in range(5)]
    hits6, hits1 = [[] for _ in six], [[] for _ in one]
    # the last 13 rows: copies of queries (the row bound is applied in this block only)
    for i in range(N % 32):
        if i < 8:
            b, q = i % 3, (5 * i + 1) % 64
            corpus[TAIL + i] = six[b][q]
            hits6[b].append((q, TAIL + i))
        else:
            b, q = i - 8, 2 * i
            corpus[TAIL + i] = one[b][q]
            hits1[b].append((q, TAIL + i))
    # 32 consecutive block-aligned rows equal to one query: all 64 lanes' columns of that query and all 16
    # accumulator registers of its group hit
    corpus[RUN6:RUN6 + 32] = six[1][40]
    corpus[RUN1:RUN1 + 32] = one[1][7]
    # one row along the sum of one query from each group: it survives in every group of the pass
    qs6 = [(g // 2, (g % 2) * 32 + 3 + g) for g in range(6)]
    corpus[SUM6] = _unit(sum(six[b][q] for b, q in qs6), dtype)
    for b, q in qs6:
        hits6[b].append((q, SUM6))
    corpus[SUM1] = _unit(sum(one[b][b + 1] for b in range(5)), dtype)
    for b in range(5):
        hits1[b].append((b + 1, SUM1))
    return corpus, six, one, hits6, hits1


def _run(torch, idx, batches, coalesce):
    idx.coalesce = coalesce
    outs = [idx.search(q, K, async_=True) for q in batches]
    redone = idx.finish()
    torch.cuda.synchronize()
    return outs, redone


def _same(torch, a, b):
    for (D, I), (D0, I0) in zip(a, b):
        assert torch.equal(I, I0) and torch.equal(D, D0)


def _check(torch, idx, batches, hits):
    want, _ = _run(torch, idx, batches, False)
    got, redone = _run(torch, idx, batches, True)
    assert redone == []
    _same(torch, got, want)
    for q, (D, I) in zip(batches, got):
        Ds, Is = idx.search(q, K)
        assert torch.equal(Is, I) and torch.equal(Ds, D)
    for (D, I), planted in zip(got, hits):
        ids = I.cpu().numpy()
        assert ids.max() < N
        for q, row in planted:
            assert row in ids[q], (q, row)
    return got


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [768, 384])   # 384: three windows per row block, the odd walk
def test_partial_last_row_block(torch_mod, dtype, d):
    torch = torch_mod
    from tristage_rag_amd.index import FlatIPIndex
    corpus, six, one, hits6, hits1 = _planted(d, dtype)
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_tq(torch, corpus, dtype))
    idx.classic_filter = True
    idx.wide_passes = True
    six, one = [_tq(torch, q, dtype) for q in six], [_tq(torch, q, dtype) for q in one]
    got = _check(torch, idx, six, hits6)                  # one pass of 6 groups: scan_wide_kernel<*, 6>
    run = got[1][1].cpu().numpy()[40]
    assert np.isin(np.arange(RUN6, RUN6 + 32), run).all()
    # Single-group batches flushed at finish() as one pass.  A pass whose images fit the LDS takes scan_multi_kernel
    # (the same epilogue): 2 and 3 groups at d = 768, 2 to 4 at d = 384; scan_wide_kernel gets 4 and 5 groups at
    # d = 768 and 5 at d = 384.  (Wide passes of 2 and 3 groups: test_small_wide_passes.)  The rows past the corpus's
    # end in the last block are zero and score 0, under every threshold: a lost row bound shows in `ids.max() < N` of
    # _check only where such a row is a survivor, so the planted rows, not the bound, are what these passes check.
    for groups in (2, 3, 4, 5):
        got = _check(torch, idx, one[:groups], hits1[:groups])
        run = got[1][1].cpu().numpy()[7]
        assert np.isin(np.arange(RUN1, RUN1 + 32), run).all()
    idx.close()


def test_small_wide_passes(torch_mod):
    """The planted rows in wide passes of 2 and 3 groups: at d = 1536 one group's image is all the LDS-resident kernel
    holds, so these passes take scan_wide_kernel<f16, 2> and <f16, 3>."""
    torch = torch_mod
    d, dtype = 1536, "f16"
    from tristage_rag_amd.index import FlatIPIndex
    corpus, _, one, _, hits1 = _planted(d, dtype)
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_tq(torch, corpus, dtype))
    idx.classic_filter = True
    idx.wide_passes = True
    one = [_tq(torch, q, dtype) for q in one]
    for groups in (2, 3):
        got = _check(torch, idx, one[:groups], hits1[:groups])
        run = got[1][1].cpu().numpy()[7]
        assert np.isin(np.arange(RUN1, RUN1 + 32), run).all()
    idx.close()


# A workgroup's 8 waves take 8 consecutive row blocks per iteration of its walk, and the repeated half of the corpus is
# 1 565 consecutive whole row blocks: whatever the grid, some workgroup has 8 row blocks in which every row ties.  With
# TIES queries along the repeated row that workgroup alone stages 8 x 32 x TIES survivors, twice the largest staging
# area there is (TS_WIDE_MAX_STAGE = 8192 entries in a wide pass, TS_MULTI_MAX_STAGE = 4096 in an LDS-resident one).
TIES = 64
STAGE_MAX = 8192
assert 8 * 32 * TIES >= 2 * STAGE_MAX
# The repeated rows start at a multiple of 8 row blocks, so no workgroup walks other rows and repeated ones in the same
# iteration: in a tombstone pass a survivor of any batch that meets a full staging area makes its own batch redo
# (nothing there knows whether its row is live), which is right but would make "only `ties` is redone" a matter of
# which wave of that one workgroup comes first.  Other rows of a workgroup lie in earlier iterations, staged before.
N_FULL = 100_000
N_OTHER = 195 * 8 * 32   # 49 920 rows that are not the repeated one; 50 080 that are


@pytest.mark.parametrize("removed", [False, True])
@pytest.mark.parametrize("wide", [True, False])
def test_staging_area_full(torch_mod, wide, removed):
    """Half the corpus (50 080 of 100 000 rows) is one repeated row and the 64 queries of one batch lie along it.  Its survivors overrun the
    staging area of every workgroup that walks the repeated half (see TIES above), so the epilogue's overflow branch
    runs: the direct append to the lists on a plain index, and after a removal, in the tombstone kernels, the atomicMax
    that pushes the list's count past its capacity.  Either way the lists overflow too, the batch is redone by finish()
    and the batches that share its pass are not.  wide: 2 + 2 + 2 groups in scan_wide_kernel<f16, 6>; not wide:
    1 + 2 groups in scan_multi_kernel<f16, 3>."""
    torch = torch_mod
    d, dtype, n, m = 768, "f16", N_FULL, N_OTHER
    row = make_corpus(1, d, seed=500, dtype=dtype)
    corpus = np.concatenate([make_corpus(m, d, seed=501, dtype=dtype), np.repeat(row, n - m, axis=0)])
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_tq(torch, corpus, dtype))
    idx.classic_filter = True
    idx.wide_passes = wide
    if removed:
        rng = np.random.default_rng(9)
        gone = np.concatenate([rng.choice(m, 150, replace=False), m + rng.choice(n - m, 150, replace=False)])
        assert idx.remove_ids(gone) == gone.size
    ties = _tq(torch, np.repeat(row, TIES, axis=0), dtype)
    # the other batches score the repeated row below zero, far under their thresholds: only `ties` can overflow
    qa = make_corpus(64, d, seed=502, dtype=dtype)
    qa *= -np.sign(qa.astype(np.float64) @ row[0].astype(np.float64))[:, None].astype(qa.dtype)
    qa = _tq(torch, qa, dtype)
    qs = (qa, ties, qa) if wide else (qa[:32], ties)
    want = [idx.search(q, 30) for q in qs]
    idx.coalesce = False
    single = [idx.search(q, 30, async_=True) for q in qs]
    idx.finish()   # (one scan per batch: `ties` overflows its lists there too and is redone)
    _same(torch, single, want)
    idx.coalesce = True
    outs = [idx.search(q, 30, async_=True) for q in qs]
    last = int(idx._lib.ts_index_last_ticket(idx._h))
    tickets = [last - len(qs) + 1 + i for i in range(len(qs))]
    redone = idx.finish()
    assert redone == [tickets[1]]
    _same(torch, outs, want)
    _same(torch, outs, single)
    if removed:
        for _, I in outs:
            assert not np.isin(I.cpu().numpy(), gone).any()
    idx.close()
