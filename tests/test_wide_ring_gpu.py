"""Wide coalesced passes (scan_wide_kernel) with the two-window corpus ring and LDS-DMA query windows: bit for bit
what one scan per batch (coalesce = False) and the synchronous search give, for walks where some waves have one row
block fewer or none at all.  Full passes of 6 groups at odd and even window counts per row block (d = 384: 3,
640: 5, 768: 6, 1024: 8); partial passes of 2..5 groups at d = 1536 (12 windows) and 1664 (13), where the images of
two groups no longer fit the LDS, so every one of them takes the wide kernel.  Each case checks that the batches
shared one scan launch."""
import pytest

from helpers import make_corpus

pytestmark = pytest.mark.gpu

# 1 025 row blocks: every wave has at most one, the last workgroup has one active wave and seven without work;
# 4 101 row blocks: on the MI355X's 256 workgroups (2 048 waves) the first five waves walk three blocks, the others two
SIZES = (32 * 1024 + 1, 32 * (2 * 2048 + 5))


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _tq(torch, a, dtype):
    t = torch.from_numpy(a).cuda()
    return t.half() if dtype == "f16" else t.bfloat16()


def _run(torch, idx, batches, coalesce):
    idx.coalesce = coalesce
    idx.set_profiling(True, every=1)
    idx.timings(reset=True)
    outs = [idx.search(q, k, async_=True) for q, k in batches]
    redone = idx.finish()
    torch.cuda.synchronize()
    n = idx.timings(reset=True)["filter_scan"][1]
    idx.set_profiling(False)
    assert redone == []
    return outs, n


def _check(torch, idx, batches):
    want, n0 = _run(torch, idx, batches, False)
    got, n1 = _run(torch, idx, batches, True)
    assert (n0, n1) == (len(batches), 1)   # one scan per batch, then one shared pass
    for (D, I), (D0, I0) in zip(got, want):
        assert torch.equal(I, I0) and torch.equal(D, D0)
    for (q, k), (D, I) in zip(batches, got):
        Ds, Is = idx.search(q, k)
        assert torch.equal(Is, I) and torch.equal(Ds, D)


def _index(torch, d, dtype, n):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_tq(torch, make_corpus(n, d, seed=11, dtype=dtype), dtype))
    idx.classic_filter = True
    idx.wide_passes = True
    return idx


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [384, 640, 768, 1024])
@pytest.mark.parametrize("n", SIZES)
def test_wide_ring_full_pass(torch_mod, dtype, d, n):
    torch = torch_mod
    idx = _index(torch, d, dtype, n)
    # three batches of 64: one pass of 6 groups
    _check(torch, idx, [(_tq(torch, make_corpus(64, d, seed=300 + i, dtype=dtype), dtype), 100) for i in range(3)])
    idx.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [1536, 1664])
@pytest.mark.parametrize("n", SIZES)
def test_wide_ring_partial_passes(torch_mod, dtype, d, n):
    torch = torch_mod
    idx = _index(torch, d, dtype, n)
    # 2..5 single-group batches flushed at finish() as one pass
    for groups in (2, 3, 4, 5):
        _check(torch, idx, [(_tq(torch, make_corpus(32, d, seed=400 + 10 * groups + i, dtype=dtype), dtype), 50)
                            for i in range(groups)])
    idx.close()
