"""The pass prologue of query-stationary coalesced passes: a batch's sample scan and thresholds are
enqueued with its first pass instead of at submission, and a pass's sample scans (scan_qstat_sample_kernel), thresholds
(tau_batch_kernel) and selects (select_batch_kernel) take one launch each.  Nothing a caller can see may change:
pass_prologue = True against False, bit for bit, with the same filter scans and the same candidate counts (which is
what holds the thresholds themselves equal), no redo, and both equal to one scan per batch and to the synchronous
search."""
import pytest

from qstat_helpers import (N_LONG, N_SHORT, batches_of as _batches, index_of as _index, run as _run, same as _same,
                           scan_launches as _scan_launches, sync_search as _sync)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _both_forms(torch, idx, batches):
    """(results, filter scans, max candidates) of the held batches with the pass prologue off and on; no redo."""
    res = {}
    for pp in (False, True):
        idx.pass_prologue = pp
        outs, n_scan = _scan_launches(torch, idx, batches)   # (asserts that finish() redid nothing)
        res[pp] = (outs, n_scan, idx.last_search_info()["max_candidates"])
    idx.pass_prologue = "auto"
    print("filter scans", res[False][1], res[True][1], "max candidates", res[False][2], res[True][2])
    _same(torch, res[True][0], res[False][0])
    assert res[True][1] == res[False][1]
    assert res[True][2] == res[False][2]
    return res[True]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [768, 640])
@pytest.mark.parametrize("n", [N_SHORT, N_LONG])
def test_pass_prologue_changes_nothing(torch_mod, n, d, dtype):
    torch = torch_mod
    idx = _index(torch, d, dtype, n=n)
    assert idx.pass_prologue == "auto"

    def held(batches, launches):
        sync = _sync(idx, batches)
        want, _ = _run(torch, idx, batches, False)
        got, n_scan, _ = _both_forms(torch, idx, batches)
        _same(torch, got, want)
        _same(torch, got, sync)
        assert n_scan == launches

    # the batch patterns of test_qstat_gpu.py::test_stationary_passes_equal_one_scan_per_batch
    pool = _batches(torch, d, dtype, (64,) * 9, 100, 100)
    # 1 batch: scan_kernel's dense scan and its own launches; 2, 4: one partial pass; 5, 9: the fifth batch's thresholds
    # come with the second pass
    for nb, launches in ((1, 1), (2, 1), (4, 1), (5, 2), (9, 3)):
        held(pool[:nb], launches)
    # eight one-group batches, mixed k (m on both sides of the threshold kernels' KEEP rule where the sample allows it):
    # eight sample groups, eight thresholds and eight selects in one launch each.  Then the batch of 33: a pass of 2.
    sizes8, ks8 = (32, 1, 8, 17, 5, 31, 2, 32), (1, 7, 100, 257, 1000, 7, 100, 1)
    eight = _batches(torch, d, dtype, sizes8 + (33,), ks8 + (257,), 200)
    held(eight[:8], 1)
    held(eight, 2)
    # the batch of 33 straddles two passes: nine sample groups for a pass of 8 (two sample launches), its thresholds with
    # the first pass, its select with the second
    split = _batches(torch, d, dtype, sizes8[:7] + (33, 64), ks8[:7] + (1000, 100), 220)
    held(split, 2)
    # seven groups: one wave of the workgroup owns no group, in the sample launch too
    held(_batches(torch, d, dtype, (32, 32, 20, 32, 1, 32, 31), 100, 300), 1)
    idx.close()


def _gen_index(torch, n, d, seed):
    """n x d f16 rows generated on the GPU in seeded blocks (bench.py's gen_rows), stationary passes forced."""
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype="f16")
    idx.reserve(n)
    step = 400_000
    for i, r0 in enumerate(range(0, n, step)):
        g = torch.Generator(device="cuda").manual_seed(seed + i)
        x = torch.randn((min(step, n - r0), d), generator=g, device="cuda", dtype=torch.float32)
        idx.add((x / (x.norm(dim=1, keepdim=True) + 1e-8)).half())
        del x
    idx.classic_filter = True
    idx.stationary_passes = True
    return idx


@pytest.mark.parametrize("n,sample_blocks", [(1_100_003, 268), (3_200_000, 781)])
def test_sample_walks_of_several_steps(torch_mod, n, sample_blocks):
    """More than 256 sample blocks: at 268 twelve workgroups of 256 walk two blocks and the rest one; at 781 every
    workgroup walks 3 or 4, so the ring (2.5 to 3 row blocks) wraps in sample mode."""
    torch = torch_mod
    d = 640
    idx = _gen_index(torch, n, d, seed=4000)
    batches = _batches(torch, d, "f16", (64, 64, 33, 64), (100, 1000, 10, 100), 4100)
    _, n_scan, _ = _both_forms(torch, idx, batches)
    assert n_scan == 1   # 7 groups
    assert idx.last_search_info()["sample_rows"] == sample_blocks * 32
    idx.close()


def test_queries_overwritten_after_submission(torch_mod):
    """Only the query preparation reads the caller's queries, and it is enqueued at submission: overwriting them on the
    submitting stream right after the asynchronous search returns changes nothing, although the sample scans and the
    thresholds are enqueued later."""
    torch = torch_mod
    d, dtype = 768, "f16"
    idx = _index(torch, d, dtype, n=N_SHORT)
    idx.pass_prologue = True
    idx.coalesce = True
    batches = _batches(torch, d, dtype, (64, 33, 64, 64, 64), 100, 5000)   # a pass of 8 and a partial one
    want, redone = _run(torch, idx, batches, True)
    assert redone == []
    outs = []
    for q, k in batches:
        late = q.clone()
        outs.append(idx.search(late, k, async_=True))
        late.zero_()
    assert idx.finish() == []
    torch.cuda.synchronize()
    _same(torch, outs, want)
    idx.close()
