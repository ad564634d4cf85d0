"""Query-stationary passes on walks of every shape the split walk of scan_qstat_kernel distinguishes:
a main loop for the steps whose refills all lie inside the walk and a tail of the last three, over a ring of 15 windows
whose slots repeat every 5 steps at d = 768 and every 3 at d = 640.  A corpus of n = 32 * (CUs * s + r) - 23 rows gives
workgroups of s and of s + 1 steps in one launch and a last block of 9 rows; s runs over walks with no, one and a few
main steps, one period of the ring, just past one and two periods, and several turns.  Stationary passes are forced;
their results are compared with one scan per batch and with the synchronous search, ids and scores, bit for bit."""
import functools

import numpy as np
import pytest

import exact_inputs as ex
from qstat_helpers import (batches_of as _batches, index_of as _index, run as _run, same as _same,
                           scan_launches as _scan_launches, sync_search as _sync, tq as _tq)

pytestmark = pytest.mark.gpu

STEPS = (4, 5, 6, 7, 9, 11, 16)
PAIRS_ALL = ((768, "f16"), (640, "bf16"))
PAIRS_S5 = ((768, "bf16"), (640, "f16"))
SEVEN = (32, 32, 20, 32, 1, 32, 31)   # seven groups: one wave of the workgroup owns no group


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=1)
def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rows(s, r_half):
    cus = _cus()
    r = cus // 2 if r_half else 8
    n = 32 * (cus * s + r) - 23
    assert n >= 33_001 and (n + 31) // 32 == cus * s + r and n % 32 == 9
    return n


def _held(torch, idx, batches, launches):
    sync = _sync(idx, batches)
    want, _ = _run(torch, idx, batches, False)
    got, n_scan = _scan_launches(torch, idx, batches)
    assert n_scan == launches
    _same(torch, got, want)
    _same(torch, got, sync)


CASES = [(s, h, d, dt) for s in STEPS for h in (False, True) for d, dt in PAIRS_ALL] + \
        [(5, h, d, dt) for h in (False, True) for d, dt in PAIRS_S5]


@pytest.mark.parametrize("s,r_half,d,dtype", CASES)
def test_walks_of_s_and_s_plus_1_steps(torch_mod, s, r_half, d, dtype):
    torch = torch_mod
    idx = _index(torch, d, dtype, n=_rows(s, r_half))
    _held(torch, idx, _batches(torch, d, dtype, (64,) * 4, 100, 1000 + s), 1)   # a pass of 8 groups
    if s == 5:
        _held(torch, idx, _batches(torch, d, dtype, SEVEN, 100, 1100), 1)       # a pass of 7
    idx.close()


def test_a_split_walk_is_exact(torch_mod):
    """tests/exact_inputs.py: every product and partial sum is an fp32 number, so the scores are the float64 ones bit
    for bit.  s = 6 and r = 8: walks of 6 and 7 steps, three and four of them in the main loop."""
    torch = torch_mod
    n, d, dtype = _rows(6, False), 768, "f16"
    corpus, queries, unit = ex.case("ints", n, d, 4 * 64)
    ex.assert_exactly_summable(corpus, queries, unit)
    idx = _index(torch, d, dtype, corpus=np.asarray(corpus))
    tq = _tq(torch, np.asarray(queries), dtype)
    batches = [(tq[i * 64: (i + 1) * 64], 100) for i in range(4)]
    want = ex.expected_topk(corpus, queries, 100)
    outs, n_scan = _scan_launches(torch, idx, batches)
    assert n_scan == 1
    assert idx.last_search_info()["path"] == "filter"
    for i, (D, I) in enumerate(outs):
        assert np.array_equal(I.cpu().numpy(), want[1][i * 64: (i + 1) * 64]), i
        assert np.array_equal(D.cpu().numpy(), want[0][i * 64: (i + 1) * 64]), i
    idx.close()
