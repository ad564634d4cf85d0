"""`ts_ivf_train` on the MI355X against the float64-normalised model of tests/ivf_train_model.py, one k-means
iteration at a time ("Train.").

Training is deterministic and `train(niter=t)` accepts every t >= 0, so fresh indices trained with niter = t and t + 1
hold consecutive states C_t, C_{t+1} of one run.  For every checked t:

1. the sample X is rebuilt on the host from the seeded shuffle (a Python replica) and the input rounded to its dtype;
2. the assignment is the quantizer's own: C_t loaded into a second index, `probe(X, 1)`, the path training uses; it is
   checked as the float64 argmax (`oracle.check_topk`: a difference must be explained by a near-tie of the scores);
3. the model sums every list's members sequentially in fp32 in ascending sample position, applies the empty-list split
   with its count bookkeeping and normalises with the norm taken in float64;
4. C_{t+1} must agree per component within (ceil(d / 256) + 16) 2^-24 |want| + 2^-149.  Derivation (the full text is
   `ivf_train_model.bound`): the sums and the split are reproduced to the bit, so only the normalisation is bounded:
   ceil(d / 256) strided additions per thread, 8 tree levels and one multiply per term, all terms positive, give the
   squared norm within (ceil(d / 256) + 9) 2^-24, the norm within half of that; the square root and the division add
   at most 2.5 ulp = 5 * 2^-24 each.  One member dropped from a list moves some component by more than 64 bounds
   (tests/test_ivf_train_host.py), typically by thousands;
5. objective[t] must be, to the bit, the sequential float64 sum of the probe's best scores in sample order, and lie
   within nt * 2e-6 of the sum of the float64 best scores.

t = 0 also pins the start: C_0 must be the first nlist sample rows, normalised, within the bound of 4.

What these tests cannot see: a sum taken in another member order, or by float atomics, differs from the sequential
sum by a few of its ulps, which is inside the bound of step 4 more often than not, so it would still pass here;
`test_train_is_deterministic_and_the_objective_does_not_get_worse` (tests/test_ivf_gpu.py) is what covers that.

Measured on one MI355X, the whole test with the 26 (or 6) trainings of its chain and the model on the host:
sampled 1.3 s (seed 3) and 1.0 s (the other seed), whole 0.6 s, split-quantizer 0.2 s, long-rows 0.1 s,
n-equals-nlist 0.02 s, empties 0.05 s; the file 5.3 s with start-up.  The mixtures are stationary from about the sixth
iteration, so the later links of the two full chains re-check the same state; the worst component of any step stood at
0.16 of the bound.
"""
import math

import numpy as np
import pytest
import torch

from oracle import oracle

import ivf_train_model as tm
from tristage_rag_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
STORAGE = {"f32": "f16", "f16": "f16", "bf16": "bf16"}       # the lists' storage; training reads the input dtype


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_chain(case, seed):
    """Checks every step of `case.steps`; returns the split pairs per checked t."""
    x = tm.case_input(case)
    xdev = torch.from_numpy(x).cuda().to(TORCH_DT[case.dtype])
    assert np.array_equal(xdev.float().cpu().numpy(), x)               # the rounding was done on the host: exact
    ids = tm.sample_ids(case.n, case.nlist, seed)
    nt, d, nlist = len(ids), case.d, case.nlist
    X = x[ids]
    Xdev = torch.from_numpy(X).cuda()
    X64 = X.astype(np.float64)

    states = {}

    def state(t):
        if t not in states:
            ivf = IVFFlatIndex(d, nlist, dtype=STORAGE[case.dtype])
            ivf.train(xdev, seed=seed, niter=t)
            states[t] = (ivf.centroids, list(ivf.objective))
            ivf.close()
        return states[t]

    quant = IVFFlatIndex(d, nlist, dtype=STORAGE[case.dtype])
    splits = {}
    for t in case.steps:
        Ct, obj_t = state(t)
        Cn, obj_n = state(t + 1)
        where = f"{case.name} seed={seed} t={t}"
        assert Ct.shape == Cn.shape == (nlist, d) and len(obj_t) == t and len(obj_n) == t + 1, where
        assert np.array_equal(np.array(obj_n[:t]).view(np.uint64), np.array(obj_t).view(np.uint64)), where
        if t == 0:
            ex = tm.excess(Ct, tm.initial(X, nlist), d)
            print(f"{where}: C_0 excess {ex.max():.3f}")
            assert ex.max() <= 1, f"{where}: C_0 is not the normalised head of the sample, list {ex.max(axis=1).argmax()}"
        # the assignment, by the quantizer path that training uses
        quant.set_centroids(Ct)
        assert np.array_equal(bits(quant.centroids), bits(Ct)), f"{where}: the centroids do not round-trip"
        S, L = quant.probe(Xdev, 1)
        S, L = S.cpu().numpy(), L.cpu().numpy()
        swaps = oracle.check_topk(S, L, Ct, X, 1)
        # the update
        want, pairs = tm.step(Ct, X, L[:, 0])
        splits[t] = pairs
        ex = tm.excess(Cn, want, d)
        worst = int(ex.max(axis=1).argmax())
        cnt = np.bincount(L[:, 0], minlength=nlist)
        print(f"{where}: C_{t + 1} excess {ex.max():.3f} (list {worst}, {cnt[worst]} members), "
              f"{len(pairs)} splits, {swaps} near-ties")
        assert ex.max() <= 1, (f"{where}: C_{t + 1} misses the model in list {worst} ({cnt[worst]} members, splits "
                               f"{pairs}): {ex.max():.1f} bounds at dimension {ex[worst].argmax()}")
        # the objective
        seq = float(np.add.accumulate(S[:, 0].astype(np.float64))[-1])
        model = math.fsum((X64 @ Ct.astype(np.float64).T).max(axis=1).tolist())
        print(f"{where}: objective {obj_n[t]!r}, sequential sum {seq!r}, float64 model {model!r}")
        assert np.float64(obj_n[t]).view(np.uint64) == np.float64(seq).view(np.uint64), where
        assert abs(obj_n[t] - model) <= nt * 2e-6, where
    quant.close()
    return splits


@pytest.mark.parametrize("case", [c for c in tm.CASES if c.name != "empties"], ids=lambda c: c.name)
def test_every_training_step_follows_the_model(case):
    run_chain(case, tm.SEED)


def test_every_training_step_follows_the_model_on_another_sample():
    case = tm.CASE["sampled"]
    a, b = tm.sample_ids(case.n, case.nlist, tm.SEED), tm.sample_ids(case.n, case.nlist, tm.OTHER_SEED)
    assert not np.array_equal(a, b) and set(a.tolist()) != set(b.tolist())
    run_chain(case, tm.OTHER_SEED)


def test_empty_lists_are_split_as_the_model_splits_them():
    """Three directions in 100 / 60 / 10 copies on 6 lists: duplicate initial centroids, every tie to the lowest list,
    several empty lists per iteration whose splits halve different lists (the count bookkeeping), and splits of
    lists that were split before."""
    case = tm.CASE["empties"]
    splits = run_chain(case, tm.SEED)
    first = splits[0]
    assert len(first) >= 2 and len({big for _, big in first}) >= 2     # iteration 0 as the host test derived it
    assert any(len(p) > 0 for t, p in splits.items() if t > 0)         # and splits again later in the run
