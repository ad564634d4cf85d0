"""A model of `ts_ivf_train` ("Train."), one k-means iteration at a time.  numpy only: no GPU, no torch.

Training is deterministic, so a fresh index trained with `niter=t` and one trained with `niter=t+1` hold consecutive
states C_t, C_{t+1} of one run.  The model reproduces the step between them from the documented algorithm:

* the sample: a partial Fisher-Yates shuffle of the point ids over nt = min(n, 256 nlist) positions, driven by
  splitmix64 (Steele, Lea, Flood 2014; the public-domain generator of Vigna) seeded with the training seed:
  position i swaps with j = i + z % (n - i).  The sample, in shuffle order, converted to fp32, is X; its first nlist
  rows, normalised, are C_0.
* the update: the fp32 sum of a list's members in ascending sample position (additions only, so it is reproduced to
  the bit by a sequential fp32 accumulation); a list without members keeps its centroid.
* the split: for every list c, ascending, whose count is zero: `big` is the list with the largest count (lowest id on
  ties); c takes big's row times (1 + 1/1024) on even dimensions and (1 - 1/1024) on odd ones, big keeps the row with
  the factors swapped (one fp32 multiply each); then cnt[c] = cnt[big] // 2 and cnt[big] -= cnt[c].
* the normalisation: every row divided by its L2 norm.  The GPU takes the norm in fp32 in a fixed tree order; the
  model takes it in float64 and `bound()` covers the difference.

The assignment is an input of `step()`: the GPU test takes it from the quantizer itself (and checks it against the
float64 argmax), because a whole-run float64 k-means diverges from the fp32 one at the first near-tie.
"""
from collections import namedtuple

import numpy as np

from oracle import oracle

MASK64 = (1 << 64) - 1
TRAIN_PER_LIST = 256            # at most this many training points per list (FAISS max_points_per_centroid)
SPLIT_EPS = np.float32(1.0 / 1024.0)
THREADS = 256                   # the normalisation's workgroup: thread j sums dimensions j, j + 256, ...


# ------------------------------------------------------------------ data
def mixture(n, d, centers=40, seed=0, spread=0.35):
    """Seeded Gaussian mixture on the sphere (float32)."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, centers, n)] + spread * rng.standard_normal((n, d)).astype(np.float32) / np.sqrt(d) * 4
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


Case = namedtuple("Case", "name n d nlist dtype data_seed steps")

FULL = tuple(range(25))         # every link of the shipped 25-iteration run
SPARSE = (0, 1, 2, 24)

CASES = (
    # n > 256 nlist: the cap (nt = 4096); d = 256 + 44: the second stride is partial
    Case("sampled", 4596, 300, 16, "f16", 21, FULL),
    # nt = n: the shuffle runs to the last position; d is less than one stride
    Case("whole", 3000, 64, 40, "bf16", 22, FULL),
    # fp32 training input; 512 < d <= 768 puts the fp32 quantizer on its bf16x3 split scan; exactly three strides
    Case("split-quantizer", 1500, 768, 8, "f32", 23, SPARSE),
    # five strides, the last with 6 live threads
    Case("long-rows", 700, 1030, 5, "f16", 24, SPARSE),
    # every sample point is an initial centroid
    Case("n-equals-nlist", 33, 40, 33, "f16", 25, SPARSE),
    # three directions in 100 / 60 / 10 copies: duplicate initial centroids, exact ties, several empty lists at once
    Case("empties", 170, 128, 6, "f16", 26, SPARSE),
)
CASE = {c.name: c for c in CASES}
SEED = 3
OTHER_SEED = 11                 # the "sampled" case runs with this seed too (another sample)
EMPTIES_COPIES = (100, 60, 10)


def case_input(case):
    """The training input of a case, float32 values already rounded to the case's input dtype."""
    if case.name == "empties":
        dirs = mixture(len(EMPTIES_COPIES), case.d, seed=case.data_seed)
        x = np.concatenate([np.repeat(dirs[i:i + 1], m, axis=0) for i, m in enumerate(EMPTIES_COPIES)])
    else:
        x = mixture(case.n, case.d, seed=case.data_seed)
    assert x.shape == (case.n, case.d)
    return oracle.quantize(x, case.dtype)


# ------------------------------------------------------------------ the sample
def splitmix64(state):
    """One draw: (new state, output), all in integers masked to 64 bits."""
    state = (state + 0x9E3779B97F4A7C15) & MASK64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return state, z ^ (z >> 31)


def sample_size(n, nlist):
    return min(n, TRAIN_PER_LIST * nlist)


def sample_ids(n, nlist, seed, moduli=None):
    """The ids of the training sample in sample order (int64 [nt]).  `moduli`, if a list, receives n - i of every draw."""
    nt = sample_size(n, nlist)
    ids = list(range(n))
    state = seed & MASK64
    for i in range(nt):
        state, z = splitmix64(state)
        if moduli is not None:
            moduli.append(n - i)
        j = i + z % (n - i)
        ids[i], ids[j] = ids[j], ids[i]
    return np.array(ids[:nt], dtype=np.int64)


# ------------------------------------------------------------------ one iteration
def list_sums(C, X, assign):
    """fp32 [nlist, d]: per list the sequential fp32 sum of its members in ascending sample position (a list without
    members keeps its row of C), and the member counts."""
    C = np.asarray(C, dtype=np.float32)
    X = np.asarray(X, dtype=np.float32)
    assign = np.asarray(assign, dtype=np.int64)
    nlist = C.shape[0]
    assert assign.shape == (X.shape[0],) and assign.min() >= 0 and assign.max() < nlist
    cnt = np.bincount(assign, minlength=nlist).astype(np.int64)
    S = C.copy()
    for c in range(nlist):
        members = np.flatnonzero(assign == c)           # ascending
        if len(members):
            S[c] = np.add.accumulate(X[members], axis=0, dtype=np.float32)[-1]
    return S, cnt


def split_empty(S, cnt):
    """The empty-list rule applied to the sums; returns the new fp32 rows and the (empty, big) pairs in order."""
    S = np.array(S, dtype=np.float32)
    cnt = np.array(cnt, dtype=np.int64)
    d = S.shape[1]
    even = (np.arange(d) & 1) == 0
    up, down = np.float32(1.0) + SPLIT_EPS, np.float32(1.0) - SPLIT_EPS
    pairs = []
    for c in range(len(cnt)):
        if cnt[c] != 0:
            continue
        big = int(np.argmax(cnt))                        # the first maximum: lowest id on ties
        v = S[big].copy()
        S[c] = v * np.where(even, up, down).astype(np.float32)
        S[big] = v * np.where(even, down, up).astype(np.float32)
        cnt[c] = cnt[big] // 2
        cnt[big] -= cnt[c]
        pairs.append((c, big))
    return S, pairs


def normalise(S):
    """float64 rows of unit L2 norm (norm in float64); a zero row stays zero."""
    S64 = np.asarray(S, dtype=np.float32).astype(np.float64)
    nrm = np.sqrt((S64 * S64).sum(axis=1, keepdims=True))
    return np.where(nrm > 0, S64 / np.where(nrm > 0, nrm, 1.0), S64)


def initial(X, nlist):
    """C_0 (float64): the first nlist sample points, normalised."""
    return normalise(np.asarray(X, dtype=np.float32)[:nlist])


def step(C, X, assign, drop=None):
    """C_{t+1} (float64 [nlist, d]) from C_t (fp32), the fp32 sample X and its assignment, and the split pairs.

    `drop` = "first" / "last" leaves that member out of every list's sum, as a faulty update kernel would (a list
    whose only member is left out sums to zero); it exists so that the host tests can show what the bound detects."""
    C = np.asarray(C, dtype=np.float32)
    S, cnt = list_sums(C, X, assign)
    if drop is not None:
        assign = np.asarray(assign, dtype=np.int64)
        for c in range(C.shape[0]):
            members = np.flatnonzero(assign == c)
            if len(members):
                kept = members[1:] if drop == "first" else members[:-1]
                S[c] = np.add.accumulate(X[kept], axis=0, dtype=np.float32)[-1] if len(kept) else 0.0
    S, pairs = split_empty(S, cnt)
    return normalise(S), pairs


def assign64(C, X):
    """The float64 argmax of X C^T, ties to the lower list (the model's own assignment, for the host tests)."""
    return np.argmax(np.asarray(X, np.float64) @ np.asarray(C, np.float64).T, axis=1).astype(np.int64)


# ------------------------------------------------------------------ the bound
def bound(want, d):
    """Per component: (ceil(d / 256) + 16) 2^-24 |want| + 2^-149.

    The sums and the split are reproduced exactly, so the only fp32 arithmetic that the model does not reproduce is the
    normalisation.  The squared norm is a sum of positive terms: ceil(d / 256) strided additions per thread, 8 levels
    of the tree over 256 threads and one multiply per term, each within 2^-24 relative, so the squared norm is within
    (ceil(d / 256) + 9) 2^-24 and the norm within half of that.  Then a square root and a division, at most 2.5 ulp
    each even if not correctly rounded, and an ulp is at most 2^-23 relative: 5 * 2^-24 each.  In units of 2^-24:
    (ceil(d / 256) + 9) / 2 + 10 <= ceil(d / 256) + 16 for every d, with at least 1.5 units to spare for the
    second-order terms.  2^-149, the smallest fp32 denormal, covers a component that rounds to zero."""
    strides = -(-d // THREADS)
    return (strides + 16) * 2.0 ** -24 * np.abs(np.asarray(want, dtype=np.float64)) + 2.0 ** -149


def excess(got, want, d):
    """|got - want| / bound, per component (float64): <= 1 passes."""
    got = np.asarray(got, dtype=np.float32).astype(np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return np.abs(got - want) / bound(want, d)
