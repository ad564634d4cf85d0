"""Exactly summable inputs for the stage-1 scans ("exact inputs").

Every generator returns ``(corpus, queries, unit)``: float32 arrays and a power of two of which every product
``c_i * q_i`` is a multiple.  Where ``assert_exactly_summable`` holds, every partial sum of those products, in any
order and over any subset, is an integer below 2^24 times ``unit``, i.e. an fp32 number: a correct kernel returns the
float64 result bit for bit, whatever its accumulation order, and the tests compare with ``np.array_equal``.

The same holds for the bf16x3 split of fp32 storage: the three terms of a value come from
truncation, so they carry its sign, add up to its magnitude and are multiples of the same grid.

Classes (which terms of the split are live):
  ints  dense integers in [-63, 63] on both sides: exact in f16 / bf16 / f32, only hi * hi
  neg   as ints, corpus in [0, 63] and queries in [-63, 0]: every score <= 0
  A     dense 20-bit corpus (hi, mid, lo), few-hot queries from {+-1, +-2, 0.5}
  B     the mirror: few-hot corpus rows, dense 20-bit queries
  C     dense 11-bit corpus (hi, mid), few-hot 11-bit queries: the one class in which mid * mid is live

No GPU is needed here; tests/test_exact_scores_host.py checks the generators and the model, and
tests/test_exact_scores_gpu.py uses them.
"""
import functools

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)

# ---------------------------------------------------------------------------------------------------------- shapes
# One place for the shapes of tests/test_exact_scores_gpu.py; the host test walks the same list.
N_DENSE = 1061                       # 33 row blocks of 32 and a partial one: the dense path
N_FILTER = 32768 + 37                # just above the filter path's floor, a partial last block
N_IVF = 5000
N_SPLIT, B_SPLIT = 257, 33
DENSE_B = (1, 33, 65)
DENSE_K = (1, 100, N_DENSE + 3)
DENSE_D = {"f16": (40, 384, 768, 1024, 1536), "bf16": (40, 384, 768, 1024, 1536),
           "f32": (40, 512, 520, 768, 776, 1024)}      # fp32: both limits of the split (512 < d <= 768) straddled
FILTER_CASES = (("f16", 128, 64), ("f16", 768, 64), ("bf16", 128, 64), ("bf16", 768, 64),
                ("f32", 64, 64),      # exact-f32 kernel, 64 queries per pass
                ("f32", 600, 70))     # split scan, 32 queries per pass: three passes
FILTER_K = (1, 100)
COALESCE_BATCHES, COALESCE_B = 7, 64  # 14 groups of 32: two wide passes of six groups and a partial one
IVF_D = (96, 768)
SPLIT_D = (520, 768)                  # scan_f32s_kernel
EXACT_F32_D = (512, 1024)             # the exact-f32 kernel on the same inputs
ACCURACY_SHAPE = (20_000, 768, 8)     # 3c: the unit-norm data of the other stage-1 tests


def one_launch_rows(num_cus=256):
    """The smallest corpus the one-launch scan takes: one 32-row block per scan wave (7/8 of the CUs, 8 waves each;
    ts_index.hip plan_fused refuses fewer), plus a partial block."""
    return (num_cus - num_cus // 8) * 8 * 32 + 37


def gpu_shapes(num_cus=256):
    """Every (class, n, d, B) the GPU file generates."""
    out = set()
    for cls in ("ints", "neg"):
        for ds in DENSE_D.values():
            out.update((cls, N_DENSE, d, max(DENSE_B)) for d in ds)
        for _, d, B in FILTER_CASES:
            out.add((cls, N_FILTER, d, B))
            out.add((cls, one_launch_rows(num_cus), d, B))
        out.add((cls, N_FILTER, 768, COALESCE_BATCHES * COALESCE_B))
        out.update((cls, n, d, 64) for d in IVF_D for n in (N_IVF, N_FILTER))
    for cls in ("A", "B", "C"):
        out.update((cls, N_SPLIT, d, B_SPLIT) for d in SPLIT_D + EXACT_F32_D)
        out.update((cls, n, d, B_SPLIT) for d in SPLIT_D + EXACT_F32_D for n in (N_FILTER, one_launch_rows(num_cus)))
    return sorted(out)


# ------------------------------------------------------------------------------------------------------ generators
def _few_hot(rows, d, rng, draw):
    """[rows, d] with 1..4 non-zeros per row, each in a different 16-wide k step; row 0 is hot only at k = 0 and
    row 1 only at k = d - 1.  ``draw(size)`` gives the non-zero values."""
    steps = (d + 15) // 16
    most = min(4, steps)
    pick = np.argsort(rng.random((rows, steps)), axis=1)[:, :most]           # distinct k steps per row
    width = np.minimum(16, d - 16 * pick)                                      # the last step may be partial
    k = 16 * pick + rng.integers(0, 16, size=pick.shape) % width
    count = rng.integers(1, most + 1, size=rows)
    vals = np.where(np.arange(most)[None, :] < count[:, None], draw((rows, most)), 0.0)
    out = np.zeros((rows, d), dtype=np.float64)
    np.put_along_axis(out, k, vals, axis=1)
    for r, kk in ((0, 0), (1, d - 1)):
        if r < rows:
            v = out[r][out[r] != 0][0]
            out[r] = 0.0
            out[r, kk] = v
    return out.astype(np.float32)


def _pow2(rng):
    return lambda size: rng.choice(np.array([1.0, -1.0, 2.0, -2.0, 0.5]), size=size)


def _dense_bits(rows, d, rng, bits):
    """Dense signed integers of `bits` magnitude bits (never zero) times 2^-bits: |x| < 1."""
    m = rng.integers(1, 1 << bits, size=(rows, d), dtype=np.int32)
    m *= rng.integers(0, 2, size=(rows, d), dtype=np.int32) * 2 - 1
    return m.astype(np.float32) * np.float32(2.0 ** -bits)


def gen_ints(n, d, B, seed=0):
    rng = np.random.default_rng([seed, 1])
    c = rng.integers(-63, 64, size=(n, d)).astype(np.float32)
    q = rng.integers(-63, 64, size=(B, d)).astype(np.float32)
    return c, q, 1.0


def gen_neg(n, d, B, seed=0):
    rng = np.random.default_rng([seed, 2])
    c = rng.integers(0, 64, size=(n, d)).astype(np.float32)
    q = -rng.integers(0, 64, size=(B, d)).astype(np.float32)
    return c, q, 1.0


def gen_a(n, d, B, seed=0):
    rng = np.random.default_rng([seed, 3])
    return _dense_bits(n, d, rng, 20), _few_hot(B, d, rng, _pow2(rng)), 2.0 ** -21


def gen_b(n, d, B, seed=0):
    rng = np.random.default_rng([seed, 4])
    c = _few_hot(n, d, rng, _pow2(rng))
    return c, _dense_bits(B, d, rng, 20), 2.0 ** -21


def gen_c(n, d, B, seed=0):
    rng = np.random.default_rng([seed, 5])
    draw = lambda size: rng.integers(1, 1 << 11, size=size) * rng.choice([-1.0, 1.0], size=size) * 2.0 ** -11
    return _dense_bits(n, d, rng, 11), _few_hot(B, d, rng, draw), 2.0 ** -22


GENERATORS = {"ints": gen_ints, "neg": gen_neg, "A": gen_a, "B": gen_b, "C": gen_c}


@functools.lru_cache(maxsize=4)
def case(cls, n, d, B, seed=0):
    """``GENERATORS[cls](n, d, B, seed)``, cached and read-only (tests share it)."""
    c, q, unit = GENERATORS[cls](n, d, B, seed)
    c.setflags(write=False)
    q.setflags(write=False)
    return c, q, unit


# ----------------------------------------------------------------------------------------------------------- guard
def exact_scores(corpus, queries):
    """float64 scores [B, n].  For guarded inputs they are integers times ``unit``, far below 2^53: exact."""
    return np.asarray(queries, np.float64) @ np.asarray(corpus, np.float64).T


def assert_exactly_summable(corpus, queries, unit):
    """The condition under which any summation order is exact in fp32: the sum of the products' magnitudes stays
    below 2^24 units, and every score is a multiple of the unit (so is every product, by construction)."""
    c, q = np.asarray(corpus, np.float64), np.asarray(queries, np.float64)
    assert np.log2(unit) == np.rint(np.log2(unit)), "the unit is a power of two"
    top = (np.abs(q) @ np.abs(c).T).max() / unit
    assert top < 2.0 ** 24, f"sum of |c||q| reaches 2^{np.log2(top):.2f} units"
    s = exact_scores(c, q) / unit
    assert np.array_equal(s, np.rint(s)), "a score is not a multiple of the unit"
    # every single product too: both factors lie on power-of-two grids whose product the unit divides
    assert _grid(c) * _grid(q) >= unit, "a product c_i * q_i may fall between multiples of the unit"
    return float(np.log2(max(top, 1.0)))


def _grid(x):
    """The largest power of two of which every entry of x is a multiple."""
    m, e = np.frexp(x[x != 0])
    mi = np.ldexp(m, 53).astype(np.int64)
    low = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)     # trailing zeros of the 53-bit significand
    return 2.0 ** int((e - 53 + low).min())


# ------------------------------------------------------------------------------------------------- expected result
def expected_topk(corpus, queries, k, live=None, allowed=None):
    """Exact top-k: float64 scores, descending, ties by ascending id, padded with -1 / -FLT_MAX.  ``live``: bool [n]
    of rows that exist; ``allowed``: a bool [n] mask, or a list with one mask or None per query."""
    s = exact_scores(corpus, queries)
    B, n = s.shape
    ok = np.ones((B, n), dtype=bool)
    if live is not None:
        ok &= np.asarray(live, bool)[None, :]
    if allowed is not None:
        masks = allowed if isinstance(allowed, (list, tuple)) else [allowed] * B
        assert len(masks) == B
        for b, m in enumerate(masks):
            if m is not None:
                ok[b] &= np.asarray(m, bool)
    s = np.where(ok, s, -np.inf)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]      # stable: equal scores keep ascending ids
    D = np.full((B, k), -FLT_MAX, dtype=np.float32)
    I = np.full((B, k), -1, dtype=np.int64)
    kk = order.shape[1]
    top = np.take_along_axis(s, order, axis=1)
    got = np.isfinite(top)
    D[:, :kk] = np.where(got, top, -FLT_MAX).astype(np.float32)
    I[:, :kk] = np.where(got, order, -1)
    return D, I


# -------------------------------------------------------------------------------- the bf16x3 split
KEPT_TERMS = ("hh", "hm", "mh", "lh", "hl", "mm")     # corpus term, query term
DROPPED_TERMS = ("ml", "lm", "ll")


def _trunc16(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(x):
    """x = hi + mid + lo, each the upper 16 bits of what the terms before it leave (fp32 subtractions, exact)."""
    x = np.ascontiguousarray(x, np.float32)
    hi = _trunc16(x)
    r1 = x - hi
    mid = _trunc16(r1)
    lo = _trunc16(r1 - mid)
    return {"h": hi.astype(np.float64), "m": mid.astype(np.float64), "l": lo.astype(np.float64)}


def split_model(corpus, queries, keep=KEPT_TERMS):
    """Scores [B, n] of the split scan with exact accumulation: the sum of the partial products in ``keep``."""
    a, b = split3(corpus), split3(queries)
    out = np.zeros((np.shape(queries)[0], np.shape(corpus)[0]), dtype=np.float64)
    for t in keep:
        out += b[t[1]] @ a[t[0]].T
    return out


# ------------------------------------------------------------------------------------- 3c: accuracy on unit rows
def accuracy_case():
    from helpers import make_corpus
    n, d, B = ACCURACY_SHAPE
    return make_corpus(n, d, seed=1234, dtype="f32"), make_corpus(B, d, seed=4321, dtype="f32")


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def single_loss_rms(corpus, queries):
    """{term: rms error of the split model without that one kept term}, and the full model's under "none"."""
    ref = exact_scores(corpus, queries)
    out = {"none": rms(split_model(corpus, queries) - ref)}
    for t in KEPT_TERMS:
        out[t] = rms(split_model(corpus, queries, keep=[u for u in KEPT_TERMS if u != t]) - ref)
    return out


def split_rms_threshold(losses):
    """3c's bound: a third of the smallest rms error that losing one kept term causes."""
    return min(v for t, v in losses.items() if t != "none") / 3.0
