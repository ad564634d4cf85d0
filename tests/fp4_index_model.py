"""Host model of the fp4 (OCP e2m1 with one E8M0 scale per 32 elements) stage-1 index, shared by
test_fp4_index_host.py and test_fp4_index_gpu.py.

The format under test is ``index.quantize_rows_mxfp4_reference``.  Here it is restated from its definition with a
brute-force nearest-grid search in float64 (``brute_force_quantize``), and the score error it causes is bounded by a
lemma (``lemma_bound``)."""
import numpy as np

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
MIDPOINTS = (GRID[:-1] + GRID[1:]) / 2.0          # 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5
FLT_MAX = float(np.finfo(np.float32).max)


def block_dims(dpad: int) -> np.ndarray:
    """[dpad // 32, 32]: row 2 g + h lists the dimensions 64 g + 16 m + 8 h + j of scale block (g, h), written out."""
    out = np.zeros((dpad // 32, 32), dtype=np.int64)
    for g in range(dpad // 64):
        for h in range(2):
            out[2 * g + h] = [64 * g + 16 * m + 8 * h + j for m in range(4) for j in range(8)]
    assert np.array_equal(np.sort(out.reshape(-1)), np.arange(dpad))
    return out


def _clean64(x) -> np.ndarray:
    """float32 input -> float64 with NaN as 0 and +-Inf as +-FLT_MAX."""
    v = np.asarray(x, dtype=np.float32).astype(np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(v, -FLT_MAX, FLT_MAX)


def brute_force_block(vals) -> tuple:
    """One scale block (32 float32 values) -> (codes [32], e), from the definition, in float64 and Python integers."""
    v = _clean64(vals)
    sign = np.signbit(np.where(np.isnan(np.asarray(vals, dtype=np.float32)), 0.0, np.asarray(vals, dtype=np.float32)))
    amax = float(np.abs(v).max())
    if amax == 0.0:
        e = 0
    else:
        fl = int(np.floor(np.log2(amax)))
        while 2.0 ** (fl + 1) <= amax:         # (log2 in float64 may be one off just below a power of two)
            fl += 1
        while 2.0 ** fl > amax:
            fl -= 1
        e = fl - 2
        if amax > 6.0 * 2.0 ** e:
            e += 1
        e = max(-100, min(100, e))
    y = np.abs(v) / 2.0 ** e                   # exact in float64: a float32 value times a power of two
    codes = np.zeros(32, dtype=np.uint8)
    for i, t in enumerate(y):
        dist = np.abs(GRID - min(t, 8.0))
        best = np.flatnonzero(dist == dist.min())
        idx = int(best[0]) if len(best) == 1 else int(best[0] if best[0] % 2 == 0 else best[1])
        codes[i] = idx | (8 if sign[i] else 0)
    return codes, e


def brute_force_quantize(x) -> tuple:
    """x [n, d] -> (codes uint8 [n, dpad], exps int8 [n, dpad // 32]) by brute_force_block, block by block."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    dpad = -(-d // 64) * 64
    v = np.zeros((n, dpad), dtype=np.float32)
    v[:, :d] = x
    dims = block_dims(dpad)
    codes = np.zeros((n, dpad), dtype=np.uint8)
    exps = np.zeros((n, dpad // 32), dtype=np.int8)
    for r in range(n):
        for b in range(dpad // 32):
            c, e = brute_force_block(v[r, dims[b]])
            codes[r, dims[b]] = c
            exps[r, b] = e
    return codes, exps


def decode64(codes, exps, d: int) -> np.ndarray:
    """sign * grid * 2^e in float64, [n, d]."""
    codes = np.asarray(codes)
    n, dpad = codes.shape
    dims = block_dims(dpad)
    out = np.zeros((n, dpad))
    for b in range(dpad // 32):
        c = codes[:, dims[b]]
        out[:, dims[b]] = np.where(c & 8, -1.0, 1.0) * GRID[c & 7] * 2.0 ** np.asarray(exps)[:, b:b + 1].astype(np.float64)
    return out[:, :d]


def block_with(values, fill=0.0) -> np.ndarray:
    """A [1, 64] row whose scale block (0, 0) holds `values` (at most 32) and `fill` elsewhere; block (0, 1) is zero."""
    row = np.zeros((1, 64), dtype=np.float32)
    dims = block_dims(64)[0]
    row[0, dims] = fill
    row[0, dims[:len(values)]] = np.asarray(values, dtype=np.float32)
    return row


def midpoint_rows(e: int) -> np.ndarray:
    """Rows whose first scale block has amax = 6 * 2^e exactly (so its exponent is e) and holds one midpoint times 2^e
    with both float32 neighbours, in both signs."""
    rows = []
    for m in MIDPOINTS:
        x = np.float32(m * 2.0 ** e)
        assert float(x) == m * 2.0 ** e
        trio = [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(0))]
        vals = [np.float32(6.0 * 2.0 ** e)] + trio + [-t for t in trio]
        rows.append(block_with(vals))
    return np.concatenate(rows)


def amax_rows(e: int) -> np.ndarray:
    """amax exactly 6 * 2^e, its float32 neighbours, and the powers of two around it, with smaller values beside."""
    six = np.float32(6.0 * 2.0 ** e)
    tops = [six, np.nextafter(six, np.float32(np.inf)), np.nextafter(six, np.float32(0)),
            np.float32(4.0 * 2.0 ** e), np.nextafter(np.float32(4.0 * 2.0 ** e), np.float32(0)),
            np.float32(8.0 * 2.0 ** e), np.nextafter(np.float32(8.0 * 2.0 ** e), np.float32(0))]
    rows = []
    for t in tops:
        for sgn in (1.0, -1.0):
            rows.append(block_with([sgn * t, 0.3 * t, -0.51 * t, 0.126 * t, 0.9 * t, -0.04 * t]))
    return np.concatenate(rows)


def special_rows() -> np.ndarray:
    rows = [block_with([]), block_with([-0.0, 0.0]), block_with([np.nan]), block_with([np.nan, 1.0, -np.nan]),
            block_with([np.inf, 1.0]), block_with([-np.inf, 1e38, -1e30]), block_with([2.0 ** -120, 2.0 ** -121, -2.0 ** -122]),
            block_with([2.0 ** 120, -2.0 ** 118, 1.0]), block_with([1e-45, -1e-45, 1e-40]), block_with([2.0 ** -126]),
            block_with([2.0 ** -98, 2.0 ** -99, 1.5 * 2.0 ** -100, 2.0 ** -102]),      # around the lower clamp
            block_with([2.0 ** 102.5, 2.0 ** 101, -2.0 ** 104]),                       # around the upper clamp
            block_with([FLT_MAX, -FLT_MAX, 1.0]), block_with([1.0] * 32), block_with([-3.0] * 32)]
    return np.concatenate(rows)


def unit_rows(n: int, d: int, seed: int) -> np.ndarray:
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d), dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def wide_rows(n: int, d: int, seed: int) -> np.ndarray:
    """Unit rows times magnitudes from 2^-30 to 2^30, with zero blocks, zeros, infinities, a NaN and huge values."""
    g = np.random.default_rng(seed)
    x = unit_rows(n, d, seed) * np.exp2(g.integers(-30, 31, size=(n, 1))).astype(np.float32)
    x *= np.exp2(g.integers(-3, 4, size=(n, d))).astype(np.float32)         # a spread inside the blocks too
    x[0, :5] = [0.0, -0.0, np.inf, -np.inf, np.nan]
    if n > 2:
        x[1, :3] = [1e30, -1e30, 2.0 ** -120]
        x[2] = 0.0
    return x.astype(np.float32)


def deltas(x) -> np.ndarray:
    """Per element, the largest |decode(x) - x|: half the grid step at |x| / 2^e, times 2^e: 2^e * {0.25 below 2, 0.5
    below 4, else 1} (no element saturates: |x| / 2^e <= 6).  float64 [n, d]."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    dpad = -(-d // 64) * 64
    dims = block_dims(dpad)
    exps = model_exponents(x)
    s = np.zeros((n, dpad))
    for b in range(dpad // 32):
        s[:, dims[b]] = 2.0 ** exps[:, b:b + 1].astype(np.float64)
    s = s[:, :d]
    y = np.abs(x.astype(np.float64)) / s
    return s * np.where(y < 2, 0.25, np.where(y < 4, 0.5, 1.0))


def model_exponents(x) -> np.ndarray:
    """The block exponents [n, dpad // 32] from the definition, in float64, whole arrays at a time (what
    brute_force_block does for one block; independent of the code under test)."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    dpad = -(-d // 64) * 64
    v = np.zeros((n, dpad))
    v[:, :d] = _clean64(x)
    amax = np.abs(v[:, block_dims(dpad)]).max(axis=2)
    safe = np.where(amax == 0, 1.0, amax)
    fl = np.floor(np.log2(safe))
    fl = np.where(2.0 ** (fl + 1) <= safe, fl + 1, fl)      # (log2 in float64 may be one off beside a power of two)
    fl = np.where(2.0 ** fl > safe, fl - 1, fl)
    assert ((2.0 ** fl <= safe) & (safe < 2.0 ** (fl + 1))).all()
    e = fl - 2
    e = np.clip(e + (safe > 6.0 * 2.0 ** e), -100, 100)
    return np.where(amax == 0, 0, e).astype(np.int8)


def lemma_bound(q, x) -> np.ndarray:
    """|q . decode(quantise(x)) - q . x| <= sum_i |q_i| delta_i, per (query, row), in float64."""
    return np.abs(np.asarray(q, dtype=np.float64)) @ deltas(x).T


def clamp_queries(q: np.ndarray) -> np.ndarray:
    """Magnitudes into [2^-20, 1], signs kept: no product of a query element with a decoded element is subnormal."""
    mag = np.clip(np.abs(q), 2.0 ** -20, 1.0)
    return (np.where(np.signbit(q), -mag, mag)).astype(np.float32)


def to_bf16_f32(q: np.ndarray) -> np.ndarray:
    """float32 -> bf16 (round to nearest even) -> float32, in integer arithmetic."""
    u = np.ascontiguousarray(q, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def planted_case(n: int = 40_000, d: int = 64, nq: int = 4, per_query: int = 20, seed: int = 71):
    """Gaussian unit rows with, per query, `per_query` planted rows of cosine 0.90 .. 0.99 to it.
    Returns (queries [nq, d], rows [n, d], planted [nq, per_query] sorted row ids)."""
    g = np.random.default_rng(seed)
    q = unit_rows(nq, d, seed + 1)
    rows = unit_rows(n, d, seed + 2)
    ids = np.sort(g.choice(n, size=nq * per_query, replace=False)).reshape(per_query, nq).T.copy()
    cos = np.linspace(0.90, 0.99, per_query)
    for j in range(nq):
        q64 = q[j].astype(np.float64)
        noise = unit_rows(per_query, d, seed + 10 + j).astype(np.float64)
        noise -= (noise @ q64)[:, None] * q64
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        rows[ids[j]] = (cos[:, None] * q64 + np.sqrt(1 - cos ** 2)[:, None] * noise).astype(np.float32)
    return q, rows, ids
