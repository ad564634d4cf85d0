"""Host model of the fp8 (e4m3) stage-1 index, shared by test_fp8_index_host.py and test_fp8_index_gpu.py.

The format under test is ``index.quantize_rows_e4m3_fixed_reference``: element x -> e4m3fn_rne(x * 2^s), one scale
exponent s per index.  Here it is checked against a brute-force search over the table of finite e4m3 values, and the
score error it causes is bounded by a lemma (``lemma_bound``)."""
import numpy as np


def e4m3_table() -> np.ndarray:
    """float64 value of every byte (NaN for 0x7F / 0xFF), from the format's definition: 1 sign, 4 exponent bits
    (bias 7), 3 mantissa bits, subnormals at exponent 0, no infinities."""
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    v = np.where((b & 0x7F) == 0x7F, np.nan, v)
    return np.where(b & 0x80, -v, v)


TABLE = e4m3_table()
POS_BYTES = np.arange(0x7F)                 # 0x00 .. 0x7E: +0, the subnormals, the normals up to 448
POS_VALUES = TABLE[:0x7F]                   # ascending
assert POS_VALUES[-1] == 448.0 and len(set(TABLE[np.isfinite(TABLE)])) == 253


def brute_force_quantize(x, s: int) -> np.ndarray:
    """Nearest of the 253 finite e4m3 values to x * 2^s (exact in float64), ties to the even mantissa; above 448 and
    +-Inf: +-448; NaN: 0x7F; the sign bit of x is kept (also where the result is zero)."""
    x = np.asarray(x, dtype=np.float32)
    y = np.abs(x.astype(np.float64)) * 2.0 ** s
    out = np.empty(x.shape, dtype=np.uint8)
    flat_y, flat_o = y.reshape(-1), out.reshape(-1)
    neg = np.signbit(x).reshape(-1)
    for i, v in enumerate(flat_y):
        if np.isnan(v):
            flat_o[i] = 0x7F
            continue
        dist = np.abs(POS_VALUES - min(v, 1024.0))   # (far above 448 float64 could no longer tell the distances apart)
        best = np.flatnonzero(dist == dist.min())
        if len(best) == 2:                  # a tie between neighbours: the even byte has the even mantissa
            byte = int(best[0] if best[0] % 2 == 0 else best[1])
        else:
            byte = int(best[0])
        flat_o[i] = byte | (0x80 if neg[i] else 0)
    return out


def midpoint_inputs(s: int) -> np.ndarray:
    """float32 inputs x whose x * 2^s is the midpoint of two consecutive representable magnitudes (and the midpoint
    between 448 and the 480 that does not exist), with both float32 neighbours, both signs."""
    mids = (POS_VALUES[:-1] + POS_VALUES[1:]) / 2.0
    mids = np.concatenate([mids, [464.0]])
    x = (mids * 2.0 ** -s).astype(np.float32)
    assert (x.astype(np.float64) * 2.0 ** s == mids).all()          # the midpoints are exact float32 inputs
    trio = np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))])
    return np.concatenate([trio, -trio])


def special_inputs(s: int) -> np.ndarray:
    sc = 2.0 ** -s
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, 448 * sc, 449 * sc, 463.9 * sc, 464 * sc, 480 * sc, 1e30, -1e30, 3.4e38,
         2.0 ** -9 * sc, 2.0 ** -10 * sc, 2.0 ** -11 * sc, 1.5 * 2.0 ** -9 * sc, 7 * 2.0 ** -9 * sc, 7.5 * 2.0 ** -9 * sc,
         2.0 ** -6 * sc, 1e-30, 1e-45, -1e-45, 2.0 ** -126, 1.0, -1.0, 0.3, -0.7]
    v += list(POS_VALUES * sc) + list(-POS_VALUES * sc)
    return np.array(v, dtype=np.float32)


def unit_rows(n: int, d: int, seed: int) -> np.ndarray:
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d), dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def lemma_bound(q, x, s: int) -> np.ndarray:
    """|q . decode(quantise(x)) - q . x| <= 2^-4 sum|q_i x_i| + 2^-(10+s) sum|q_i|, per (query, row), in float64.
    An element whose x * 2^s is an e4m3 normal (no saturation: |x * 2^s| <= 448) moves by at most half an ulp of a
    3-bit mantissa, 2^-4 of itself; one in the subnormal range by at most half the step 2^-9, which is 2^-(10+s) of
    the unscaled value."""
    q, x = np.asarray(q, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return 2.0 ** -4 * (np.abs(q) @ np.abs(x).T) + 2.0 ** -(10 + s) * np.abs(q).sum(axis=1, keepdims=True)


def clamp_queries(q: np.ndarray) -> np.ndarray:
    """Magnitudes into [2^-20, 1], signs kept: no product of a query element with a decoded element is subnormal."""
    mag = np.clip(np.abs(q), 2.0 ** -20, 1.0)
    return (np.where(np.signbit(q), -mag, mag)).astype(np.float32)


def to_bf16_f32(q: np.ndarray) -> np.ndarray:
    """float32 -> bf16 (round to nearest even) -> float32, in integer arithmetic."""
    u = np.ascontiguousarray(q, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)
