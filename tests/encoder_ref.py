"""Float64 references of the encoder-forward kernels (ts_fwd.hip, ts_linear.hip, ts_mlp.hip), each with an ELEMENTWISE
error bound derived from the kernel's arithmetic.  A plain helper module (no fixtures), usable on any torch device.

Conventions:
  * the kernels round to a 16-bit type at fixed points (the projection's output, the GELU's output, the final copy).
    The reference rounds its float64 value at the same points (``round16``), and where the kernel's own pre-rounding
    error could carry the value across a rounding boundary the bound says so: a 16-bit result is a ``Ref16`` — the
    float64 value rounded once, plus the interval ``[lo, hi]`` of 16-bit values the kernel may legitimately produce,
    ``lo = round16(z - e)``, ``hi = round16(z + e)`` for the pre-rounding value ``z`` and its error bound ``e``.
    Rounding is monotonic, so the kernel's result lies in that interval whenever its pre-rounding error is within
    ``e``.  Where ``e`` cannot move the value out of its rounding cell the interval is a single value: bit-exact.
  * a fp32 result is an ``Ref32``: the float64 value and an absolute per-element bound.
  * unit roundoff of fp32 with round-to-nearest: U = 2^-24.  Matrix-core accumulation is given 2 U per addition
    (``UM``): it also covers an accumulator that truncates instead of rounding.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

U = 2.0 ** -24          # fp32 unit roundoff (round to nearest)
UM = 2.0 ** -23         # per addition of a matrix-core fp32 accumulation (round to nearest or toward zero)
GELU_DMAX = 1.1289      # max |gelu'(u)| over the reals (at u = +-sqrt(2))
GELU_ARGMIN = -0.7517916  # gelu's minimum

_FMT = {  # precision bits (with the implicit one), smallest normal exponent, largest finite value
    torch.bfloat16: (8, -126, float.fromhex("0x1.fep127")),
    torch.float16: (11, -14, 65504.0),
}


def fmt_of(dt):
    if dt in ("bf16", torch.bfloat16):
        return torch.bfloat16
    if dt in ("f16", "fp16", torch.float16):
        return torch.float16
    raise ValueError(dt)


def _pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k exactly, as float64, for integers -1022 <= k <= 1023: the exponent field written directly (torch.ldexp may
    form 2^k in float32, and pow on a GPU need not be exact)."""
    return ((k.to(torch.int64) + 1023) << 52).view(torch.float64)


def round16(x: torch.Tensor, dt) -> torch.Tensor:
    """float64 -> the nearest value of the 16-bit type (ties to even, overflow to +-inf, gradual underflow), as float64.
    One rounding: torch's float64 -> bfloat16 cast goes through float32 and may round twice."""
    p, emin, vmax = _FMT[fmt_of(dt)]
    x = x.to(torch.float64)
    _, e = torch.frexp(x)                                   # |x| = m 2^e, m in [0.5, 1)
    q = _pow2(torch.clamp(e - 1, min=emin) - (p - 1))
    r = torch.round(x / q) * q                              # (torch.round: half to even)
    r = torch.where(r.abs() > vmax, torch.copysign(torch.full_like(r, math.inf), x), r)
    return torch.where(torch.isfinite(x), r, x)


def ulp16(x: torch.Tensor, dt) -> torch.Tensor:
    """Spacing of the 16-bit type at |x| (the subnormal spacing below the smallest normal)."""
    p, emin, _ = _FMT[fmt_of(dt)]
    x = x.to(torch.float64)
    _, e = torch.frexp(x)
    e = torch.where(x == 0, torch.full_like(e, emin + 1), e)
    return _pow2(torch.clamp(e - 1, min=emin) - (p - 1))


@dataclass
class Ref16:
    value: torch.Tensor     # float64 reference rounded once to the 16-bit type
    lo: torch.Tensor        # the interval of 16-bit results the kernel's arithmetic allows (float64)
    hi: torch.Tensor


@dataclass
class Ref32:
    value: torch.Tensor     # float64 reference
    bound: torch.Tensor     # absolute, per element


def interval16(z: torch.Tensor, e: torch.Tensor, dt) -> Ref16:
    """A value computed as ``z`` with absolute error at most ``e`` and then rounded to the 16-bit type."""
    return Ref16(round16(z, dt), round16(z - e, dt), round16(z + e, dt))


def half_width(r: Ref16) -> torch.Tensor:
    """Largest distance from the reference to an end of its interval (inf where an end overflows)."""
    return torch.maximum(r.value - r.lo, r.hi - r.value).nan_to_num(nan=0.0)


# ---------------------------------------------------------------------------------------------------------------- GELU
def gelu64(u: torch.Tensor) -> torch.Tensor:
    u = u.to(torch.float64)
    return 0.5 * u * (1.0 + torch.special.erf(u / math.sqrt(2.0)))


def gelu_formula_error(u: torch.Tensor) -> torch.Tensor:
    """Bound on |gelu32(u) - gelu(u)| for the fp32 formula ``(u * 0.5) * (1 + erf(u / sqrt 2))`` of the kernels.

    The erf is either the device libm's erff (ts_geglu) or Abramowitz & Stegun 7.1.26 (fs_erf: |approximation error|
    < 1.5e-7) evaluated with fp32 fmas, the approximate v_rcp_f32 and v_exp_f32 (about 1 ulp each): its absolute
    error is below 1.5e-7 + 5 U < 4.5e-7.  ``1 + erf`` adds no error of its own for erf <= -0.5 (Sterbenz) and at
    most U elsewhere, and the factor 0.5 |u| scales the erf error to at most 2.25e-7 |u| < |u| 2^-22 — the floor that
    the cancellation of ``1 + erf`` for negative u leaves: as |gelu(u)| falls towards zero the error stays near
    0.5 |u| times the erf error, which torch's own fp32 formula has as well.  The two products and the scaling add at
    most 3 U relative: 2^-22 |gelu(u)|.  Infinite inputs: inf for +inf, nan for -inf (-inf * 0), like torch."""
    u = u.to(torch.float64)
    return (u.abs() + gelu64(u).abs()) * 2.0 ** -22


def gelu_ref(u: Ref16, dt) -> Ref16:
    """round16(gelu32(u')) for a 16-bit input u' anywhere in ``u``'s interval: the reference is round16(gelu(u.value));
    the interval spans gelu over [u.lo, u.hi] (gelu is monotonic except around its minimum, taken where it falls
    inside) widened by ``gelu_formula_error``."""
    g0, g1, gv = gelu64(u.lo), gelu64(u.hi), gelu64(u.value)
    gmin = torch.minimum(g0, g1)
    inside = (u.lo < GELU_ARGMIN) & (u.hi > GELU_ARGMIN)
    gmin = torch.where(inside, torch.full_like(gmin, float(gelu64(torch.tensor(GELU_ARGMIN, dtype=torch.float64)))), gmin)
    gmax = torch.maximum(g0, g1)
    f = torch.maximum(gelu_formula_error(u.lo), gelu_formula_error(u.hi))
    f = torch.where(torch.isfinite(f), f, torch.zeros_like(f))   # (an infinite input has an exact result: inf or nan)
    return Ref16(round16(gv, dt), round16(gmin - f, dt), round16(gmax + f, dt))


def exact16(x: torch.Tensor) -> Ref16:
    """A 16-bit input as a degenerate interval."""
    v = x.to(torch.float64)
    return Ref16(v, v, v)


# -------------------------------------------------------------------------------------------------------------- linear
def linear_ref(x: Ref16, w: torch.Tensor, b, dt) -> Ref16:
    """round16(x W^T + b) of the streamed-weight kernels (ffn_stream_kernel, proj_ln_kernel, mlp_ln_kernel).

    The products of 16-bit values are exact in fp32; the matrix cores add them in fp32.  Any order of n additions of
    terms whose absolute values sum to S errs by at most (n - 1) UM S; the bias is one more fp32 addition: UM (S + |b|).
    n counts the NONZERO products of an output (adding an exact zero is exact): an identity weight reproduces x exactly.
    If ``x`` is itself an interval (the GELU'd intermediate of the MLP, the staged rows of proj_ln with GELU_IN),
    sum_k max(x.hi - x, x - x.lo)_k |w_k| is added: the rounded inputs' own allowance carried through W."""
    w64 = w.to(torch.float64)
    xv = x.value
    xa = torch.maximum(xv.abs(), torch.maximum(x.lo.abs(), x.hi.abs()))
    z = xv @ w64.T
    s = xa @ w64.abs().T
    n = (xa != 0).to(torch.float64) @ (w64 != 0).to(torch.float64).T
    adds = torch.clamp(n - 1, min=0)
    if b is not None:
        b64 = b.to(torch.float64)
        z = z + b64
        s = s + b64.abs()
        adds = adds + 1
    e = adds * UM * s
    dx = half_width(x)
    if bool((dx > 0).any()):
        e = e + dx @ w64.abs().T
    return interval16(z, e, dt)


def linear_gelu_ref(x: Ref16, w, b, dt) -> Ref16:
    """round16(gelu32(round16(x W^T + b))): the projection's rounding, then the GELU's."""
    return gelu_ref(linear_ref(x, w, b, dt), dt)


# ----------------------------------------------------------------------------------------------------------- LayerNorm
def ln_shape(H: int):
    """(NCH, LPR) of ts_fwd.hip's ln_launch: 4-element chunks per lane and lanes per row."""
    q = H // 4
    if q <= 96:
        nch = (q + 31) // 32
        return (1 if nch <= 1 else 2 if nch <= 2 else 3), 32
    nch = (q + 63) // 64
    return (2 if nch <= 2 else 3 if nch <= 3 else 4 if nch <= 4 else 8), 64


def ln_depth(nch: int, lpr: int) -> int:
    """Additions on the longest path of ln_row's sums: a chunk's ((a + b) + (c + d)), NCH chunks in sequence, then a
    butterfly over the LPR lanes."""
    return 2 + nch + int(math.log2(lpr))


def layernorm_ref(v: torch.Tensor, dv, gamma, beta, eps: float, depth: int) -> Ref32:
    """y = (v - mean) rstd gamma + beta of ln_row (two-pass mean / variance in fp32, ts_ln_dev.h), v float64 [rows, H],
    ``dv`` a per-element bound on |v' - v| for the fp32 row v' the kernel actually holds (0 when it holds v exactly).

    With d = v - mean, var = sum(d^2) / H, r = (var + eps)^-1/2, first order in every error:
      mean:  e_mean = sum(dv) / H + depth U sum|v| / H + U |mean|            (inputs; the sum's additions; the division)
      sum of squares: sum((d + eps_i - delta)^2) - sum(d^2) = 2 sum(d eps_i) + sum((eps_i - delta)^2) since sum(d) = 0, so
             e_S = 2 sum|d| dv + sum((dv + e_mean)^2) + (depth + 3) U sum(d^2)   (+ the subtraction, square, sum roundings)
      var' + eps: e_var = e_S / H + U var + U (var + eps)
      rstd (sqrt and reciprocal, ~1 ulp each): relative e_r = e_var / (2 (var + eps)) + 4 U
      y:     |gamma| r (dv + e_mean) + |gamma d| r e_r + 4 U (|gamma d r| + |beta|)   (the last: the output's products
             and sum, with or without fused multiply-adds)"""
    v = v.to(torch.float64)
    H = v.shape[-1]
    dv = torch.zeros_like(v) if dv is None else torch.broadcast_to(dv.to(torch.float64), v.shape)
    eps = float(torch.tensor(eps, dtype=torch.float32))
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    g = gamma.to(torch.float64)
    bt = beta.to(torch.float64) if beta is not None else torch.zeros_like(g)
    y = d * r * g + bt
    e_mean = dv.sum(-1, keepdim=True) / H + depth * U * v.abs().sum(-1, keepdim=True) / H + U * mean.abs()
    e_s = (2 * (d.abs() * dv).sum(-1, keepdim=True) + ((dv + e_mean) ** 2).sum(-1, keepdim=True)
           + (depth + 3) * U * (d * d).sum(-1, keepdim=True))
    e_var = e_s / H + U * var + U * (var + eps)
    e_r = e_var / (2 * (var + eps)) + 4 * U
    bound = g.abs() * r * (dv + e_mean) + (g * d).abs() * r * e_r + 4 * U * ((g * d * r).abs() + bt.abs())
    return Ref32(y, bound)


def to16(y: Ref32, dt) -> Ref16:
    """The 16-bit copy of a fp32 result (ln_pack2: one rounding of the fp32 value)."""
    return interval16(y.value, y.bound, dt)


def add_layernorm_ref(x, res, gamma, beta, eps: float, prenorm: bool = False):
    """ts_add_layernorm / ts_add_prenorm: v = x + res in fp32 (one rounding when there is a residual; x of any input
    type is exact in fp32).  Returns (fp32 output, its LayerNorm) — the fp32 output is v itself under prenorm."""
    H = x.shape[-1]
    v = x.to(torch.float64) + (res.to(torch.float64) if res is not None else 0.0)
    dv = U * v.abs() if res is not None else None
    y = layernorm_ref(v, dv, gamma, beta, eps, ln_depth(*ln_shape(H)))
    if prenorm:
        return Ref32(v, dv if dv is not None else torch.zeros_like(v)), y
    return y, y


def embed_layernorm_ref(ids, pos_ids, type_ids, word, pos, typ, gamma, beta, eps: float) -> Ref32:
    """ts_embed_layernorm: v = (word[ids] + type[tt]) + pos[p], two fp32 additions (type 0 when type_ids is None)."""
    w = word.to(torch.float64)[ids]
    t = typ.to(torch.float64)[type_ids if type_ids is not None else torch.zeros_like(ids)]
    wt = w + t
    v = wt + pos.to(torch.float64)[pos_ids]
    dv = U * wt.abs() * 2 + U * v.abs()
    H = v.shape[-1]
    return layernorm_ref(v.reshape(-1, H), dv.reshape(-1, H), gamma, beta, eps, ln_depth(*ln_shape(H)))


def proj_ln_ref(x: torch.Tensor, w, b, res, gamma, beta, eps: float, dt, gelu_in: bool = False, depth: int = 10) -> Ref32:
    """proj_ln_kernel (ts_linear_add_layernorm): LayerNorm(round16(x' W^T + b) + res), x' = x or round16(gelu(x)) when
    GELU_IN.  The staged projection output may sit anywhere in its interval: that allowance is the LayerNorm's input
    error dv (plus the fp32 rounding of the residual add).  ln_row<3, 32>: depth 10."""
    xin = gelu_ref(exact16(x), dt) if gelu_in else exact16(x)
    return _ln_of_projection(linear_ref(xin, w, b, dt), res, gamma, beta, eps, depth)


def _ln_of_projection(p: Ref16, res, gamma, beta, eps, depth) -> Ref32:
    v = p.value + (res.to(torch.float64) if res is not None else 0.0)
    dp = half_width(p)
    dv = dp + (U * (v.abs() + dp) if res is not None else 0.0)
    return layernorm_ref(v, dv, gamma, beta, eps, depth)


def mlp_ref(x, w1, b1, w2, b2, res, gamma, beta, eps: float, dt) -> Ref32:
    """mlp_ln_kernel (ts_mlp_add_layernorm): LayerNorm(round16(round16(gelu(round16(x W1^T + b1))) W2^T + b2) + res).
    The intermediate's interval is carried through W2 (linear_ref), the output projection's through the LayerNorm."""
    a = linear_gelu_ref(exact16(x), w1, b1, dt)
    return _ln_of_projection(linear_ref(a, w2, b2, dt), res, gamma, beta, eps, 10)


# ------------------------------------------------------------------------------------------------ rotary, gated GELU
def rope_ref(x: torch.Tensor, cos, sin, dt) -> Ref16:
    """transformers' apply_rotary_pos_emb on x [..., L, dh] (16-bit), tables [L, dh] fp32: x cos + rotate_half(x) sin,
    the two fp32 products and their sum each rounded (no fused multiply-add): error <= 2 U (|x cos| + |x' sin|)."""
    xv = x.to(torch.float64)
    half = x.shape[-1] // 2
    rot = torch.cat([-xv[..., half:], xv[..., :half]], -1)
    c, s = cos.to(torch.float64), sin.to(torch.float64)
    a, bb = xv * c, rot * s
    return interval16(a + bb, 2 * U * (a.abs() + bb.abs()), dt)


def geglu_ref(u: torch.Tensor, dt) -> Ref16:
    """ts_geglu: round16(round16(gelu(a)) * gate), u = [a, gate].  The product of two 16-bit values is exact in fp32
    (16 or 22 significant bits), so the only allowance is the GELU's interval, scaled by the gate."""
    I = u.shape[-1] // 2
    a = gelu_ref(exact16(u[..., :I]), dt)
    g = u[..., I:].to(torch.float64)
    p0, p1 = a.lo * g, a.hi * g
    return Ref16(round16(a.value * g, dt), round16(torch.minimum(p0, p1), dt), round16(torch.maximum(p0, p1), dt))


# ----------------------------------------------------------------------------------------------------------- attention
def attention_ref(q, k, v, lens, scale: float, dt, window: int = 0) -> Ref16:
    """attn_varlen_kernel: softmax(q k^T scale) v over each sequence's first lens[b] keys (|query - key| <= window when
    window > 0), q / k / v [B, heads, L, dh] 16-bit (already rotated when the kernel applies rope).  Output [B, heads, L, dh].

    The kernel: s' = q.k on the matrix cores (error UM (dh - 1) sum|q k|), t = s' c2 in base 2, running max m, e = exp2(t - m)
    (v_exp_f32, ~1 ulp; argument error c2 |s' - s| + 2 U (|t| + |m|)), P = round16(e) for the second product (relative
    2^-8 bf16 / 2^-11 fp16, plus fp16's subnormal spacing 2^-25 below 2^-14), l = sum e in fp32, O = (V^T P) / l.
    With p = e / l and O = sum p v:
      |O' - O| <= (eps16 + 2 eps_e + (n + 2 tiles + 2) UM) sum p |v| + (eps_e + (n + 2 tiles) UM) |O| + n sub / l max|v|
    where eps_e = ln 2 (c2 max|s' - s| + 2 U (max|t| + max|m|)) + 2 U bounds the relative error of each e (and of each
    rescale factor, one per key tile), n = keys seen.  Then the output is rounded once."""
    B, nh, L, dh = q.shape
    q64, k64, v64 = (t.to(torch.float64) for t in (q, k, v))
    s = torch.einsum("bhqd,bhkd->bhqk", q64, k64)
    sa = torch.einsum("bhqd,bhkd->bhqk", q64.abs(), k64.abs())
    pos = torch.arange(L, device=q.device)
    valid = pos[None, :] < lens.to(q.device)[:, None]                       # [B, L]
    mask = valid[:, None, None, :].expand(B, nh, L, L)
    if window > 0:
        mask = mask & ((pos[:, None] - pos[None, :]).abs() <= window)[None, None]
    s = s * scale
    sm = s.masked_fill(~mask, -math.inf)
    mx = sm.amax(-1, keepdim=True)
    e = torch.exp(sm - mx)
    l = e.sum(-1, keepdim=True)
    p = e / l
    o = p @ v64
    pv = p @ v64.abs()
    c2 = scale / math.log(2.0)
    ds = UM * (dh - 1) * sa.masked_fill(~mask, 0).amax(-1, keepdim=True)
    tmax = (sm * c2).abs().masked_fill(~mask, 0).amax(-1, keepdim=True)
    eps_e = math.log(2.0) * (c2 * ds + 2 * U * 2 * tmax) + 2 * U
    n = mask.sum(-1, keepdim=True).to(torch.float64)
    tiles = (L + 31) // 32
    eps16 = 2.0 ** -8 if fmt_of(dt) == torch.bfloat16 else 2.0 ** -11
    sub = 0.0 if fmt_of(dt) == torch.bfloat16 else 2.0 ** -25
    vmax = v64.abs().amax(-2, keepdim=True)
    err = ((eps16 + 2 * eps_e + (n + 2 * tiles + 2) * UM) * pv + (eps_e + (n + 2 * tiles) * UM) * o.abs()
           + n * sub * vmax)
    return interval16(o, err, dt)


# ------------------------------------------------------------------------------------------------------------ checking
def ratio_stats(err: torch.Tensor, bound: torch.Tensor):
    """(median, max) of err / bound over the elements whose bound is positive and finite (elsewhere exactness is required)."""
    m = (bound > 0) & torch.isfinite(bound)
    if not bool(m.any()):
        return 0.0, 0.0
    r = (err[m] / bound[m]).float()
    return float(r.median()), float(r.max())


REPORT: dict = {}


def _record(name, med, mx, n_exact):
    old = REPORT.get(name)
    if old is None:
        REPORT[name] = {"median": med, "max": mx, "exact_elements": n_exact, "calls": 1}
    else:
        old["median"] = max(old["median"], med)
        old["max"] = max(old["max"], mx)
        old["exact_elements"] += n_exact
        old["calls"] += 1


def check16(name: str, got: torch.Tensor, ref: Ref16, where=None):
    """got (16-bit) within [ref.lo, ref.hi] everywhere (nan exactly where the reference is nan)."""
    g = got.to(torch.float64)
    if where is not None:
        g, ref = g[where], Ref16(ref.value[where], ref.lo[where], ref.hi[where])
    nan_ref = torch.isnan(ref.value)
    assert torch.equal(torch.isnan(g), nan_ref), f"{name}: nan where the reference has none (or the reverse)"
    g, lo, hi, v = (t[~nan_ref] for t in (g, ref.lo, ref.hi, ref.value))
    bad = ~((g >= lo) & (g <= hi))
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound; first: got {float(g.flatten()[i])!r}, "
                             f"reference {float(v.flatten()[i])!r}, allowed [{float(lo.flatten()[i])!r}, {float(hi.flatten()[i])!r}]")
    fin = torch.isfinite(v) & torch.isfinite(g)
    bound = torch.maximum(v - lo, hi - v)[fin]
    med, mx = ratio_stats((g - v).abs()[fin], bound)
    _record(name, med, mx, int((bound == 0).sum()))


def check32(name: str, got: torch.Tensor, ref: Ref32, where=None):
    g = got.to(torch.float64)
    v, b = ref.value, ref.bound
    if where is not None:
        g, v, b = g[where], v[where], b[where]
    err = (g - v).abs()
    bad = ~(err <= b)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound; first: got {float(g.flatten()[i])!r}, "
                             f"reference {float(v.flatten()[i])!r}, bound {float(b.flatten()[i])!r}")
    med, mx = ratio_stats(err, b)
    _record(name, med, mx, int((b == 0).sum()))
