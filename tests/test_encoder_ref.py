"""CPU checks of tests/encoder_ref.py, the float64 references of the encoder-forward kernels: its rounding is the 16-bit
types' own, and fp32 restatements of the kernels' arithmetic stay within its bounds."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_ref as er


def all_finite(dt):
    """Every finite value of a 16-bit type (both zeros and the subnormals included)."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    x = bits.view(dt)
    return x[torch.isfinite(x)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_round16_is_the_types_rounding(dt):
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(200_000, generator=g) * 10.0 ** torch.randint(-9, 6, (200_000,), generator=g),
                   all_finite(dt).float()])
    # midpoints between neighbouring values (ties: to even), just beside them, and values around the overflow threshold
    v = all_finite(dt).double().sort().values
    mid = ((v[1:] + v[:-1]) / 2).float()
    edge = torch.tensor([65504.0, 65519.0, 65520.0, 65536.0, 1e30, -65520.0, float.fromhex("0x1.fep127"), 3.4e38])
    x = torch.cat([x, mid, torch.nextafter(mid, torch.full_like(mid, math.inf)), edge])
    assert torch.equal(er.round16(x.double(), dt), x.to(dt).double())     # float32 -> 16 bit is a single rounding in torch
    assert bool((er.ulp16(torch.tensor([1.0, 3.0, 0.0], dtype=torch.float64), dt) ==
                 torch.tensor([2.0 ** (1 - er._FMT[dt][0]), 2.0 ** (2 - er._FMT[dt][0]), 2.0 ** (er._FMT[dt][1] + 1 - er._FMT[dt][0])],
                              dtype=torch.float64)).all())


def _fs_erf32(x: np.ndarray) -> np.ndarray:
    """ts_linear_dev.h fs_erf restated in numpy fp32 (exact reciprocal and exp2 in place of the approximate hardware ones)."""
    f = np.float32
    ax = np.abs(x)
    t = (f(1.0) / (f(0.3275911) * ax + f(1.0))).astype(f)
    poly = (f(1.061405429) * t + f(-1.453152027)).astype(f)
    for c in (1.421413741, -0.284496736, 0.254829592):
        poly = (poly * t + f(c)).astype(f)
    poly = (poly * t).astype(f)
    e = np.exp2((f(-1.44269504088896341) * ax * ax).astype(f)).astype(f)
    return np.copysign((f(1.0) - poly * e).astype(f), x)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_gelu_bound_holds_for_the_fp32_formulas(dt):
    """Over every finite 16-bit input: torch's fp32 GELU and the kernels' formula (fs_erf, restated) rounded to the
    16-bit type fall inside gelu_ref's interval — the floor |u| 2^-22 is what makes that true around -5 — and the
    interval is a single value for most inputs (the rest: where the floor exceeds the spacing of the result)."""
    x = all_finite(dt)
    ref = er.gelu_ref(er.exact16(x), dt)
    small = x.double().abs() < 2.0 ** 126        # (torch's CPU formula forms x (1 + erf) first: it overflows above 2^127)
    er.check16("cpu_torch_gelu", F.gelu(x.float()).to(dt), ref, where=small)
    xf = x.float().numpy()
    with np.errstate(over="ignore"):
        y = (xf * np.float32(0.5)) * (np.float32(1.0) + _fs_erf32(xf * np.float32(0.70710678118654752440)))
    er.check16("cpu_fs_erf_gelu", torch.from_numpy(y.astype(np.float32)).to(dt), ref)
    single = int((ref.lo == ref.hi).sum())
    assert single >= 0.7 * x.numel()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_linear_bound_holds_for_fp32_matmul(dt):
    """torch's fp32 matmul of 16-bit operands (another summation order), plus bias, rounded once: inside linear_ref;
    an identity weight must reproduce x bit for bit (the interval is a single value)."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((300, 256), generator=g) * 2).to(dt)
    w = (torch.randn((96, 256), generator=g) * 0.05).to(dt)
    b = (torch.randn((96,), generator=g)).to(dt)
    got = (x.float() @ w.float().T + b.float()).to(dt)
    er.check16("cpu_linear", got, er.linear_ref(er.exact16(x), w, b, dt))
    eye = torch.eye(256).to(dt)
    r = er.linear_ref(er.exact16(x), eye, None, dt)
    assert torch.equal(r.lo, r.hi) and torch.equal(r.value, x.double())
    # a wrong bias (one block shifted by one 16-bit step) is outside the bound somewhere
    with pytest.raises(AssertionError):
        er.check16("cpu_linear_bad", (x.float() @ w.float().T + (b.float() + (torch.arange(96) // 32 == 1) * 0.03)).to(dt),
                   er.linear_ref(er.exact16(x), w, b, dt))


def test_layernorm_bound_holds_for_fp32_two_pass_and_rejects_one_pass():
    """A fp32 two-pass LayerNorm in ln_row's order stays in layernorm_ref's bound, including rows whose mean is 1e3
    standard deviations and near-constant rows; the one-pass variance E[v^2] - mean^2 on the offset rows does not."""
    g = torch.Generator().manual_seed(7)
    H = 384
    base = torch.randn((64, H), generator=g)
    rows = torch.cat([base, base * 1.0 + 1e3, 1.0 + 1e-3 * base, base[:4] * 1e-4 - 2.0])
    gamma = 1.0 + 0.2 * torch.randn((H,), generator=g)
    beta = 0.1 * torch.randn((H,), generator=g)
    for eps in (1e-12, 1e-5):
        ref = er.layernorm_ref(rows.double(), None, gamma, beta, eps, er.ln_depth(3, 32))
        lanes = rows.view(-1, 3, 32, 4).permute(0, 2, 1, 3)                 # [row, lane, chunk, 4]: lane lir owns chunks c * 32 + lir
        s = ((lanes[..., 0] + lanes[..., 1]) + (lanes[..., 2] + lanes[..., 3]))
        acc = torch.zeros(lanes.shape[:2])
        for c in range(3):
            acc = acc + s[:, :, c]
        for o in (16, 8, 4, 2, 1):
            acc = acc + acc[:, torch.arange(32) ^ o]
        mean = acc[:, :1] / H
        d = rows - mean
        var = (d * d).sum(-1, keepdim=True) / H
        y = (d * (1.0 / torch.sqrt(var + eps))) * gamma + beta
        er.check32("cpu_layernorm", y, ref)
        one_pass = (rows * rows).mean(-1, keepdim=True) - rows.mean(-1, keepdim=True) ** 2
        y1 = (rows - rows.mean(-1, keepdim=True)) / torch.sqrt(one_pass.clamp_min(0) + eps) * gamma + beta
        with pytest.raises(AssertionError):
            er.check32("cpu_layernorm_one_pass", y1, ref)


def test_attention_bound_holds_for_fp32_softmax():
    """An fp32 softmax whose probabilities are rounded to the 16-bit type before the product with V (the kernel's
    rounding point) stays within attention_ref's bound; logits up to +-80 included."""
    g = torch.Generator().manual_seed(9)
    for dt in (torch.bfloat16, torch.float16):
        B, nh, L, dh = 2, 2, 70, 32
        q, k, v = ((torch.randn((B, nh, L, dh), generator=g) * 1.5).to(dt) for _ in range(3))
        q[1] = (q[1].float() * 6).to(dt)
        lens = torch.tensor([70, 33], dtype=torch.int32)
        ref = er.attention_ref(q, k, v, lens, dh ** -0.5, dt)
        s = (q.float() @ k.float().transpose(-1, -2)) * dh ** -0.5
        valid = torch.arange(L)[None, :] < lens[:, None]
        s = s.masked_fill(~valid[:, None, None, :], -math.inf)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = (e.to(dt).float() @ v.float()) / e.sum(-1, keepdim=True)
        er.check16("cpu_attention", o.to(dt), ref, where=valid[:, None, :, None].expand(B, nh, L, dh))
