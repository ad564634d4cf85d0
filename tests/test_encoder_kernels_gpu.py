"""GPU: the encoder-forward kernels (ts_fwd.hip, ts_linear.hip, ts_mlp.hip) against float64 references with
elementwise bounds (tests/encoder_ref.py), at every compiled instantiation, over every finite 16-bit GELU input and
at the extreme rows where these kernels change behaviour.

A 16-bit result must lie in the interval of 16-bit values the kernel's arithmetic allows around the float64 value
(a single value wherever its pre-rounding error cannot cross a rounding boundary); a fp32 result within its bound.
``ENCODER_REF_REPORT=<file>`` writes the median and maximum error / bound of each check as JSON."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import encoder_ref as er

pytestmark = pytest.mark.gpu

DTS = {"bf16": torch.bfloat16, "f16": torch.float16}

# 16-bit subnormal operands of the matrix cores (v_mfma_f32_32x32x16_{bf16,f16} on gfx950), measured by
# test_gelu_exhaustive_ffn_stream through an identity projection: "kept" = the subnormal reaches the fp32 accumulator
# unchanged, "flushed" = it is read as zero.
SUBNORMAL_OPERANDS = {"bf16": "kept", "f16": "kept"}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("ENCODER_REF_REPORT")
    if path:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(er.REPORT)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rows(tile: int, many: int):
    """1, tile - 1, tile, tile + 1, and `many` (more tiles than compute units, the last one ragged)."""
    return [r for r in (1, tile - 1, tile, tile + 1) if r > 0] + [many]


def _finite(dt):
    bits = torch.arange(-32768, 32768, dtype=torch.int32, device="cuda").to(torch.int16)
    x = bits.view(dt)
    return x[torch.isfinite(x)]


def _subnormal(x, dt):
    return (x != 0) & (x.double().abs() < 2.0 ** er._FMT[dt][1])


def _as_rows(x, width):
    n = x.numel()
    pad = (-n) % width
    return torch.cat([x, x[n - pad:]] if pad else [x]).view(-1, width)


def _tiled(w, b=None):
    from tristage_rag_amd.index import TiledLinear
    N, K = w.shape
    return TiledLinear(w, b, with_layernorm=not TiledLinear.usable(N, K))


# ------------------------------------------------------------------------------------- a. exhaustive 16-bit GELU
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gelu_exhaustive_ffn_stream(dt):
    """ffn_stream_kernel with gelu over every finite 16-bit input: an identity weight (K = N = 128, no bias) reproduces
    x exactly, so the epilogue's GELU is compared directly with float64 GELU.  Without the activation the identity must
    return x bit for bit — which also measures what the matrix cores make of subnormal operands."""
    tdt = DTS[dt]
    x = _as_rows(_finite(tdt), 128)
    lin = _tiled(torch.eye(128, device="cuda").to(tdt))
    sub = _subnormal(x, tdt)
    same = lin(x)
    assert torch.equal(same[~sub], x[~sub])                      # (by value: -0 comes back as +0 from the accumulator)
    kept, flushed = bool((same[sub] == x[sub]).all()), bool((same[sub] == 0).all())
    measured = "kept" if kept else "flushed" if flushed else "mixed"
    assert measured == SUBNORMAL_OPERANDS[dt], f"{dt} subnormal operands: {measured}"
    got = lin(x, gelu=True)
    ref = er.gelu_ref(er.exact16(x), tdt)
    er.check16(f"gelu_exhaustive_ffn_stream_{dt}", got, ref, where=~sub)
    if SUBNORMAL_OPERANDS[dt] == "kept":
        er.check16(f"gelu_exhaustive_ffn_stream_{dt}", got, ref, where=sub)
    else:
        assert bool((got[sub] == 0).all())


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gelu_exhaustive_geglu(dt):
    """geglu_kernel over every finite 16-bit input (the gate 1.0: the output is the rounded GELU itself)."""
    from tristage_rag_amd.index import geglu
    tdt = DTS[dt]
    x = _as_rows(_finite(tdt), 128)
    u = torch.cat([x, torch.ones_like(x)], -1).contiguous()
    er.check16(f"gelu_exhaustive_geglu_{dt}", geglu(u), er.geglu_ref(u, tdt))


def _ln_patterns(tdt):
    """Every finite pattern whose square stays finite in the fp32 variance, positives and negatives each in bit order:
    a 384-wide row holds neighbouring values (a well-conditioned LayerNorm)."""
    x = _finite(tdt)
    x = x[x.double().abs() < 2.0 ** 56]
    bits = x.view(torch.int16).to(torch.int32)
    pos, neg = x[bits >= 0], x[bits < 0]
    pos = pos[torch.argsort(pos.view(torch.int16))]
    neg = neg[torch.argsort(neg.view(torch.int16).to(torch.int32) & 0x7fff)]
    return _as_rows(torch.cat([pos, neg]), 384)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gelu_exhaustive_fused_paths_equal_the_two_kernels(dt):
    """proj_ln_kernel<DT, true> (the GELU applied while staging) and mlp_ln_kernel<DT, 1> (bf16: the LDS table for
    2^-12 <= |u| < 8, the computed path outside it) against the two-kernel path — ts_linear_act with the GELU epilogue,
    then ts_linear_add_layernorm — bit for bit, over every finite pattern (identity W1 / W2, H = I = 384): every table
    entry, both signs and both sides of the table's edges against the computed GELU, which the test above pins to float64."""
    from tristage_rag_amd.index import mlp_add_layernorm
    tdt = DTS[dt]
    x = _ln_patterns(tdt)
    g = _gen(11)
    eye = torch.eye(384, device="cuda").to(tdt)
    up, down = _tiled(eye), _tiled(eye)
    gamma = 1.0 + 0.1 * torch.randn((384,), generator=g, device="cuda")
    beta = 0.1 * torch.randn((384,), generator=g, device="cuda")
    w32, wlp = down.add_layernorm(up(x, gelu=True), None, gamma, beta, 1e-12)
    a32, alp = down.add_layernorm(x, None, gamma, beta, 1e-12, gelu_input=True)
    m32, mlp = mlp_add_layernorm(up, down, x, None, gamma, beta, 1e-12)
    for got in (a32, m32):
        assert torch.equal(got.view(torch.int32), w32.view(torch.int32))
    for got in (alp, mlp):
        assert torch.equal(got.view(torch.int16), wlp.view(torch.int16))


# ----------------------------------------------------------------------------- b. every instantiation vs float64
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_ffn_stream_every_instantiation(dt):
    """ffn_stream_kernel<DT, QH, GELU> for QH = 3 (K = 128, 384), 2 (K = 768), 1 (K = 1536), with and without the GELU
    and the bias, at 1, tile - 1, tile, tile + 1 rows and more tiles than compute units with a ragged last tile."""
    tdt = DTS[dt]
    g = _gen(21)
    cus = _cus()
    for K, N, qh in ((128, 288, 3), (384, 96, 3), (768, 160, 2), (1536, 96, 1)):
        tile = 32 * qh
        w = (torch.randn((N, K), generator=g, device="cuda") * K ** -0.5).to(tdt)
        b = (torch.randn((N,), generator=g, device="cuda") * 0.5).to(tdt)
        for i, M in enumerate(_rows(tile, tile * (cus + 3) + 7)):
            x = (torch.randn((M, K), generator=g, device="cuda") * 1.5).to(tdt)
            bias = b if i % 2 == 0 else None
            lin = _tiled(w, bias)
            er.check16(f"ffn_stream_qh{qh}_{dt}", lin(x), er.linear_ref(er.exact16(x), w, bias, tdt))
            er.check16(f"ffn_stream_gelu_qh{qh}_{dt}", lin(x, gelu=True), er.linear_gelu_ref(er.exact16(x), w, bias, tdt))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_proj_ln_every_instantiation(dt):
    """proj_ln_kernel<DT, GELU_IN> for N in {32, 128, 160, 384}, one and four 384-wide chunks, with and without bias,
    residual and beta: the fp32 stream and the 16-bit copy against float64, and the fused GELU_IN path against the
    two-kernel path bit for bit."""
    from tristage_rag_amd.index import add_layernorm
    tdt = DTS[dt]
    g = _gen(31)
    for N, K in ((32, 384), (128, 1536), (160, 384), (384, 384), (384, 1536)):
        w = (torch.randn((N, K), generator=g, device="cuda") * K ** -0.5).to(tdt)
        b = (torch.randn((N,), generator=g, device="cuda") * 0.3).to(tdt)
        gamma = 1.0 + 0.2 * torch.randn((N,), generator=g, device="cuda")
        beta = 0.2 * torch.randn((N,), generator=g, device="cuda")
        for i, M in enumerate(_rows(96, 96 * 300 + 5)):
            full = i % 2 == 0
            bias, bt = (b, beta) if full else (None, None)
            lin = _tiled(w, bias)
            x = (torch.randn((M, K), generator=g, device="cuda") * 1.2).to(tdt)
            res = torch.randn((M, N), generator=g, device="cuda") if full or i == 3 else None
            for gelu_in in (False, True):
                y32, ylp = lin.add_layernorm(x, res, gamma, bt, 1e-12, gelu_input=gelu_in)
                ref = er.proj_ln_ref(x, w, bias, res, gamma, bt, 1e-12, tdt, gelu_in=gelu_in)
                name = f"proj_ln{'_gelu_in' if gelu_in else ''}_{dt}"
                er.check32(name, y32, ref)
                er.check16(name + "_lp", ylp, er.to16(ref, tdt))
                assert torch.equal(ylp, y32.to(tdt))
                if gelu_in:     # == the GELU of ts_linear_act's epilogue, then the plain kernel: bit for bit
                    e32, elp = lin.add_layernorm(_gelu_rows(x), res, gamma, bt, 1e-12)
                    assert torch.equal(y32, e32) and torch.equal(ylp, elp)
            if N > 128 and M == 96:     # the two-kernel path: ts_linear_act, then ts_add_layernorm (same bits, as promised)
                e32, elp = add_layernorm(lin(x), res, gamma, bt, 1e-12, lp_dtype=tdt)
                y32, ylp = lin.add_layernorm(x, res, gamma, bt, 1e-12)
                assert torch.equal(y32, e32) and torch.equal(ylp, elp)


def _gelu_rows(x):
    """The GELU epilogue of ts_linear_act on x itself (identity weights of 384 over each 384-wide slice)."""
    tdt, K = x.dtype, x.shape[-1]
    eye = _tiled(torch.eye(384, device="cuda").to(tdt))
    return torch.cat([eye(x[:, i:i + 384].contiguous(), gelu=True) for i in range(0, K, 384)], -1).contiguous()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_mlp_every_instantiation(dt):
    """mlp_ln_kernel<DT, NCH> for NCH = 1..4 (I = 384 .. 1536) against float64 and, bit for bit, against the two-kernel
    path (ts_linear_act with the GELU, then ts_linear_add_layernorm), with and without biases, residual and beta."""
    from tristage_rag_amd.index import mlp_add_layernorm, mlp_usable
    tdt = DTS[dt]
    g = _gen(41)
    H = 384
    gamma = 1.0 + 0.2 * torch.randn((H,), generator=g, device="cuda")
    beta = 0.2 * torch.randn((H,), generator=g, device="cuda")
    for nch in (1, 2, 3, 4):
        I = 384 * nch
        w1 = (torch.randn((I, H), generator=g, device="cuda") * H ** -0.5 * 1.5).to(tdt)
        b1 = (torch.randn((I,), generator=g, device="cuda") * 0.5).to(tdt)
        w2 = (torch.randn((H, I), generator=g, device="cuda") * I ** -0.5).to(tdt)
        b2 = (torch.randn((H,), generator=g, device="cuda") * 0.3).to(tdt)
        for i, M in enumerate(_rows(96, 96 * 300 + 5)):
            full = i % 2 == 0
            up, down = _tiled(w1, b1 if full else None), _tiled(w2, b2 if full else None)
            assert mlp_usable(up, down)
            x = (torch.randn((M, H), generator=g, device="cuda")).to(tdt)
            res = torch.randn((M, H), generator=g, device="cuda") if full or i == 3 else None
            bt = beta if full else None
            m32, mlp = mlp_add_layernorm(up, down, x, res, gamma, bt, 1e-12)
            ref = er.mlp_ref(x, w1, b1 if full else None, w2, b2 if full else None, res, gamma, bt, 1e-12, tdt)
            er.check32(f"mlp_nch{nch}_{dt}", m32, ref)
            er.check16(f"mlp_nch{nch}_{dt}_lp", mlp, er.to16(ref, tdt))
            w32, wlp = down.add_layernorm(up(x, gelu=True), res, gamma, bt, 1e-12)
            assert torch.equal(m32, w32) and torch.equal(mlp, wlp)


LN_BUCKETS = (128, 256, 384, 512, 768, 1024, 1540)   # (NCH, LPR) = (1,32) (2,32) (3,32) (2,64) (3,64) (4,64) (8,64)


@pytest.mark.parametrize("xdt", ["f32", "bf16", "f16"])
def test_add_layernorm_every_bucket(xdt):
    """add_layernorm_kernel<XDT, NCH, LPR, false>: every (NCH, LPR) bucket, every input type, both 16-bit outputs,
    post-LN and pre-LN, with and without residual and beta, at 1, 7, 8, 9 rows (8 rows per workgroup at half-wave rows)
    and more rows than the 2048-workgroup grid covers in one pass."""
    from tristage_rag_amd.index import add_layernorm
    tdt = {"f32": torch.float32, **DTS}[xdt]
    g = _gen(51)
    for H in LN_BUCKETS:
        nch, lpr = er.ln_shape(H)
        per_wg = 4 * (64 // lpr)
        gamma = 1.0 + 0.2 * torch.randn((H,), generator=g, device="cuda")
        beta = 0.2 * torch.randn((H,), generator=g, device="cuda")
        for i, rows in enumerate(_rows(per_wg, 2048 * per_wg + 5)):
            x = (torch.randn((rows, H), generator=g, device="cuda") * 0.8).to(tdt)
            res = torch.randn((rows, H), generator=g, device="cuda") * 1.5 + 0.3 if i != 1 else None
            bt = beta if i != 2 else None
            lp = (torch.bfloat16, torch.float16)[i % 2]
            for prenorm in (False, True):
                y32, ylp = add_layernorm(x, res, gamma, bt, 1e-12, lp_dtype=lp, prenorm=prenorm)
                r32, rln = er.add_layernorm_ref(x, res, gamma, bt, 1e-12, prenorm=prenorm)
                er.check32(f"add_layernorm_H{H}_{xdt}{'_prenorm' if prenorm else ''}", y32, r32)
                er.check16(f"add_layernorm_H{H}_{xdt}_lp", ylp, er.to16(rln, lp))
                if not prenorm:
                    assert torch.equal(ylp, y32.to(lp))


def test_embed_layernorm_every_bucket():
    """add_layernorm_kernel<F32, NCH, LPR, true> (ts_embed_layernorm): every bucket, with and without token types."""
    from tristage_rag_amd.index import embed_layernorm
    g = _gen(61)
    for j, H in enumerate(LN_BUCKETS):
        nch, lpr = er.ln_shape(H)
        per_wg = 4 * (64 // lpr)
        V, P = 1000, 600
        word = torch.randn((V, H), generator=g, device="cuda")
        pos = torch.randn((P, H), generator=g, device="cuda") * 0.3
        typ = torch.randn((2, H), generator=g, device="cuda") * 0.5
        gamma = 1.0 + 0.2 * torch.randn((H,), generator=g, device="cuda")
        beta = 0.2 * torch.randn((H,), generator=g, device="cuda")
        for i, rows in enumerate(_rows(per_wg, 2048 * per_wg + 5)):
            ids = torch.randint(0, V, (rows,), generator=g, device="cuda")
            pid = torch.randint(0, P, (rows,), generator=g, device="cuda")
            tt = torch.randint(0, 2, (rows,), generator=g, device="cuda") if (i + j) % 2 == 0 else None
            lp = (torch.bfloat16, torch.float16)[i % 2]
            y32, ylp = embed_layernorm(ids, pid, tt, word, pos, typ, gamma, beta, 1e-12, lp_dtype=lp)
            ref = er.embed_layernorm_ref(ids, pid, tt, word, pos, typ, gamma, beta, 1e-12)
            er.check32(f"embed_layernorm_H{H}", y32, ref)
            er.check16(f"embed_layernorm_H{H}_lp", ylp, er.to16(ref, lp))


def _rope_tables(L, dh, base=10000.0):
    inv = 1.0 / base ** (torch.arange(0, dh, 2, device="cuda", dtype=torch.float32) / dh)
    f = torch.arange(L, device="cuda", dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat([f, f], -1)
    return emb.cos().contiguous(), emb.sin().contiguous()


def _attention_case(name, qkv, lens, nh, dt, window=0, rope=False, scale=None):
    """attn_varlen_kernel on qkv [B, L, 3 H] against float64 over each sequence's valid queries; with rope, the rotation
    (rope_kernel, itself checked against float64 here) is the reference's input — fw_rope8 in the attention kernel is
    the same arithmetic, which test_pipeline_gpu checks bit for bit."""
    from tristage_rag_amd.index import attention_varlen, rope_inplace
    tdt = DTS[dt]
    B, L, W = qkv.shape
    dh = W // (3 * nh)
    scale = dh ** -0.5 if scale is None else scale
    tabs = _rope_tables(L, dh) if rope else None
    got = attention_varlen(qkv, lens, nh, window=window, rope=tabs, scale=scale)
    src = qkv
    if rope:
        src = rope_inplace(qkv.clone(), tabs[0], tabs[1], nh)
        for which in (0, 1):
            x = qkv.view(B, L, 3, nh, dh)[:, :, which].transpose(1, 2)
            er.check16(f"rope_{dt}", src.view(B, L, 3, nh, dh)[:, :, which].transpose(1, 2), er.rope_ref(x, tabs[0], tabs[1], tdt))
    q, k, v = (src.view(B, L, 3, nh, dh)[:, :, i].transpose(1, 2) for i in range(3))
    ref = er.attention_ref(q, k, v, lens, scale, tdt, window=window)
    valid = torch.arange(L, device="cuda")[None, :] < lens[:, None]
    er.check16(name, got.view(B, L, nh, dh).transpose(1, 2), ref, where=valid[:, None, :, None].expand(B, nh, L, dh))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("rope", [False, True])
def test_attention_every_instantiation(dt, dh, rope):
    """attn_varlen_kernel<DT, DH, ROPE>: sequences of 1, 31, 32, 33 and many query tiles, windows wider and narrower
    than a key tile."""
    tdt = DTS[dt]
    g = _gen(71 + dh)
    nh, L = 3, 200
    lens = torch.tensor([1, 31, 32, 33, 200, 137], dtype=torch.int32, device="cuda")
    qkv = (torch.randn((len(lens), L, 3 * nh * dh), generator=g, device="cuda") * 1.2).to(tdt)
    for window in (0, 5, 40):
        _attention_case(f"attention_dh{dh}{'_rope' if rope else ''}_{dt}", qkv, lens, nh, dt, window=window, rope=rope)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rope_and_geglu_kernels(dt):
    """rope_kernel (in place on q and k) and geglu_kernel on random data against float64."""
    from tristage_rag_amd.index import geglu, rope_inplace
    tdt = DTS[dt]
    g = _gen(81)
    for B, L, nh, dh in ((3, 77, 4, 64), (1, 5, 2, 8), (2, 33, 6, 32)):
        qkv = (torch.randn((B, L, 3 * nh * dh), generator=g, device="cuda") * 2).to(tdt)
        cos, sin = _rope_tables(L, dh)
        out = rope_inplace(qkv.clone(), cos, sin, nh).view(B, L, 3, nh, dh)
        src = qkv.view(B, L, 3, nh, dh)
        for which in (0, 1):
            er.check16(f"rope_{dt}", out[:, :, which].transpose(1, 2), er.rope_ref(src[:, :, which].transpose(1, 2), cos, sin, tdt))
        assert torch.equal(out[:, :, 2], src[:, :, 2])                       # v is not touched
    for rows, I in ((1, 8), (1000, 1152), (7, 24)):
        u = (torch.randn((rows, 2 * I), generator=g, device="cuda") * 2.5).to(tdt)
        er.check16(f"geglu_{dt}", geglu(u), er.geglu_ref(u, tdt))


# --------------------------------------------------------------------------------------------- c. extreme rows
@pytest.mark.parametrize("xdt", ["f32", "bf16"])
def test_layernorm_extreme_rows(xdt):
    """Rows whose mean is about 1e3 standard deviations (BERT's outlier dimensions: a one-pass variance loses all of it)
    and near-constant rows at eps = 1e-12 and 1e-5, through ts_add_layernorm (several buckets) and the LayerNorm
    epilogues of ts_linear_add_layernorm and ts_mlp_add_layernorm."""
    from tristage_rag_amd.index import add_layernorm, mlp_add_layernorm
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[xdt]
    g = _gen(91)
    for H in (128, 384, 1024):
        base = torch.randn((64, H), generator=g, device="cuda")
        gamma = 1.0 + 0.2 * torch.randn((H,), generator=g, device="cuda")
        beta = 0.2 * torch.randn((H,), generator=g, device="cuda")
        offset = base + 1e3 * torch.sign(torch.randn((64, 1), generator=g, device="cuda"))
        near = 1.0 + 1e-3 * base
        for rows, res in ((offset, None), (near, None), (base * 0.01, offset - base * 0.01)):
            x = rows.to(tdt)
            for eps in (1e-12, 1e-5):
                y32, ylp = add_layernorm(x, res, gamma, beta, eps, lp_dtype=torch.bfloat16)
                ref, _ = er.add_layernorm_ref(x, res, gamma, beta, eps)
                er.check32(f"layernorm_extreme_H{H}_{xdt}", y32, ref)
                er.check16(f"layernorm_extreme_H{H}_{xdt}_lp", ylp, er.to16(ref, torch.bfloat16))
    if xdt == "bf16":   # the fused epilogues: the outlier lives in the residual stream
        H = 384
        x = (torch.randn((500, H), generator=g, device="cuda")).to(tdt)
        res = torch.randn((500, H), generator=g, device="cuda") + 1e3
        res[::2] = 1.0 + 1e-4 * torch.randn((250, H), generator=g, device="cuda")
        w = (torch.randn((H, H), generator=g, device="cuda") * 0.001).to(tdt)
        gamma = 1.0 + 0.2 * torch.randn((H,), generator=g, device="cuda")
        for eps in (1e-12, 1e-5):
            lin = _tiled(w)
            y32, _ = lin.add_layernorm(x, res, gamma, None, eps)
            er.check32("proj_ln_extreme_bf16", y32, er.proj_ln_ref(x, w, None, res, gamma, None, eps, tdt))
            m32, _ = mlp_add_layernorm(_tiled(w), lin, x, res, gamma, None, eps)
            er.check32("mlp_extreme_bf16", m32, er.mlp_ref(x, w, None, w, None, res, gamma, None, eps, tdt))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_attention_extreme_logits(dt):
    """Logits up to +-80 (exp overflows fp32 without the running maximum), a single dominating key, all keys equal,
    and windows shorter than a key tile."""
    tdt = DTS[dt]
    g = _gen(101)
    B, L, nh, dh = 3, 100, 2, 32
    c = math.sqrt(80.0 / (dh * dh ** -0.5))                     # q.k scale = +-80 for q, k = +-c (1, ..., 1)
    q = torch.sign(torch.randn((B, L, nh, 1), generator=g, device="cuda")) * c * torch.ones((B, L, nh, dh), device="cuda")
    k = torch.linspace(-1, 1, L, device="cuda")[None, :, None, None] * c * torch.ones((B, L, nh, dh), device="cuda")
    k = k[:, torch.randperm(L, generator=g, device="cuda")]
    v = torch.randn((B, L, nh, dh), generator=g, device="cuda")
    lens = torch.tensor([100, 33, 64], dtype=torch.int32, device="cuda")
    qkv = torch.stack([q, k, v], 2).reshape(B, L, 3 * nh * dh).to(tdt).contiguous()
    for window in (0, 3, 20):
        _attention_case(f"attention_extreme_{dt}", qkv, lens, nh, dt, window=window)
    # one key far above the rest (logit about 18 against about 0)
    e = torch.full((dh,), dh ** -0.5, device="cuda")
    q = torch.randn((B, L, nh, dh), generator=g, device="cuda") * 0.3 + e
    k = torch.randn((B, L, nh, dh), generator=g, device="cuda") * 0.3
    k[:, 17] = 100.0 * e
    qkv = torch.stack([q, k, v], 2).reshape(B, L, 3 * nh * dh).to(tdt).contiguous()
    _attention_case(f"attention_extreme_{dt}", qkv, lens, nh, dt)
    # all keys equal: the output is the mean of the valid values
    k = torch.randn((1, 1, nh, dh), generator=g, device="cuda").expand(B, L, nh, dh)
    qkv = torch.stack([q, k, v], 2).reshape(B, L, 3 * nh * dh).to(tdt).contiguous()
    for window in (0, 7):
        _attention_case(f"attention_extreme_{dt}", qkv, lens, nh, dt, window=window)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_projection_extremes(dt):
    """Up-projection outputs far beyond +-8 (the bf16 MLP's computed GELU under its wave-level branch, for whole waves
    and for single lanes), and fp16 projections that overflow 65504: +-inf exactly where torch's F.linear has them."""
    from tristage_rag_amd.index import mlp_add_layernorm
    tdt = DTS[dt]
    g = _gen(111)
    H, I, M = 384, 768, 1000
    w1 = (torch.randn((I, H), generator=g, device="cuda") * H ** -0.5).to(tdt)
    w2 = (torch.randn((H, I), generator=g, device="cuda") * I ** -0.5).to(tdt)
    b1 = (torch.randn((I,), generator=g, device="cuda")).to(tdt)
    gamma = 1.0 + 0.2 * torch.randn((H,), generator=g, device="cuda")
    x = torch.randn((M, H), generator=g, device="cuda")
    x[: M // 2] *= 30.0                                           # whole rows far outside the table
    x[M // 2:, ::7] *= 40.0                                       # single large inputs within ordinary rows
    x = x.to(tdt)
    res = torch.randn((M, H), generator=g, device="cuda")
    up, down = _tiled(w1, b1), _tiled(w2)
    m32, mlp = mlp_add_layernorm(up, down, x, res, gamma, None, 1e-12)
    ref = er.mlp_ref(x, w1, b1, w2, None, res, gamma, None, 1e-12, tdt)
    er.check32(f"mlp_large_{dt}", m32, ref)
    w32, wlp = down.add_layernorm(up(x, gelu=True), res, gamma, None, 1e-12)
    assert torch.equal(m32, w32) and torch.equal(mlp, wlp)
    if dt == "f16":
        K, N = 128, 64
        w = (torch.randn((N, K), generator=g, device="cuda") * 4).to(tdt)
        xb = (torch.randn((300, K), generator=g, device="cuda") * 2000).to(tdt)
        lin = _tiled(w)
        got = lin(xb)
        assert bool(torch.isinf(got).any()) and bool((got == -math.inf).any()) and bool((got == math.inf).any())
        er.check16("linear_overflow_f16", got, er.linear_ref(er.exact16(xb), w, None, tdt))
        want = F.linear(xb.float(), w.float()).to(tdt)
        assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(got[torch.isinf(got)], want[torch.isinf(want)])
        assert not bool(torch.isnan(got).any())
        gg = lin(xb, gelu=True)                                  # gelu(+inf) = +inf; gelu(-inf) = nan, like torch's formula
        pre = er.linear_ref(er.exact16(xb), w, None, tdt)
        sure = (pre.lo > -math.inf) | (pre.hi == -math.inf)     # (not where the projection may or may not reach -inf)
        er.check16("linear_overflow_gelu_f16", gg, er.gelu_ref(pre, tdt), where=sure)
