"""The e4m3 stage-2 token store on the MI355X: the quantiser kernel against the torch reference bit for bit, the
streaming MaxSim over an e4m3 store against the float64 oracle on the decoded rows, batching, determinism, accuracy
against a bf16 store, and the pipeline with token_store_dtype = "fp8"."""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _edge_rows(torch, H):
    """Rows that exercise every rule of the format: zero, NaN, +-Inf, maxima at powers of two and at 448, values on
    e4m3 rounding ties, values that land in the e4m3 subnormal range, f32 subnormal maxima."""
    rows = []
    z = torch.zeros(H)
    rows.append(z.clone())
    r = torch.linspace(-1, 1, H); r[3] = float("nan"); rows.append(r)
    r = torch.linspace(-1, 1, H); r[0] = float("inf"); rows.append(r)
    r = torch.linspace(-1, 1, H); r[-1] = float("-inf"); rows.append(r)
    for e in (-126, -20, -1, 0, 1, 7, 8, 9, 30, 100):
        r = torch.linspace(-1, 1, H) * (2.0 ** e); r[1] = 2.0 ** e; rows.append(r)
    r = torch.linspace(-448, 448, H); r[0] = 448.0; rows.append(r)
    # k = 0 (max 448): ties between neighbours (mantissa 3 bits) and the subnormal grid (2^-9), both signs
    t = torch.tensor([1.0625, 1.1875, 17.0, 19.0, 2.0 ** -9 * 1.5, 2.0 ** -9 * 2.5, 2.0 ** -9 * 0.5, 2.0 ** -10 * 1.5,
                      2.0 ** -12, 3 * 2.0 ** -11, 2.0 ** -6 * 1.0625, 240.0, 232.0])
    r = torch.zeros(H); r[0] = 448.0; r[1:1 + t.numel()] = t; r[1 + t.numel(): 1 + 2 * t.numel()] = -t
    rows.append(r)
    r = torch.zeros(H); r[0] = 2.0 ** -140; r[1] = 2.0 ** -149; r[2] = -(2.0 ** -145); rows.append(r)   # f32 subnormals
    r = torch.zeros(H); r[5] = -0.0; rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize("xdt", ["f32", "f16", "bf16"])
def test_quantize_kernel_bit_identical_to_reference(torch_mod, xdt):
    torch = torch_mod
    from tristage_rag_amd.index import quantize_rows_fp8, quantize_rows_fp8_reference
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[xdt]
    H = 768
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4096, H, generator=g) * torch.exp(torch.randn(4096, 1, generator=g) * 3)
    x = torch.cat([x, _edge_rows(torch, H)]).to(tdt)
    got = quantize_rows_fp8(x.cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.float8_e4m3fn and got.shape == x.shape
    want = quantize_rows_fp8_reference(x)
    gb, wb = got.cpu().view(torch.uint8), want.view(torch.uint8)
    bad = (gb != wb).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), gb[bad[:8, 0], bad[:8, 1]].tolist(), wb[bad[:8, 0], bad[:8, 1]].tolist())
    # other row lengths: a row that is not a whole number of 1024-element passes, and a short one
    for Hx in (16, 1040):
        y = (torch.randn(37, Hx, generator=g) * 5).to(tdt)
        assert torch.equal(quantize_rows_fp8(y.cuda()).cpu().view(torch.uint8),
                           quantize_rows_fp8_reference(y).view(torch.uint8))


def _fp8_store(torch, rng, n_rows, H):
    from tristage_rag_amd.index import quantize_rows_fp8
    x = torch.from_numpy(rng.standard_normal((n_rows, H)).astype(np.float32)).cuda()
    st = quantize_rows_fp8(x)
    return st, st.float().cpu().numpy()


@pytest.mark.parametrize("H", [128, 384, 768, 1024, 2048])
@pytest.mark.parametrize("Lq", [5, 32, 33, 64, 65, 150])
def test_fp8_maxsim_against_float64_oracle(torch_mod, H, Lq):
    torch = torch_mod
    from tristage_rag_amd.index import maxsim_indexed
    rng = np.random.default_rng(H * 7 + Lq)
    n = 600 if (H == 768 and Lq in (5, 64)) else 120
    lens = rng.integers(0, 193, size=n)
    lens[:7] = [0, 1, 31, 32, 33, 192, 64]
    st, dec = _fp8_store(torch, rng, int(lens.sum()) + 64, H)
    st[5].view(torch.uint8).zero_()                                  # an all-zero token row
    dec[5] = 0.0
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 3
    docs = [dec[starts[i]: starts[i] + lens[i]] for i in range(n)]
    ts, tl = torch.from_numpy(starts).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    for qdt in ("bf16", "f16"):
        q = oracle.quantize(rng.standard_normal((Lq, H)).astype(np.float32), qdt)
        tq = torch.from_numpy(q).cuda().to(torch.bfloat16 if qdt == "bf16" else torch.float16)
        for mode in ("maxsim", "colbert"):
            want = oracle.maxsim_scores(q, docs, mode)
            got = maxsim_indexed(tq, st, ts, tl, mode=mode).cpu().numpy()
            np.testing.assert_allclose(got, want, atol=1e-5, rtol=0, err_msg=f"{qdt} {mode}")
            assert got[0] == 0.0                                     # a zero-length candidate scores 0.0


def test_fp8_maxsim_f32_query_goes_to_bf16(torch_mod):
    torch = torch_mod
    from tristage_rag_amd.index import maxsim_indexed
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 100, size=50)
    st, dec = _fp8_store(torch, rng, int(lens.sum()), 256)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    q = rng.standard_normal((20, 256)).astype(np.float32)
    got = maxsim_indexed(torch.from_numpy(q).cuda(), st, torch.from_numpy(starts).cuda(),
                         torch.from_numpy(lens.astype(np.int32)).cuda()).cpu().numpy()
    want = oracle.maxsim_scores(oracle.quantize(q, "bf16"), [dec[a: a + n] for a, n in zip(starts, lens)])
    np.testing.assert_allclose(got, want, atol=1e-5, rtol=0)


def test_fp8_candidate_and_query_batching(torch_mod):
    torch = torch_mod
    from tristage_rag_amd.index import maxsim_indexed, maxsim_indexed_batch
    rng = np.random.default_rng(11)
    H, n_store = 768, 6000
    lens_all = rng.integers(1, 193, size=n_store)
    lens_all[:3] = [0, 32, 33]
    starts_all = np.concatenate([[0], np.cumsum(lens_all)[:-1]])
    st, dec = _fp8_store(torch, rng, int(lens_all.sum()), H)
    tsa, tla = torch.from_numpy(starts_all).cuda(), torch.from_numpy(lens_all.astype(np.int32)).cuda()
    # more than 4096 candidates: the chunked launch
    q = oracle.quantize(rng.standard_normal((32, H)).astype(np.float32), "bf16")
    tq = torch.from_numpy(q).cuda().bfloat16()
    pick = rng.permutation(n_store)[:5000]
    got = maxsim_indexed(tq, st, tsa[pick], tla[pick]).cpu().numpy()
    want = oracle.maxsim_scores(q, [dec[starts_all[i]: starts_all[i] + lens_all[i]] for i in pick])
    np.testing.assert_allclose(got, want, atol=1e-5, rtol=0)
    # 64 queries of different Lq in one launch = per-query launches = the oracle
    lqs = rng.integers(1, 151, size=64)
    qs = [oracle.quantize(rng.standard_normal((int(L), H)).astype(np.float32), "bf16") for L in lqs]
    ncs = rng.integers(0, 300, size=64)
    ncs[0] = 0
    picks = [rng.permutation(n_store)[: int(c)] for c in ncs]
    q_off = np.concatenate([[0], np.cumsum(lqs)]).tolist()
    c_off = np.concatenate([[0], np.cumsum(ncs)]).tolist()
    pk = np.concatenate(picks)
    tqs = torch.from_numpy(np.concatenate(qs)).cuda().bfloat16()
    for mode in ("maxsim", "colbert"):
        got = maxsim_indexed_batch(tqs, q_off, st, tsa[pk], tla[pk], c_off, mode=mode).cpu().numpy()
        one = np.concatenate([maxsim_indexed(tqs[q_off[j]: q_off[j + 1]], st, tsa[picks[j]], tla[picks[j]],
                                             mode=mode).cpu().numpy() for j in range(64)])
        want = np.concatenate([oracle.maxsim_scores(qs[j], [dec[starts_all[i]: starts_all[i] + lens_all[i]]
                                                             for i in picks[j]], mode) for j in range(64)])
        np.testing.assert_allclose(got, want, atol=1e-5, rtol=0, err_msg=mode)
        np.testing.assert_allclose(one, want, atol=1e-5, rtol=0, err_msg=mode)
    # 50 launches on one input: the same bits
    first = maxsim_indexed_batch(tqs, q_off, st, tsa[pk], tla[pk], c_off)
    for _ in range(49):
        assert torch.equal(maxsim_indexed_batch(tqs, q_off, st, tsa[pk], tla[pk], c_off), first)


@pytest.mark.parametrize("H,min_overlap", [(768, 95), (128, 90)])
@pytest.mark.parametrize("seed", [0, 1])
def test_fp8_accuracy_against_bf16_store(torch_mod, H, min_overlap, seed):
    """Planted relevance: 1000 candidates of 64-192 Gaussian tokens, Lq = 32; 20 of them hold noisy copies of query
    tokens.  The e4m3 store's scores against exact arithmetic on the unrounded rows, and its top-100 against the bf16
    store's."""
    torch = torch_mod
    from tristage_rag_amd.index import maxsim_indexed, quantize_rows_fp8
    rng = np.random.default_rng(100 + seed)
    n, Lq = 1000, 32
    lens = rng.integers(64, 193, size=n)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rows = rng.standard_normal((int(lens.sum()), H)).astype(np.float32)
    q = oracle.quantize(rng.standard_normal((Lq, H)).astype(np.float32), "bf16")
    planted = rng.permutation(n)[:20]
    for d in planted:
        take = rng.permutation(Lq)[: 16]
        where = starts[d] + rng.permutation(int(lens[d]))[: 16]
        rows[where] = q[take] + 0.3 * rng.standard_normal((16, H)).astype(np.float32)
    exact = oracle.maxsim_scores(q, [rows[a: a + m] for a, m in zip(starts, lens)])
    tq = torch.from_numpy(q).cuda().bfloat16()
    ts, tl = torch.from_numpy(starts).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    x = torch.from_numpy(rows).cuda()
    s8 = maxsim_indexed(tq, quantize_rows_fp8(x), ts, tl).cpu().numpy()
    s16 = maxsim_indexed(tq, x.bfloat16(), ts, tl).cpu().numpy()
    err8, err16 = float(np.abs(s8 - exact).max()), float(np.abs(s16 - exact).max())
    top8, top16 = np.argsort(-s8, kind="stable")[:100], np.argsort(-s16, kind="stable")[:100]
    overlap = len(set(top8.tolist()) & set(top16.tolist()))
    planted_in_top20 = len(set(planted.tolist()) & set(np.argsort(-s8, kind="stable")[:20].tolist()))
    print(f"fp8 accuracy H={H} seed={seed}: max|err| fp8 {err8:.2e} bf16 {err16:.2e}; top-100 overlap {overlap}; "
          f"planted in top 20: {planted_in_top20}/20")
    assert err8 <= 5e-3
    assert overlap >= min_overlap
    assert planted_in_top20 == 20


def test_pipeline_with_fp8_store(tmp_path, torch_mod):
    torch = torch_mod
    from tests.test_pipeline_gpu import _corpus
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    docs = _corpus(700)
    queries = ["neural network attention", "gpu memory index", docs[5], "language model retrieval"]

    def build(name, dtype):
        pc = PipelineConfig(stage1_model="random:minilm", stage2_model="random:modernbert:64:4:2",
                            stage3_model="random:minilm", device="cuda", cache_dir=str(tmp_path / "m"),
                            index_dir=str(tmp_path / name), log_file=str(tmp_path / f"{name}.log"), log_level="WARNING",
                            stage1_top_k=200, stage2_top_k=40, stage3_top_k=10, stage1_enable_bm25=False,
                            stage2_precompute_document_embeddings=True, stage3_cache_document_tokens=True,
                            stage2_token_store_dtype=dtype)
        return RetrievalPipeline(config=pc)
    p = build("f8", "fp8")
    p.add_documents(docs)
    st = p.stage2.token_store
    assert st.data.dtype == torch.float8_e4m3fn and st.data.is_cuda
    assert p.get_pipeline_info()["stage2_token_store_dtype"] == "fp8"
    calls = []
    orig = p.stage2.score_arrays_partial
    p.stage2.score_arrays_partial = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    res = p.search_many(queries)
    assert calls, "search_many did not take the arrays path"
    assert all(len(r["results"]) == 10 for r in res)
    for q, m in zip(queries, res):
        one = p.search(q)
        assert [x["doc_id"] for x in one["results"]] == [x["doc_id"] for x in m["results"]]
        for a, b in zip(one["results"], m["results"]):
            assert a["stage2_score"] == pytest.approx(b["stage2_score"], abs=1e-5)
    path = str(tmp_path / "idx" / "pipeline_index.pkl")
    p.save_index(path)
    p2 = build("f8b", "fp8")
    p2.load_index(path)
    s2 = p2.stage2.token_store
    assert s2.data.dtype == torch.float8_e4m3fn and s2.lens == st.lens
    assert torch.equal(s2.data[: s2.rows].view(torch.uint8).cpu(), st.data[: st.rows].view(torch.uint8).cpu())
    for q, m in zip(queries, res):
        got = p2.search(q)
        assert [(x["doc_id"], x["stage2_score"]) for x in got["results"]] == \
            [(x["doc_id"], x["stage2_score"]) for x in p.search(q)["results"]]
