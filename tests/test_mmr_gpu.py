"""Maximal marginal relevance on the GPU (ts_index_mmr / ts_mmr_ivf) against the float64 host model
of tests/mmr_model.py.

Exact: integer rows (exact_inputs.gen_ints) make every similarity, relevance and objective an f32 number whatever the
order of the additions (tests/test_mmr_host.py), so ids and relevances must EQUAL the model's, and bulk exact ties pin
the tie rule and the bit symmetry of the Gram matrix.  Unit rows: accepted step by step (``step_valid``) with the
``tie_tol`` of ``oracle.check_topk``: the objective's only inexact term is one f32 MFMA sum of unit-row products
against float64, the arithmetic that tolerance was set for, times (1 - lambda) <= 1."""
import inspect

import numpy as np
import pytest

import exact_inputs as xi
import mmr_model as mm
from oracle import oracle

pytestmark = pytest.mark.gpu

LAMBDAS = (0.0, 0.25, 0.5, 0.75, 1.0)
TIE_TOL = inspect.signature(oracle.check_topk).parameters["tie_tol"].default
N_EXACT = 1061
EXACT_CASES = [(dt, d) for dt in ("f16", "bf16", "f32") for d in (40, 768, 1024)] + [("fp8", 256), ("fp8", 768)]
EXACT_B = (1, 33)
EXACT_C = (1, 31, 32, 33, 100, 1024)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _ix():
    from tristage_rag_amd import index
    return index


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _exact_rows(dtype, d, n=N_EXACT, B=max(EXACT_B)):
    c, q, _ = xi.gen_ints(n, d, B)
    if dtype == "fp8":       # integers |v| <= 15: what e4m3 holds exactly (scale exponent 0)
        c = np.random.default_rng([d, 15]).integers(-15, 16, size=(n, d)).astype(np.float32)
    return c, q


def _flat(dtype, d, rows):
    idx = _ix().FlatIPIndex(d, dtype=dtype, fp8_scale_log2=0) if dtype == "fp8" else _ix().FlatIPIndex(d, dtype=dtype)
    idx.add(rows)
    return idx


def _gram(X, ids):
    """S [B, C, C] float32 of the stored rows ids index (-1: a zero row).  For the integer rows every entry is an
    integer below 2^22 (asserted), so the float32 product IS the float64 one."""
    rows = np.where(ids[..., None] >= 0, X[np.clip(ids, 0, None)], np.float32(0.0))
    return rows @ rows.transpose(0, 2, 1)


def _expect(ids, rel, S, k, lam, valid=None):
    """(D, I) [B, k] of the model."""
    picks = mm.mmr_select_batch(rel, S, k, lam, valid)
    B = ids.shape[0]
    D = np.full((B, k), -mm.FLT_MAX, dtype=np.float32)
    I = np.full((B, k), -1, dtype=np.int64)
    ok = picks >= 0
    r, _ = np.nonzero(ok)
    D[ok] = rel[r, picks[ok]]
    I[ok] = ids[r, picks[ok]]
    return D, I


# ---------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("dtype,d", EXACT_CASES)
def test_exact_rows_equal_the_model(torch_mod, dtype, d):
    torch = torch_mod
    c, q = _exact_rows(dtype, d)
    amp = 15 if dtype == "fp8" else 63
    assert amp * amp * d < 2 ** 22
    idx = _flat(dtype, d, c)
    X = idx.reconstruct_n()
    assert np.array_equal(X, c)                                   # stored exactly: sim is the integers' product
    rng = np.random.default_rng([d, 7])
    for B in EXACT_B:
        qt = torch.from_numpy(q[:B]).cuda()
        for C in EXACT_C:
            D0, I0 = idx.search(qt, C)
            ids, rel = _np(I0).copy(), _np(D0).copy()
            for b in range(1, B, 2):          # odd queries: an explicit list in no particular order, with padding
                perm = rng.permutation(C)
                ids[b], rel[b] = ids[b, perm], rel[b, perm]
                ids[b, rng.integers(0, C, size=max(1, C // 16))] = -1
            if B == 1 and C >= 32:            # ... and one with repeated relevances at the front
                rel[0, :8] = rel[0, 0]
            valid = ids >= 0
            S = _gram(X, ids)
            assert np.abs(S).max() < 2 ** 22 and np.abs(rel).max() < 2 ** 22
            ids_t, rel_t = torch.from_numpy(ids).cuda(), torch.from_numpy(rel).cuda()
            for lam in LAMBDAS:
                want_D, want_I = _expect(ids, rel, S, C, lam, valid)          # the picks of a smaller k: a prefix
                for k in sorted({1, min(20, C), C}):
                    D, I = idx.mmr(ids_t, rel_t, k, lam)
                    kk = (dtype, d, B, C, k, lam)
                    if k < C:     # (the tail of a short query is padding also where a longer k goes on)
                        wD, wI = _expect(ids, rel, S, k, lam, valid)
                        assert np.array_equal(wI, want_I[:, :k])
                    else:
                        wD, wI = want_D, want_I
                    assert np.array_equal(_np(I), wI), kk
                    assert np.array_equal(_np(D).view(np.uint32), wD.view(np.uint32)), kk
                    if lam == 1.0 and not (B == 1 and C >= 32):
                        even = np.arange(0, B, 2)                             # search's own lists: their first k entries
                        assert np.array_equal(_np(I)[even], _np(I0)[even, :k]), kk


def test_numpy_lists_go_through_host_pointers_and_bad_ids_are_refused(torch_mod):
    c, q = _exact_rows("f16", 40)
    idx = _flat("f16", 40, c)
    D0, I0 = idx.search(q[:3], 33)                                # numpy in, numpy out
    X = idx.reconstruct_n()
    want = _expect(I0, D0, _gram(X, I0), 7, 0.5)
    D, I = idx.mmr(I0, D0, 7, 0.5)
    assert isinstance(I, np.ndarray) and np.array_equal(I, want[1]) and np.array_equal(D, want[0])
    for bad in (N_EXACT, -2, 1 << 40):
        ids = I0.copy()
        ids[1, 4] = bad
        with pytest.raises(ValueError, match="outside"):
            idx.mmr(ids, D0, 7, 0.5)
    # device ids cannot be checked without a synchronisation: an unknown id is skipped like padding, never read
    ids = I0.copy()
    ids[1, 4] = N_EXACT + 5
    Dd, Id = idx.mmr(torch_mod.from_numpy(ids).cuda(), torch_mod.from_numpy(D0).cuda(), 7, 0.5)
    ids[1, 4] = -1
    want = _expect(ids, D0, _gram(X, ids), 7, 0.5, ids >= 0)
    assert np.array_equal(_np(Id), want[1]) and np.array_equal(_np(Dd), want[0])


def test_mask_leaving_ten_rows_gives_a_padded_tail(torch_mod):
    c, q = _exact_rows("bf16", 768)
    idx = _flat("bf16", 768, c)
    allowed = np.zeros(N_EXACT, dtype=bool)
    keep = np.array([3, 40, 41, 333, 512, 700, 701, 702, 1000, 1060])
    allowed[keep] = True
    qt = torch_mod.from_numpy(q[:5]).cuda()
    for lam in LAMBDAS:
        D, I = idx.search_mmr(qt, 20, fetch_k=32, lambda_mult=lam, allowed=allowed)
        D0, I0 = idx.search(qt, 32, allowed=allowed)
        ids, rel = _np(I0), _np(D0)
        assert (ids[:, 10:] == -1).all() and (np.sort(ids[:, :10], axis=1) == keep).all()
        wD, wI = _expect(ids, rel, _gram(idx.reconstruct_n(), ids), 20, lam, ids >= 0)
        assert np.array_equal(_np(I), wI) and np.array_equal(_np(D).view(np.uint32), wD.view(np.uint32))
        assert (_np(I)[:, 10:] == -1).all() and (_np(D)[:, 10:] == -mm.FLT_MAX).all()


# ---------------------------------------------------------------------------------------------------- composition
def _same_bits(a, b):
    assert np.array_equal(_np(a[1]), _np(b[1])), "ids"
    assert np.array_equal(_np(a[0]).view(np.uint32), _np(b[0]).view(np.uint32)), "relevances"


@pytest.mark.parametrize("dtype", ["f16", "f32", "fp8"])
def test_search_mmr_is_search_then_mmr_also_after_remove_update_and_offset(torch_mod, dtype):
    torch = torch_mod
    d, B, k, fk = 256, 9, 12, 48
    c, q = _exact_rows(dtype, d, n=2000, B=B)
    idx = _flat(dtype, d, c)
    qt = torch.from_numpy(q).cuda()
    allowed = np.random.default_rng(3).random(2000) < 0.5
    for lam in (0.25, 0.75):
        for al in (None, allowed):
            _same_bits(idx.search_mmr(qt, k, fk, lam, allowed=al), idx.mmr(*idx.search(qt, fk, allowed=al)[::-1], k, lam))
    D, I = idx.search_mmr(qt, k)                                   # the default fetch_k
    assert tuple(I.shape) == (B, k)
    _same_bits((D, I), idx.mmr(*idx.search(qt, _ix().mmr_default_fetch_k(k))[::-1], k, 0.5))
    # removed rows are never returned, neither through the search nor from an explicit list that still names them
    D0, I0 = idx.search(qt, fk)
    gone = np.unique(_np(I0)[:, :6].reshape(-1))
    assert idx.remove_ids(gone) == gone.size
    for lam in (0.25, 0.75):
        got = idx.search_mmr(qt, k, fk, lam)
        _same_bits(got, idx.mmr(*idx.search(qt, fk)[::-1], k, lam))
        assert not np.isin(_np(got[1]), gone).any()
        Ds, Is = idx.mmr(I0, D0, k, lam)                           # the list from before the removal
        assert not np.isin(_np(Is), gone).any()
        ids, rel = _np(I0), _np(D0)
        valid = ~np.isin(ids, gone)
        wD, wI = _expect(ids, rel, _gram(idx.reconstruct_n(), ids), k, lam, valid)
        assert np.array_equal(_np(Is), wI) and np.array_equal(_np(Ds), wD)
    # update: the similarity is that of the new row
    D1, I1 = idx.search(qt, fk)
    upd = np.unique(_np(I1)[:, 1])
    new_rows = np.random.default_rng(11).integers(-15, 16, size=(upd.size, d)).astype(np.float32)
    idx.update_rows(upd, new_rows)
    X = idx.reconstruct_n()
    assert np.array_equal(X[upd], new_rows)
    for lam in (0.25, 0.75):
        _same_bits(idx.search_mmr(qt, k, fk, lam), idx.mmr(*idx.search(qt, fk)[::-1], k, lam))
        ids, rel = _np(I1), _np(D1)                                # an explicit list: old relevances, new rows
        wD, wI = _expect(ids, rel, _gram(X, ids), k, lam)
        Du, Iu = idx.mmr(I1, D1, k, lam)
        assert np.array_equal(_np(Iu), wI) and np.array_equal(_np(Du), wD)
    # ids come back in the offset id space
    base = idx.search_mmr(qt, k, fk, 0.5)
    idx.set_id_offset(1_000_000)
    off = idx.search_mmr(qt, k, fk, 0.5)
    assert np.array_equal(_np(off[1]), _np(base[1]) + 1_000_000) and np.array_equal(_np(off[0]), _np(base[0]))
    _same_bits(off, idx.mmr(*idx.search(qt, fk)[::-1], k, 0.5))


# ------------------------------------------------------------------------------------------------------------ IVF
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_ivf_search_mmr_equals_flat_mmr_of_the_ivf_search(torch_mod, dtype):
    torch = torch_mod
    n, d, B = 3000, 96, 17
    rng = np.random.default_rng(21)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = torch.from_numpy(x[rng.integers(0, n, size=B)] + 0.05 * rng.standard_normal((B, d)).astype(np.float32)).cuda()
    ivf = _ix().IVFFlatIndex(d, nlist=16, dtype=dtype, nprobe=4)
    ivf.train(x)
    ivf.add(x)
    flat = _ix().FlatIPIndex(d, dtype=dtype)
    flat.add(x)
    assert np.array_equal(ivf.reconstruct_n().view(np.uint32), flat.reconstruct_n().view(np.uint32))
    for fk, k in ((33, 10), (200, 40)):
        for lam in (0.3, 0.7):
            D0, I0 = ivf.search(q, fk)
            _same_bits(ivf.search_mmr(q, k, fk, lam), flat.mmr(I0, D0, k, lam))
    gone = np.unique(_np(ivf.search(q, 4)[1]))
    gone = gone[gone >= 0]
    D0, I0 = ivf.search(q, 64)
    assert ivf.remove_ids(gone) == gone.size and flat.remove_ids(gone) == gone.size
    got = ivf.mmr(I0, D0, 20, 0.5)                                 # a list that still names removed rows
    assert not np.isin(_np(got[1]), gone).any()
    _same_bits(got, flat.mmr(I0, D0, 20, 0.5))
    _same_bits(ivf.search_mmr(q, 20, 64, 0.5), flat.mmr(*ivf.search(q, 64)[::-1], 20, 0.5))


# ------------------------------------------------------------------------------------------------------ unit rows
@pytest.fixture(scope="module")
def unit_rows():
    rng = np.random.default_rng(31)
    x = rng.standard_normal((4096, 384)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    # clustered, so that the diversity term decides picks: every row is pulled towards one of 64 centres
    cen = x[:64]
    x = x + 2.0 * cen[rng.integers(0, 64, size=4096)]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = x[rng.integers(0, 4096, size=8)] + 0.1 * rng.standard_normal((8, 384)).astype(np.float32)
    return x.astype(np.float32), (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16", "fp8"])
def test_unit_rows_every_step_is_a_best_choice(torch_mod, unit_rows, dtype):
    x, q = unit_rows
    idx = _ix().FlatIPIndex(384, dtype=dtype)
    idx.add(x)
    X = idx.reconstruct_n().astype(np.float64)                     # the stored rows
    qt = torch_mod.from_numpy(q).cuda()
    B, C, k = 8, 256, 32
    D0, I0 = idx.search(qt, C)
    ids, rel = _np(I0), _np(D0)
    for lam in (0.3, 0.7):
        D, I = idx.search_mmr(qt, k, C, lam)
        D2, I2 = idx.search_mmr(qt, k, C, lam)
        _same_bits((D, I), (D2, I2))                               # two runs: identical bits
        D, I = _np(D), _np(I)
        moved = 0
        for b in range(B):
            assert len(set(I[b].tolist())) == k and np.isin(I[b], ids[b]).all()
            pos = np.array([int(np.nonzero(ids[b] == i)[0][0]) for i in I[b]])
            assert np.array_equal(D[b].view(np.uint32), rel[b, pos].view(np.uint32))
            S = X[ids[b]] @ X[ids[b]].T
            worst = mm.step_valid(rel[b], S, pos, lam, TIE_TOL)
            print(f"{dtype} lambda={lam} query {b}: largest shortfall {worst:.3e} (tol {TIE_TOL:.1e})")
            moved += int((pos != np.arange(k)).sum())
        assert moved > 0                                           # the diversity term did decide picks


# -------------------------------------------------------------------------------------- retriever and pipeline
WORDS = ("neural network attention transformer language retrieval index vector query document "
         "learning model data system search rank score token embedding gpu memory").split()
PLANTED = "maximal marginal relevance picks results that differ from one another"
QUERY = "marginal relevance picks results that differ"


def _docs(n=200):
    rng = np.random.default_rng(3)
    docs = [" ".join(rng.choice(WORDS, size=int(rng.integers(4, 30)))) for _ in range(n)]
    for at in (17, 90, 151):
        docs[at] = PLANTED
    return docs


def _records_model(index, recs, key, k, lam):
    """Positions the model picks among the records ``recs`` (relevance: their ``key`` as f32; similarity: the stored
    rows in float64), and what step_valid needs."""
    ids = np.array([r["doc_id"] for r in recs])
    rel = np.array([r[key] for r in recs], dtype=np.float32)
    X = index.reconstruct_n().astype(np.float64)[ids]
    S = X @ X.T
    return ids, rel, S, mm.mmr_select(rel, S, k, lam)


def test_retriever_diversifies_the_dense_candidates(tmp_path):
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    cfg = dict(model_name="random:tiny", device="cuda", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
               use_fp16=False)
    r = Stage1Retriever(Stage1Config(enable_bm25=False, **cfg))
    r.add_documents(_docs())
    top_k = 5
    plain = r.search(QUERY, top_k)
    assert [x["doc_id"] for x in plain[:3]] == [17, 90, 151]                  # the three copies lead the plain list
    same = r.search(QUERY, top_k, mmr_lambda=1.0)
    assert same == plain
    wide = r.search(QUERY, min(1024, 4 * top_k))                              # the list the picks are chosen from
    ids, rel, S, picks = _records_model(r.faiss_index, wide, "stage1_score", top_k, 0.5)
    got = r.search(QUERY, top_k, mmr_lambda=0.5)
    got_ids = [x["doc_id"] for x in got]
    assert got_ids == ids[picks].tolist()
    assert got_ids[0] == 17 and len({17, 90, 151} & set(got_ids[:2])) == 1    # one copy in the first two places
    mm.step_valid(rel, S, [int(np.nonzero(ids == i)[0][0]) for i in got_ids], 0.5, TIE_TOL)
    by_id = {x["doc_id"]: x for x in wide}
    assert all(x == by_id[x["doc_id"]] for x in got)                          # the records are the plain ones
    many = r.search_many([QUERY, "gpu memory index", QUERY], top_k, mmr_lambda=0.5)
    for m, one in zip(many, (got, r.search("gpu memory index", top_k, mmr_lambda=0.5), got)):
        assert [x["doc_id"] for x in m] == [x["doc_id"] for x in one]
        # (the encoder pads a batch's queries to one length: the scores carry that noise, as in test_pipeline_gpu.py)
        np.testing.assert_allclose([x["score"] for x in m], [x["score"] for x in one], atol=1e-4)
    r.config.mmr_lambda = 0.5                                                 # the config's value is the default
    assert r.search(QUERY, top_k) == got and r.search(QUERY, top_k, mmr_lambda=1.0) == plain
    with pytest.raises(ValueError, match="mmr_lambda"):
        r.search(QUERY, top_k, mmr_lambda=1.5)
    fused = Stage1Retriever(Stage1Config(enable_bm25=True, **cfg))
    fused.add_documents(_docs())
    with pytest.raises(ValueError, match="BM25"):
        fused.search(QUERY, top_k, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="BM25"):
        fused.search_many([QUERY], top_k, mmr_lambda=0.5)
    assert len(fused.search(QUERY, top_k)) == top_k


def _pipeline(tmp_path, name, **extra):
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    pc = PipelineConfig(stage1_model="random:tiny", stage2_model="random:tiny", stage3_model="random:tiny",
                        device="cuda", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
                        log_file=str(tmp_path / f"{name}.log"), stage1_top_k=40, stage2_top_k=20, stage3_top_k=12,
                        stage1_use_fp16=False, stage2_use_fp16=False, stage3_use_fp16=False,
                        stage1_enable_bm25=False, **extra)
    p = RetrievalPipeline(config=pc)
    p.initialize_stages()
    p.add_documents(_docs())
    return p


def test_pipeline_diversifies_what_stage_three_returns(tmp_path):
    rec = _pipeline(tmp_path, "rec")
    arr = _pipeline(tmp_path, "arr", stage2_precompute_document_embeddings=True, stage3_cache_document_tokens=True)
    assert arr._arrays_ready() and not rec._arrays_ready()
    queries = [QUERY, "gpu memory index", "language retrieval system"]
    results = {}
    for name, p in (("rec", rec), ("arr", arr)):
        final = p.stage3.config.top_k_final
        for q in queries:
            plain = p.search(q, top_k=final)["results"]
            assert 5 < len(plain) <= final
            ids, rel, S, picks = _records_model(p.stage1.faiss_index, plain, "stage3_score", 5, 0.5)
            got = p.search(q, top_k=5, mmr_lambda=0.5)["results"]
            assert len(got) == 5
            pos = [int(np.nonzero(ids == x["doc_id"])[0][0]) for x in got]
            worst = mm.step_valid(rel, S, pos, 0.5, TIE_TOL)
            print(f"{name} {q!r}: picks {pos} model {picks} largest shortfall {worst:.3e}")
            by_id = {x["doc_id"]: x for x in plain}
            for x in got:                                              # the keys and scores they have anyway
                assert set(x) == set(by_id[x["doc_id"]]) and x["stage3_score"] == by_id[x["doc_id"]]["stage3_score"]
            assert p.search(q, top_k=5, mmr_lambda=1.0)["results"] == plain[:5]
            results[name, q] = (ids, rel, S, pos, got)
        many = p.search_many(queries, top_k=5, mmr_lambda=0.5)
        for q, m in zip(queries, many):                                # search_many equals search per query
            assert [x["doc_id"] for x in m["results"]] == [x["doc_id"] for x in results[name, q][4]]
        batch = p.batch_search(queries[:2], top_k=5, mmr_lambda=0.5)
        assert [[x["doc_id"] for x in b["results"]] for b in batch] == \
               [[x["doc_id"] for x in results[name, q][4]] for q in queries[:2]]
    # The record path and the array path agree: the array path's picks are best choices under the record path's
    # relevances too, up to twice the largest difference of the two paths' stage-3 scores (lambda <= 1 of it on each
    # side of a comparison).
    for q in queries:
        ids_r, rel_r, S_r, pos_r, got_r = results["rec", q]
        ids_a, rel_a, _, pos_a, got_a = results["arr", q]
        assert sorted(ids_r.tolist()) == sorted(ids_a.tolist())
        ra = dict(zip(ids_a.tolist(), rel_a.tolist()))
        delta = max(abs(ra[i] - s) for i, s in zip(ids_r.tolist(), rel_r.tolist()))
        pos = [int(np.nonzero(ids_r == x["doc_id"])[0][0]) for x in got_a]
        mm.step_valid(rel_r, S_r, pos, 0.5, TIE_TOL + 2.0 * delta)
    rec.config.mmr_lambda = 0.5                                        # the config's value is the default
    assert [x["doc_id"] for x in rec.search(QUERY, top_k=5)["results"]] == [x["doc_id"] for x in results["rec", QUERY][4]]
