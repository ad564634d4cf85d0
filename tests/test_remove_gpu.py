"""Removal (FlatIPIndex.remove_ids / compact) on the GPU.  After remove_ids(D), search(q, k) is the filtered search of
the live rows bit for bit — on the same index (allowed = ~D) and on a twin index from which nothing was removed
(allowed = live) — on every path: synchronous, classic, one-launch requested, asynchronous coalesced (wide and
LDS-resident passes), filtered, dense (small N, k > 2048), k > 16384, and f16 / bf16 / f32 storage.  compact() gives
the index that adding only the live rows would have built."""
import numpy as np
import pytest

from helpers import make_corpus

pytestmark = pytest.mark.gpu

NEG = -3.0e38


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _index(d, dtype, rows):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(rows)
    return idx


def _same(a, b):
    Da, Ia = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in a)
    Db, Ib = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in b)
    assert np.array_equal(Ia, Ib)
    assert np.array_equal(Da.view(np.uint32), Db.view(np.uint32))


def _removed_set(n, frac, rng):
    return np.flatnonzero(rng.random(n) < frac)


@pytest.mark.parametrize("dtype,d", [("f16", 384), ("bf16", 768), ("f16", 1024), ("f32", 384), ("bf16", 1024)])
@pytest.mark.parametrize("mode", ["sync", "classic", "one_launch"])
def test_remove_equals_filtered(dtype, d, mode):
    n, k = 100_000, 100
    rng = np.random.default_rng(d)
    corpus = make_corpus(n, d, seed=21, dtype=dtype)
    q = make_corpus(40, d, seed=22, dtype=dtype)
    idx, twin = _index(d, dtype, corpus), _index(d, dtype, corpus)
    D = _removed_set(n, 0.1, rng)
    assert idx.remove_ids(D) == D.size
    assert idx.nlive == n - D.size and idx.ntotal == n
    live = np.ones(n, bool)
    live[D] = False
    kw = {"classic": mode == "classic", "one_launch": mode == "one_launch"}
    got = idx.search(q, k, **kw)
    assert not np.isin(got[1], D).any()
    _same(got, idx.search(q, k, allowed=live))
    _same(got, twin.search(q, k, allowed=live))
    if dtype != "f32":
        assert idx.last_search_info()["path"] == "filter"
    idx.close()
    twin.close()


@pytest.mark.parametrize("wide", [True, False])
def test_async_coalesced_across_removal(torch_mod, wide):
    torch = torch_mod
    n, d, k = 100_000, 768, 100
    corpus = make_corpus(n, d, seed=31, dtype="f16")
    idx, twin = _index(d, "f16", corpus), _index(d, "f16", corpus)
    for x in (idx, twin):
        x.classic_filter = True   # (the five-launch path is the one that coalesces at this size)
        x.wide_passes = wide
    qs = [torch.from_numpy(make_corpus(32, d, seed=40 + i, dtype="f16")).cuda().half() for i in range(6)]
    before = [idx.search(q, k, async_=True) for q in qs[:3]]   # held by the coalesced queue
    D = _removed_set(n, 0.05, np.random.default_rng(5))
    idx.remove_ids(D)
    after = [idx.search(q, k, async_=True) for q in qs[3:]]
    idx.finish()
    live = np.ones(n, bool)
    live[D] = False
    for q, r in zip(qs[:3], before):
        _same(r, twin.search(q, k))
    for q, r in zip(qs[3:], after):
        assert not np.isin(r[1].cpu().numpy(), D).any()
        _same(r, twin.search(q, k, allowed=live))
    idx.close()
    twin.close()


def test_filtered_and_removed():
    n, d, k = 100_000, 384, 64
    rng = np.random.default_rng(7)
    corpus = make_corpus(n, d, seed=51, dtype="f16")
    q = make_corpus(20, d, seed=52, dtype="f16")
    idx, twin = _index(d, "f16", corpus), _index(d, "f16", corpus)
    D = _removed_set(n, 0.2, rng)
    idx.remove_ids(D)
    live = np.ones(n, bool)
    live[D] = False
    user = rng.random(n) < 0.3
    masks = [user if i % 2 else None for i in range(20)]
    got = idx.search(q, k, allowed=masks)
    want = twin.search(q, k, allowed=[(m & live) if m is not None else live for m in masks])
    _same(got, want)
    idx.close()
    twin.close()


@pytest.mark.parametrize("n,k", [(5000, 50), (100_000, 3000), (40_000, 20_000)])
def test_dense_and_large_k(n, k):
    d = 128
    rng = np.random.default_rng(n)
    corpus = make_corpus(n, d, seed=61, dtype="bf16")
    q = make_corpus(5, d, seed=62, dtype="bf16")
    idx, twin = _index(d, "bf16", corpus), _index(d, "bf16", corpus)
    D = _removed_set(n, 0.3, rng)
    idx.remove_ids(D)
    live = np.ones(n, bool)
    live[D] = False
    got = idx.search(q, k)
    _same(got, idx.search(q, k, allowed=live))
    _same(got, twin.search(q, k, allowed=live))
    kk = min(k, int(live.sum()))
    assert (got[1][:, kk:] == -1).all() and (got[0][:, kk:] <= NEG).all()
    assert not np.isin(got[1], D).any()
    idx.close()
    twin.close()


def test_adversarial_removal_stays_on_the_filter_path():
    n, d, k = 400_000, 128, 1000
    corpus = make_corpus(n, d, seed=71, dtype="f16")
    q = make_corpus(64, d, seed=72, dtype="f16")
    idx, twin = _index(d, "f16", corpus), _index(d, "f16", corpus)
    _, I0 = idx.search(q, k)
    D = np.unique(I0.reshape(-1))
    idx.remove_ids(D)
    live = np.ones(n, bool)
    live[D] = False
    got = idx.search(q, k)
    assert idx.last_search_info()["path"] == "filter"
    assert not np.isin(got[1], D).any()
    _same(got, twin.search(q, k, allowed=live))
    idx.close()
    twin.close()


def test_remove_everything_then_add():
    n, d, k = 50_000, 128, 10
    corpus = make_corpus(n, d, seed=81, dtype="f16")
    q = make_corpus(4, d, seed=82, dtype="f16")
    idx = _index(d, "f16", corpus)
    idx.set_id_offset(1000)
    assert idx.remove_ids(np.arange(n) + 1000) == n
    assert idx.nlive == 0
    D, I = idx.search(q, k)
    assert (I == -1).all() and (D <= NEG).all()
    extra = make_corpus(100, d, seed=83, dtype="f16")
    idx.add(extra)
    assert idx.ntotal == n + 100 and idx.nlive == 100
    D, I = idx.search(q, k)
    ref = _index(d, "f16", extra)
    Dr, Ir = ref.search(q, k)
    assert np.array_equal(I, Ir + n + 1000)
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32))
    idx.close()
    ref.close()


def test_double_and_unknown_ids():
    n, d = 3000, 64
    idx = _index(d, "f16", make_corpus(n, d, seed=91, dtype="f16"))
    assert idx.remove_ids([5, 5, 7, -1, n, 10 ** 12]) == 2
    assert idx.remove_ids([5, 7]) == 0
    assert idx.remove_ids(np.array([], dtype=np.int64)) == 0
    assert idx.remove_ids([8]) == 1
    assert idx.nlive == n - 3
    m = idx.live_mask()
    assert m.sum() == n - 3 and not m[[5, 7, 8]].any()
    idx.close()


@pytest.mark.parametrize("dtype,n,d", [("f16", 100_000, 384), ("f32", 20_000, 96), ("bf16", 1_500_000, 128)])
def test_compact_equals_fresh_index(dtype, n, d):
    rng = np.random.default_rng(n + d)
    corpus = make_corpus(n, d, seed=101, dtype=dtype)
    q = make_corpus(16, d, seed=102, dtype=dtype)
    k = 100
    idx = _index(d, dtype, corpus)
    D = _removed_set(n, 0.01, rng)
    idx.remove_ids(D)
    live = np.ones(n, bool)
    live[D] = False
    pre = idx.search(q, k)
    old2new = idx.compact()
    assert idx.ntotal == idx.nlive == int(live.sum())
    assert np.array_equal(old2new[live], np.arange(int(live.sum()))) and (old2new[~live] == -1).all()
    fresh = _index(d, dtype, corpus[live])
    if n <= 100_000:
        assert np.array_equal(idx.reconstruct_n(), fresh.reconstruct_n())
    else:
        assert np.array_equal(idx.reconstruct_n(idx.ntotal - 1000, 1000), corpus[live][-1000:])
    got = idx.search(q, k)
    _same(got, fresh.search(q, k))
    assert np.array_equal(got[1], np.where(pre[1] >= 0, old2new[np.maximum(pre[1], 0)], -1))
    assert np.array_equal(got[0].view(np.uint32), pre[0].view(np.uint32))
    # adding after compaction continues from the new ntotal, and the padding of the last block was cleared
    extra = make_corpus(50, d, seed=103, dtype=dtype)
    idx.add(extra)
    fresh.add(extra)
    _same(idx.search(q, k), fresh.search(q, k))
    idx.close()
    fresh.close()


@pytest.mark.parametrize("dt,d", [("f16", 384), ("bf16", 768)])
def test_ivf_remove_equals_filtered_flat_search(dt, d):
    """The IVF identity (ivf.search == flat.search(allowed = rows of the probed lists)) with the live rows ANDed in."""
    import torch
    from test_ivf_gpu import build, dev, mixture, probed_masks, row_lists, same
    nlist = 50
    x = mixture(40000, d, seed=4)
    ivf, flat = build(x, d, nlist, dt)
    lists = row_lists(ivf)
    rng = np.random.default_rng(d)
    D = np.flatnonzero(rng.random(x.shape[0]) < 0.2)
    qs = dev(mixture(64, d, seed=12), dt)
    _, I0 = ivf.search(qs, 100, nprobe=10)
    D = np.union1d(D, I0.cpu().numpy()[:, :50].reshape(-1))   # each query's best rows too
    assert ivf.remove_ids(np.concatenate([D, D[:10], [-5, 10 ** 9]])) == D.size
    live = np.ones(x.shape[0], bool)
    live[D] = False
    assert ivf.nlive == live.sum() and ivf.ntotal == x.shape[0]
    assert np.array_equal(np.bincount(lists[live], minlength=nlist), ivf.list_sizes())
    for B in (1, 64):
        q = qs[:B]
        for p in (1, 10, nlist):
            masks = [m & live for m in probed_masks(ivf, q, p, lists)]
            for k in (10, 1000, 2048):
                got = ivf.search(q, k, nprobe=p)
                assert not np.isin(got[1].cpu().numpy(), D).any()
                same(got, flat.search(q, k, allowed=masks))
    # adding after a removal: the new rows are found, the holes stay empty
    extra = mixture(500, d, seed=99)
    ivf.add(dev(extra, dt))
    flat.add(dev(extra, dt))
    live = np.concatenate([live, np.ones(500, bool)])
    lists = row_lists(ivf)
    masks = [m & live for m in probed_masks(ivf, qs, nlist, lists)]
    same(ivf.search(qs, 100, nprobe=nlist), flat.search(qs, 100, allowed=masks))
    ivf.close()
    flat.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ pipeline
def _pipeline(tmp_path, **extra):
    from test_pipeline_gpu import _build
    return _build("cuda", tmp_path, doubles=False, stage2_precompute_document_embeddings=True,
                  stage3_cache_document_tokens=True, **extra)


PQ = ["neural networks attention", "language retrieval system", "gpu memory index", "token embedding search"]
STAGES = (("stage1_results", "stage1_score"), ("stage2_results", "stage2_score"), ("results", "stage3_score"))


@pytest.mark.parametrize("bm25", [False, True])
@pytest.mark.parametrize("store", ["bf16", "fp8"])
def test_pipeline_remove_then_compact(tmp_path, bm25, store):
    from test_pipeline_gpu import _corpus
    docs = _corpus()
    p = _pipeline(tmp_path, stage1_enable_bm25=bm25, stage2_token_store_dtype=store)
    p.add_documents(docs)
    first = p.search_many(PQ)
    gone = sorted({r["doc_id"] for res in first for r in res["stage1_results"][:10]} | {0, 5, len(docs) - 1})
    assert p.remove_documents(gone + gone[:3]) == len(gone)
    info = p.get_pipeline_info()["documents"]
    assert info == {"total": len(docs), "removed": len(gone), "live": len(docs) - len(gone)}
    # no stage returns a removed document: arrays path (search_many), record path (search, filtered search_many)
    runs = [p.search_many(PQ), [p.search(q) for q in PQ], p.search_many(PQ, filter=lambda md: True)]
    for results in runs:
        for res in results:
            for stage, _ in STAGES:
                assert not {r["doc_id"] for r in res[stage]} & set(gone), stage
    if bm25:
        return
    # compaction: the dense-only results before it, renumbered, with bit-identical scores at every stage
    before = p.search_many(PQ)
    old2new = p.compact()
    assert (old2new[gone] == -1).all() and len(p.stage1.documents) == len(docs) - len(gone)
    assert p.stage1.faiss_index.ntotal == len(docs) - len(gone)
    after = p.search_many(PQ)
    for a, b in zip(before, after):
        for stage, key in STAGES:
            assert [old2new[r["doc_id"]] for r in a[stage]] == [r["doc_id"] for r in b[stage]], stage
            assert [r[key] for r in a[stage]] == [r[key] for r in b[stage]], stage
            assert all(p.stage1.documents[r["doc_id"]] == r["document"] for r in b[stage])


def test_pipeline_save_load_keeps_tombstones(tmp_path):
    from test_pipeline_gpu import _corpus
    docs = _corpus(120)
    p = _pipeline(tmp_path, stage1_enable_bm25=True)
    p.add_documents(docs)
    p.remove_documents([1, 2, 3, 50])
    path = str(tmp_path / "i" / "pipe.json")
    p.save_index(path)
    q = _pipeline(tmp_path, stage1_enable_bm25=True)
    q.load_index(path)
    assert q.get_pipeline_info()["documents"]["removed"] == 4
    assert q.stage1.faiss_index.nlive == len(docs) - 4
    for a, b in zip(p.search_many(PQ), q.search_many(PQ)):
        assert [r["doc_id"] for r in a["results"]] == [r["doc_id"] for r in b["results"]]
        assert not {r["doc_id"] for r in b["stage1_results"]} & {1, 2, 3, 50}


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("frac", [0.001, 0.3])
def test_async_coalesced_passes_keep_coalescing_after_removal(torch_mod, dtype, wide, frac):
    """With removed rows, asynchronous batches still join the coalesced passes (their tombstone instantiations): no
    call goes through the filtered path, and every result equals the filtered search of the live rows."""
    torch = torch_mod
    n, d, k = 100_000, 768, 100
    corpus = make_corpus(n, d, seed=33, dtype=dtype)
    idx, twin = _index(d, dtype, corpus), _index(d, dtype, corpus)
    idx.classic_filter = True   # (the five-launch path is the one that coalesces at this size)
    idx.wide_passes = wide
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    qs = [torch.from_numpy(make_corpus(64, d, seed=60 + i, dtype=dtype)).cuda().to(tdt) for i in range(7)]
    D = _removed_set(n, frac, np.random.default_rng(9))
    # each batch's own best rows go too (the thresholds count live sample rows only)
    D = np.union1d(D, np.concatenate([idx.search(q, 20)[1].cpu().numpy().reshape(-1) for q in qs[:2]]))
    idx.remove_ids(D)
    live = np.ones(n, bool)
    live[D] = False
    outs = [idx.search(q, k, async_=True) for q in qs]
    idx.finish()
    assert idx.last_filter_info()["filter_passes"] == 0   # nothing took the filtered path
    for q, r in zip(qs, outs):
        assert not np.isin(r[1].cpu().numpy(), D).any()
        _same(r, twin.search(q, k, allowed=live))
    idx.close()
    twin.close()


# (d, groups, kernel family of the pass): every tombstone group count once, scan_multi_kernel 1..4, scan_wide_kernel 2..6
PARTIAL = [(768, 3, "multi"), (768, 4, "wide"), (768, 5, "wide"), (1024, 3, "wide"), (1536, 1, "multi"),
           (1536, 2, "wide"), (1536, 6, "wide"), (768, 2, "multi"), (384, 4, "multi")]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d,groups,family", PARTIAL)
def test_partial_tombstone_passes(torch_mod, dtype, d, groups, family):
    """Single-group batches on an index with removed rows, flushed at finish() as one tombstone pass: LDS-resident
    where the images fit, wide otherwise (test_partial_wide_passes of test_coalesce_wide_gpu.py, after a removal)."""
    from tristage_rag_amd import _lib
    torch = torch_mod
    n, k = 100_000, 100   # the floor below which the five-launch path does not coalesce
    code = _lib.TS_F16 if dtype == "f16" else _lib.TS_BF16
    assert (groups <= _lib.load().ts_coalesce_groups(d, code)) == (family == "multi")
    corpus = make_corpus(n, d, seed=35, dtype=dtype)
    idx, twin = _index(d, dtype, corpus), _index(d, dtype, corpus)
    idx.classic_filter = True
    idx.wide_passes = True
    D = _removed_set(n, 0.05, np.random.default_rng(11))
    assert idx.remove_ids(D) == D.size
    live = np.ones(n, bool)
    live[D] = False
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    qs = [torch.from_numpy(make_corpus(32, d, seed=260 + i, dtype=dtype)).cuda().to(tdt) for i in range(groups)]
    idx.set_profiling(True, every=1)
    idx.timings(reset=True)
    outs = [idx.search(q, k, async_=True) for q in qs]
    redone = idx.finish()
    torch.cuda.synchronize()
    launches = idx.timings(reset=True)["filter_scan"][1]
    idx.set_profiling(False)
    assert redone == []
    assert idx.last_filter_info()["filter_passes"] == 0   # nothing took the filtered path
    assert launches == 1
    for q, r in zip(qs, outs):
        assert not np.isin(r[1].cpu().numpy(), D).any()
        _same(r, twin.search(q, k, allowed=live))
    idx.close()
    twin.close()
