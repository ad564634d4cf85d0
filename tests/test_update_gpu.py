"""Update in place (FlatIPIndex.update_rows, IVFFlatIndex.update_rows, RetrievalPipeline.update_documents) on the
GPU.  After update_rows(U, Y) a flat index holds the bytes a fresh index of the final matrix holds, so reconstruct_n and
every search path agree with that fresh index bit for bit; the IVF index keeps its search identity against the flat
index of the final matrix; the pipeline leaves untouched documents untouched at every stage and agrees with a pipeline
built from the final documents under the criterion of test_pipeline_gpu_matches_cpu_doubles."""
import numpy as np
import pytest

from helpers import make_corpus

pytestmark = pytest.mark.gpu


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


def _update_set(n, rng, frac=0.01, blocks=3, block0=7):
    """1 % random ids, one whole aligned range of `blocks` row blocks, the first and the last row; shuffled, so that
    the rows of a fully updated block arrive in no particular order."""
    ids = np.union1d(np.flatnonzero(rng.random(n) < frac), np.arange(32 * block0, 32 * (block0 + blocks)))
    ids = np.union1d(ids, [0, n - 1])
    return rng.permutation(ids)


def _updated_pair(n, d, dtype, seed, normalize=False):
    """(updated index, fresh index of the final matrix, U, final matrix)"""
    rng = np.random.default_rng(seed)
    X = make_corpus(n, d, seed=seed, dtype=dtype)
    U = _update_set(n, rng)
    Y = make_corpus(U.size, d, seed=seed + 1, dtype=dtype)
    if normalize:   # unnormalised f32 rows: the index normalises, as add(normalize=True) does
        X = (X * rng.uniform(0.5, 3.0, size=(n, 1))).astype(np.float32)
        Y = (Y * rng.uniform(0.5, 3.0, size=(U.size, 1))).astype(np.float32)
    from tristage_rag_amd.index import FlatIPIndex
    idx, fresh = FlatIPIndex(d, dtype=dtype), FlatIPIndex(d, dtype=dtype)
    idx.add(X, normalize=normalize)
    idx.update_rows(U, Y, normalize=normalize)
    F = X.copy()
    F[U] = Y
    fresh.add(F, normalize=normalize)
    assert idx.ntotal == idx.nlive == n
    return idx, fresh, U, F


# ------------------------------------------------------------------ 1. flat: equals a fresh index
@pytest.mark.parametrize("dtype,d", [("f16", 384), ("bf16", 768), ("f16", 1024), ("f32", 384)])
@pytest.mark.parametrize("mode", ["sync", "classic", "one_launch"])
def test_update_equals_fresh_index(dtype, d, mode):
    n = 100_003
    idx, fresh, U, _ = _updated_pair(n, d, dtype, seed=200 + d)
    assert np.array_equal(idx.reconstruct_n(), fresh.reconstruct_n())
    q = make_corpus(40, d, seed=23, dtype=dtype)
    kw = {"classic": mode == "classic", "one_launch": mode == "one_launch"}
    for k in (10, 1000):
        _same(idx.search(q, k, **kw), fresh.search(q, k, **kw))
    idx.close()
    fresh.close()


def test_update_normalize_from_f32_rows():
    n, d = 50_001, 384
    idx, fresh, U, _ = _updated_pair(n, d, "f16", seed=77, normalize=True)
    assert np.array_equal(idx.reconstruct_n(), fresh.reconstruct_n())
    q = make_corpus(16, d, seed=24, dtype="f16")
    for k in (10, 1000):
        _same(idx.search(q, k), fresh.search(q, k))
    idx.close()
    fresh.close()


def test_update_from_device_tensors(torch_mod):
    """CUDA tensors in (f32 rows into bf16 storage), as add takes them; the ids ascending but not one run"""
    torch = torch_mod
    n, d = 40_000, 768
    rng = np.random.default_rng(3)
    X = make_corpus(n, d, seed=5, dtype="f32")
    U = np.sort(_update_set(n, rng))
    Y = make_corpus(U.size, d, seed=6, dtype="f32")
    idx, F = _index(d, "bf16", torch.from_numpy(X).cuda()), X.copy()
    idx.update_rows(torch.from_numpy(U).cuda(), torch.from_numpy(Y).cuda())
    F[U] = Y
    fresh = _index(d, "bf16", torch.from_numpy(F).cuda())
    assert np.array_equal(idx.reconstruct_n(), fresh.reconstruct_n())
    idx.close()
    fresh.close()


@pytest.mark.parametrize("dtype,d", [("f16", 384), ("f32", 96), ("bf16", 1024)])
@pytest.mark.parametrize("start,count", [(32 * 5, 32 * 40), (17, 1000), (99_990, 13)])
@pytest.mark.parametrize("normalize", [False, True])
def test_update_contiguous_range(torch_mod, dtype, d, start, count, normalize):
    """one ascending run of ids (the bulk re-embed of a range), aligned to row blocks or not, up to the last row: it is
    written by add's own relayout at its rows, and the rows around it keep their bytes"""
    torch = torch_mod
    n = 100_003
    rng = np.random.default_rng(start + d)
    X = make_corpus(n, d, seed=start, dtype=dtype)
    Y = make_corpus(count, d, seed=start + 1, dtype=dtype)
    if normalize:
        X = (X * rng.uniform(0.5, 3.0, size=(n, 1))).astype(np.float32)
        Y = (Y * rng.uniform(0.5, 3.0, size=(count, 1))).astype(np.float32)
    from tristage_rag_amd.index import FlatIPIndex
    a, b, fresh = (FlatIPIndex(d, dtype=dtype) for _ in range(3))
    for x in (a, b):
        x.add(X, normalize=normalize)
    U = np.arange(start, start + count)
    a.update_rows(U, Y, normalize=normalize)                                               # host rows
    b.update_rows(torch.from_numpy(U).cuda(), torch.from_numpy(Y).cuda(), normalize=normalize)   # device rows
    X[U] = Y
    fresh.add(X, normalize=normalize)
    want = fresh.reconstruct_n()
    assert np.array_equal(a.reconstruct_n(), want) and np.array_equal(b.reconstruct_n(), want)
    q = make_corpus(8, d, seed=3, dtype=dtype)
    _same(a.search(q, 100), fresh.search(q, 100))
    for x in (a, b, fresh):
        x.close()


@pytest.mark.parametrize("wide", [True, False])
def test_update_async_coalesced_equals_fresh(torch_mod, wide):
    torch = torch_mod
    n, d = 100_003, 768
    idx, fresh, U, _ = _updated_pair(n, d, "f16", seed=31)
    for x in (idx, fresh):
        x.classic_filter = True   # (the five-launch path is the one that coalesces at this size)
        x.wide_passes = wide
    qs = [torch.from_numpy(make_corpus(32, d, seed=40 + i, dtype="f16")).cuda().half() for i in range(4)]
    for k in (10, 1000):
        got = [idx.search(q, k, async_=True) for q in qs]
        idx.finish()
        for q, r in zip(qs, got):
            _same(r, fresh.search(q, k))
    idx.close()
    fresh.close()


def test_update_filtered_search_equals_fresh():
    n, d = 100_003, 384
    idx, fresh, U, _ = _updated_pair(n, d, "f16", seed=51)
    rng = np.random.default_rng(8)
    q = make_corpus(20, d, seed=52, dtype="f16")
    user = rng.random(n) < 0.3
    user[U[:50]] = True
    masks = [user if i % 2 else None for i in range(20)]
    for k in (10, 1000):
        _same(idx.search(q, k, allowed=masks), fresh.search(q, k, allowed=masks))
    idx.close()
    fresh.close()


@pytest.mark.parametrize("n,k", [(5003, 50), (20_003, 3000), (40_003, 20_000)])
def test_update_dense_and_large_k(n, k):
    """the dense path (n < 32768, also with k > 2048) and k > 16384"""
    d = 128
    idx, fresh, U, _ = _updated_pair(n, d, "bf16", seed=n)
    q = make_corpus(5, d, seed=62, dtype="bf16")
    _same(idx.search(q, k), fresh.search(q, k))
    idx.close()
    fresh.close()


def test_update_beyond_one_staging_chunk():
    """1.5 M rows of bf16 x 128: the staging tile of one chunk holds 64 MiB / 256 B = 262144 rows, so a range of
    300 000 ids plus the random ones takes several chunks (host rows: at most 64 MiB of them per chunk as well).  The
    sorted ids are cut into pieces of about 2048 and the pieces shuffled, so every chunk holds whole row blocks (pieces
    from inside the range) and single rows (pieces of random ids) from all over the index."""
    n, d, k = 1_500_003, 128, 100
    rng = np.random.default_rng(11)
    X = make_corpus(n, d, seed=101, dtype="bf16")
    U = np.union1d(np.flatnonzero(rng.random(n) < 0.01), np.arange(32 * 1000, 32 * 1000 + 300_000))
    U = np.union1d(U, [0, n - 1])
    pieces = np.array_split(U, max(1, U.size // 2048))   # not sorted: every chunk holds ids from the whole range
    U = np.concatenate([pieces[i] for i in rng.permutation(len(pieces))])
    Y = make_corpus(U.size, d, seed=102, dtype="bf16")
    idx = _index(d, "bf16", X)
    idx.update_rows(U, Y)
    X[U] = Y
    # and one ascending run of host rows longer than a host staging chunk (64 MiB / 512 B = 131072 rows), unaligned
    R = np.arange(n // 2 - 13, n // 2 - 13 + 300_007)
    Z = make_corpus(R.size, d, seed=104, dtype="bf16")
    idx.update_rows(R, Z)
    X[R] = Z
    fresh = _index(d, "bf16", X)
    for i0 in (0, 32 * 1000 - 500, n // 2 - 1000, n // 2 + 300_007 - 2000, n - 3000):
        assert np.array_equal(idx.reconstruct_n(i0, 3000), fresh.reconstruct_n(i0, 3000))
    sample = rng.choice(U, 2000, replace=False)
    for i in sample[:200]:
        assert np.array_equal(idx.reconstruct_n(int(i), 1), fresh.reconstruct_n(int(i), 1))
    q = make_corpus(16, d, seed=103, dtype="bf16")
    for kk in (10, 1000):
        _same(idx.search(q, kk), fresh.search(q, kk))
    idx.close()
    fresh.close()


# ------------------------------------------------------------------ 2. flat: ordering
@pytest.mark.parametrize("wide", [True, False])
def test_async_coalesced_across_update(torch_mod, wide):
    torch = torch_mod
    n, d, k = 100_000, 768, 100
    rng = np.random.default_rng(5)
    X = make_corpus(n, d, seed=31, dtype="f16")
    idx, old = _index(d, "f16", X), _index(d, "f16", X)
    qs = [torch.from_numpy(make_corpus(32, d, seed=40 + i, dtype="f16")).cuda().half() for i in range(6)]
    # the rows the first batches would return are among the updated ones, so that an update seen early shows
    U = np.union1d(_update_set(n, rng), np.unique(old.search(qs[0], 20)[1].cpu().numpy()))
    Y = make_corpus(U.size, d, seed=33, dtype="f16")
    F = X.copy()
    F[U] = Y
    new = _index(d, "f16", F)
    for x in (idx, old, new):
        x.classic_filter = True   # (the five-launch path is the one that coalesces at this size)
        x.wide_passes = wide
    before = [idx.search(q, k, async_=True) for q in qs[:3]]   # held by the coalesced queue
    idx.update_rows(U, Y)
    after = [idx.search(q, k, async_=True) for q in qs[3:]]
    idx.finish()
    for q, r in zip(qs[:3], before):
        _same(r, old.search(q, k))
    for q, r in zip(qs[3:], after):
        _same(r, new.search(q, k))
    for x in (idx, old, new):
        x.close()


# ------------------------------------------------------------------ 3. flat: with tombstones
def test_update_with_tombstones_and_refusals():
    n, d, k = 100_003, 384, 100
    rng = np.random.default_rng(9)
    X = make_corpus(n, d, seed=71, dtype="f16")
    q = make_corpus(20, d, seed=72, dtype="f16")
    idx = _index(d, "f16", X)
    idx.set_id_offset(1000)
    D = np.flatnonzero(rng.random(n) < 0.1)
    idx.remove_ids(D + 1000)
    live = np.ones(n, bool)
    live[D] = False
    U = _update_set(n, rng)
    U = U[live[U]]
    Y = make_corpus(U.size, d, seed=73, dtype="f16")
    idx.update_rows(U + 1000, Y)
    assert idx.ntotal == n and idx.nlive == n - D.size
    F = X.copy()
    F[U] = Y
    fresh = _index(d, "f16", F)
    fresh.set_id_offset(1000)
    for kk in (10, 1000):
        _same(idx.search(q, kk), fresh.search(q, kk, allowed=live))
    # removed rows were not rewritten, live ones hold the new bytes
    rec = idx.reconstruct_n()
    assert np.array_equal(rec[live], fresh.reconstruct_n()[live])
    assert np.array_equal(rec[D], X[D].astype(np.float32))
    # refusals: nothing is written
    ok = np.flatnonzero(live)[:5] + 1000
    Z = make_corpus(6, d, seed=74, dtype="f16")
    for bad in (int(D[3]) + 1000, n + 1000, 10 ** 12, 999, -1, int(ok[2])):
        with pytest.raises(ValueError) as e:
            idx.update_rows(np.concatenate([ok, [bad]]), Z)
        assert str(bad) in str(e.value)
        assert np.array_equal(idx.reconstruct_n(), rec)
    with pytest.raises(ValueError):
        idx.update_rows(ok, Z)   # six rows for five ids
    assert idx.nlive == n - D.size
    # compaction after updates: a fresh index of the final live rows
    idx.compact()
    ref = _index(d, "f16", F[live])
    ref.set_id_offset(1000)
    assert np.array_equal(idx.reconstruct_n(), ref.reconstruct_n())
    _same(idx.search(q, k), ref.search(q, k))
    for x in (idx, fresh, ref):
        x.close()


# ------------------------------------------------------------------ 4. IVF
@pytest.mark.parametrize("dt,d", [("f16", 384), ("bf16", 768)])
def test_ivf_update_keeps_the_search_identity(dt, d):
    import torch
    from tristage_rag_amd.index import IVFFlatIndex
    from test_ivf_gpu import build, dev, mixture, probed_masks, row_lists, same
    nlist = 50
    big = mixture(42000, d, seed=4)
    x = big[:40000].copy()
    ivf, flat = build(x, d, nlist, dt)
    rng = np.random.default_rng(d)
    U = rng.choice(40000, 2000, replace=False)
    Y = big[40000:]
    before = row_lists(ivf)
    ivf.update_rows(U, dev(Y, dt))
    flat.update_rows(U, dev(Y, dt))
    x[U] = Y
    lists = row_lists(ivf)
    # a condition on the input, not on the feature: the new rows land all over the trained lists
    assert (before[U] != lists[U]).mean() >= 0.5
    assert ivf.ntotal == 40000 and ivf.nlive == 40000
    fresh = IVFFlatIndex(d, nlist, dtype=dt)
    fresh.set_centroids(ivf.centroids)
    fresh.add(dev(x, dt))
    assert np.array_equal(ivf.list_sizes(), fresh.list_sizes())
    assert np.array_equal(ivf.reconstruct_n(), fresh.reconstruct_n())
    assert np.array_equal(np.bincount(lists, minlength=nlist), ivf.list_sizes())
    qs = dev(mixture(64, d, seed=12), dt)

    def identity(live=None):
        ls = row_lists(ivf)
        for B in (1, 64):
            q = qs[:B]
            for p in (1, 10, nlist):
                masks = probed_masks(ivf, q, p, ls)
                if live is not None:
                    masks = [m & live for m in masks]
                for k in (10, 1000, 2048):
                    same(ivf.search(q, k, nprobe=p), flat.search(q, k, allowed=masks))

    identity()
    # the same ids again, in a second call: one copy of each row
    Y2 = mixture(2000, d, seed=77)[:500]
    ivf.update_rows(U[:500], dev(Y2, dt))
    flat.update_rows(U[:500], dev(Y2, dt))
    assert ivf.nlive == 40000
    assert np.array_equal(np.bincount(row_lists(ivf), minlength=nlist), ivf.list_sizes())
    identity()
    # after a removal: updating a removed row raises and changes nothing
    D = np.union1d(rng.choice(40000, 3000, replace=False), U[:100])
    assert ivf.remove_ids(D) == D.size
    live = np.ones(40000, bool)
    live[D] = False
    rec, sizes = ivf.reconstruct_n(), ivf.list_sizes()
    keep = np.flatnonzero(live)[:7]
    for bad in (int(D[5]), 40000, -3, int(keep[0])):
        with pytest.raises(ValueError) as e:
            ivf.update_rows(np.concatenate([keep, [bad]]), dev(Y2[:8], dt))
        assert str(bad) in str(e.value)
        assert np.array_equal(ivf.reconstruct_n(), rec) and np.array_equal(ivf.list_sizes(), sizes)
    V = np.flatnonzero(live)[::37]
    Y3 = mixture(V.size + 100, d, seed=78)[:V.size]
    ivf.update_rows(V, dev(Y3, dt))
    flat.update_rows(V, dev(Y3, dt))
    assert ivf.nlive == int(live.sum())
    assert np.array_equal(np.bincount(row_lists(ivf)[live], minlength=nlist), ivf.list_sizes())
    identity(live)
    # and after an add
    extra = mixture(500, d, seed=99)
    ivf.add(dev(extra, dt))
    flat.add(dev(extra, dt))
    live = np.concatenate([live, np.ones(500, bool)])
    identity(live)
    # updates after the add: ids of the add (the part of id2slot and the blocks it grew) mixed with old live ids,
    # rows of another mixture seed, so that content and lists change
    old_live = np.flatnonzero(live[:40000])
    W = rng.permutation(np.concatenate([rng.choice(np.arange(40000, 40500), 200, replace=False),
                                        rng.choice(old_live, 200, replace=False), [40000, 40499]]))
    W = W[np.sort(np.unique(W, return_index=True)[1])]
    Y4 = mixture(W.size + 50, d, seed=123)[:W.size]
    lists_before = row_lists(ivf)
    nlive = ivf.nlive
    ivf.update_rows(W, dev(Y4, dt))
    flat.update_rows(W, dev(Y4, dt))
    assert ivf.nlive == nlive == int(live.sum()) and ivf.ntotal == 40500
    lists_after = row_lists(ivf)
    assert (lists_before[W] != lists_after[W]).mean() >= 0.5   # (a condition on the input, as above)
    assert np.array_equal(np.bincount(lists_after[live], minlength=nlist), ivf.list_sizes())
    rec = ivf.reconstruct_n()
    assert np.array_equal(rec[W], flat.reconstruct_n()[W])
    identity(live)
    for i in (ivf, flat, fresh):
        i.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ pipeline
def _pipeline(tmp_path, ivf=False, **extra):
    from test_pipeline_gpu import _build
    p = _build("cuda", tmp_path, doubles=False, stage2_precompute_document_embeddings=True,
               stage3_cache_document_tokens=True, **extra)
    if ivf:   # every list probed: the result does not depend on where k-means put its centres
        c = p.stage1.config
        c.index_type, c.nlist, c.nprobe, c.index_dtype = "ivf", 16, 16, "f16"
    return p


def _exact(a, b, renumber=None):
    """two result records: the same doc_ids and bit-identical scores at all three stages"""
    from test_update_host import STAGES
    for stage, key in STAGES:
        ia = [r["doc_id"] if renumber is None else int(renumber[r["doc_id"]]) for r in a[stage]]
        assert ia == [r["doc_id"] for r in b[stage]], stage
        assert [r[key] for r in a[stage]] == [r[key] for r in b[stage]], stage


def _token_rows(p, doc_id):
    from tristage_rag_amd.stage2_rescorer import _as_bytes
    st, s = p.stage2.token_store, p.stage2._store_slot[doc_id]
    return _as_bytes(st.data[st.starts[s]: st.starts[s] + st.lens[s]]).cpu()


@pytest.mark.parametrize("store", ["bf16", "fp8"])
def test_pipeline_update_leaves_other_documents_untouched(tmp_path, store):
    from test_pipeline_gpu import _corpus
    from test_update_host import PQ, updated_texts
    docs = _corpus()
    p = _pipeline(tmp_path, stage1_enable_bm25=False, stage2_token_store_dtype=store)
    p.add_documents(docs)
    ids = sorted({r["doc_id"] for res in p.search_many(PQ) for r in res["stage1_results"][:4]} | {0, len(docs) - 1})
    keep = np.ones(len(docs), bool)
    keep[ids] = False
    before_many = p.search_many(PQ, filter=keep)
    before_one = [p.search(q, filter=keep) for q in PQ]
    info = p.get_pipeline_info()["documents"]
    assert p.update_documents(ids, updated_texts(docs, ids)) == len(ids)
    assert p.get_pipeline_info()["documents"] == info
    for a, b in zip(before_many, p.search_many(PQ, filter=keep)):
        _exact(a, b)
    for a, q in zip(before_one, PQ):
        _exact(a, p.search(q, filter=keep))
    with pytest.raises(ValueError):
        p.update_documents([ids[0], ids[0]], ["a", "b"])
    with pytest.raises(ValueError):
        p.update_documents([len(docs)], ["a"])


def test_pipeline_ivf_update_leaves_other_rows_untouched(tmp_path):
    """(the IVF retriever refuses filter=: the stored rows and token rows of the untouched documents instead)"""
    import torch
    from test_pipeline_gpu import _corpus
    from test_update_host import updated_texts
    docs = _corpus()
    p = _pipeline(tmp_path, ivf=True, stage1_enable_bm25=False)
    p.add_documents(docs)
    assert type(p.stage1.faiss_index).__name__ == "IVFFlatIndex"
    ids = [2, 50, 51, 120, len(docs) - 1]
    keep = np.ones(len(docs), bool)
    keep[ids] = False
    rows = p.stage1.faiss_index.reconstruct_n()
    toks = {d: _token_rows(p, d) for d in np.flatnonzero(keep).tolist()}
    assert p.update_documents(ids, updated_texts(docs, ids)) == len(ids)
    after = p.stage1.faiss_index.reconstruct_n()
    assert np.array_equal(after[keep], rows[keep]) and not np.array_equal(after[ids], rows[ids])
    assert p.stage1.faiss_index.ntotal == p.stage1.faiss_index.nlive == len(docs)
    for d, t in toks.items():
        assert torch.equal(_token_rows(p, d), t), d


@pytest.mark.parametrize("store", ["bf16", "fp8"])
def test_pipeline_update_save_load(tmp_path, store):
    from test_pipeline_gpu import _corpus
    from test_update_host import PQ, updated_texts
    docs = _corpus(120)
    p = _pipeline(tmp_path, stage1_enable_bm25=True, stage2_token_store_dtype=store)
    p.add_documents(docs)
    ids = [1, 7, 50, len(docs) - 1]
    new = updated_texts(docs, ids)
    slots0 = [p.stage2._store_slot[i] for i in ids]
    lens0 = [p.stage2.token_store.lens[s] for s in slots0]
    p.update_documents(ids, new)
    lens1 = [p.stage2.token_store.lens[p.stage2._store_slot[i]] for i in ids]
    assert lens1[0] > lens0[0] and lens1[1] < lens0[1]              # one grown beyond its slot, one shrunk
    assert p.stage2._store_slot[ids[0]] >= len(docs) and p.stage2._store_slot[ids[1]] == slots0[1]
    path = str(tmp_path / "i" / "pipe.json")
    p.save_index(path)
    q = _pipeline(tmp_path, stage1_enable_bm25=True, stage2_token_store_dtype=store)

    def no_encode(*a, **k):
        raise AssertionError("the token store was re-encoded instead of loaded")
    q.stage2.index_documents = no_encode
    q.load_index(path)
    assert len(q.stage2._store_slot) == len(docs) and len(q.stage2.token_store) == len(docs)
    assert q.stage1.documents == p.stage1.documents
    queries = PQ + [new[0], new[1]]
    for a, b in zip(p.search_many(queries), q.search_many(queries)):
        _exact(a, b)
    for qq in queries:
        _exact(p.search(qq), q.search(qq))


@pytest.mark.parametrize("store", ["bf16", "fp8"])
def test_pipeline_remove_update_then_compact(tmp_path, store):
    from test_pipeline_gpu import _corpus
    from test_update_host import PQ, updated_texts
    docs = _corpus()
    p = _pipeline(tmp_path, stage1_enable_bm25=False, stage2_token_store_dtype=store)
    p.add_documents(docs)
    first = p.search_many(PQ)
    gone = sorted({r["doc_id"] for res in first for r in res["stage1_results"][:5]} | {0, 5})
    ids = [i for i in sorted({r["doc_id"] for res in first for r in res["stage1_results"][5:9]} | {1, len(docs) - 1})
           if i not in gone]
    assert p.remove_documents(gone) == len(gone)
    with pytest.raises(ValueError):
        p.update_documents([ids[0], gone[0]], ["a", "b"])
    new = updated_texts(docs, ids)
    assert p.update_documents(ids, new) == len(ids)
    info = p.get_pipeline_info()["documents"]
    assert info == {"total": len(docs), "removed": len(gone), "live": len(docs) - len(gone)}
    queries = PQ + [new[0], new[1]]
    before = p.search_many(queries)
    old2new = p.compact()
    after = p.search_many(queries)
    for a, b in zip(before, after):
        _exact(a, b, renumber=old2new)
        assert all(p.stage1.documents[r["doc_id"]] == r["document"] for r in b["results"])
    st = p.stage2.token_store
    assert len(st) == len(docs) - len(gone)
    assert st.rows == sum(st.lens[p.stage2._store_slot[d]] for d in range(len(docs) - len(gone)))
    final = [t for i, t in enumerate(docs) if i not in gone]
    assert sum(1 for t in new if t in p.stage1.documents) == len(new) and len(p.stage1.documents) == len(final)


@pytest.mark.parametrize("bm25", [False, True])
@pytest.mark.parametrize("ivf", [False, True])
def test_pipeline_update_equals_a_rebuilt_pipeline(tmp_path, bm25, ivf):
    from test_pipeline_gpu import _corpus
    from test_update_host import PQ, assert_close_results, updated_texts
    docs = _corpus()
    meta = [{"tenant": "a" if i % 3 else "b", "i": i} for i in range(len(docs))]
    p = _pipeline(tmp_path, ivf=ivf, stage1_enable_bm25=bm25)
    p.add_documents(docs, meta)
    ids = sorted({r["doc_id"] for res in p.search_many(PQ) for r in res["stage1_results"][:3]} | {3, len(docs) - 1})
    new = updated_texts(docs, ids)
    # a metadata change that moves one document into the filter {"tenant": "b"} and another out of it
    into, out_of = next(i for i in ids if i % 3), next((i for i in ids if i % 3 == 0), None)
    new_meta = [dict(meta[i]) for i in ids]
    new_meta[ids.index(into)]["tenant"] = "b"
    if out_of is not None:
        new_meta[ids.index(out_of)]["tenant"] = "a"
    if not ivf:
        p.search_many(PQ, filter={"tenant": "b"})   # (the filter caches are warm when the update comes)
    assert p.update_documents(ids, new, new_meta) == len(ids)
    final, final_meta = list(docs), list(meta)
    for i, t, m in zip(ids, new, new_meta):
        final[i], final_meta[i] = t, m
    ref = _pipeline(tmp_path, ivf=ivf, stage1_enable_bm25=bm25)
    ref.add_documents(final, final_meta)
    queries = PQ + [new[0], new[-1]]
    for q in queries:
        assert_close_results(p.search(q), ref.search(q))
    for a, b in zip(p.search_many(queries), ref.search_many(queries)):
        assert_close_results(a, b)
    if not ivf:
        f = {"tenant": "b"}
        got = p.search_many(queries, filter=f)
        for a, b in zip(got, ref.search_many(queries, filter=f)):
            assert_close_results(a, b)
        seen = {r["doc_id"] for res in got for r in res["stage1_results"]}
        assert all(final_meta[d]["tenant"] == "b" for d in seen)
        assert into in {r["doc_id"] for r in p.search(new[ids.index(into)], filter=f)["stage1_results"]}
        if out_of is not None:
            assert out_of not in seen
    if not bm25:   # dense only: the new text finds its document at rank 1 with score 1, the old text no longer does
        for i, t in zip(ids, new):
            top = p.search(t)["stage1_results"][0]
            assert top["doc_id"] == i and abs(top["stage1_score"] - 1.0) < 1e-3
            assert not [r for r in p.search(docs[i])["stage1_results"]
                        if r["doc_id"] == i and abs(r["stage1_score"] - 1.0) < 1e-3]
