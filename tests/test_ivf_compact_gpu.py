"""IVF compaction on the MI355X (IVFFlatIndex.compact, RetrievalPipeline.remove_documents / compact on an IVF index):
a compacted index is indistinguishable from a fresh index with the same centroids after add of the surviving rows —
list sizes, reconstructed rows, occupied blocks and search results bit for bit, now and after later adds, removals and
updates — and keeps the IVF search identity against the flat index."""
import numpy as np
import pytest

from test_ivf_gpu import build, dev, mixture, probed_masks, row_lists, same

pytestmark = pytest.mark.gpu

NLIST = 16


def _fresh_like(ivf, rows, dt, offset=0):
    """A new index with ivf's centroids after ONE add of `rows` (float32, already rounded to the storage type)."""
    from tristage_rag_amd.index import IVFFlatIndex
    fresh = IVFFlatIndex(ivf.d, ivf.nlist, dtype=dt)
    fresh.set_centroids(ivf.centroids)
    if offset:
        fresh.set_id_offset(offset)
    if len(rows):
        fresh.add(dev(rows, dt))
    return fresh


def _blocks(ivf):
    return int(((ivf.list_sizes() + 31) // 32).sum())


def _holey_pair(dt, d, offset=0):
    """An IVF index and its flat mirror (40 000 mixture rows in 3 adds) after: 5 000 random removals plus every row of
    one list, 2 000 updates with new content (rows change lists and leave holes), an add of 500 rows, the removal of
    100 of those, and of whatever the updates and the add put into the emptied list.  -> ivf, flat, live mask."""
    x = mixture(40000, d, seed=21)
    ivf, flat = build(x, d, NLIST, dt, chunks=3, offset=offset)
    rng = np.random.default_rng(1000 * d + offset)
    lists = row_lists(ivf)
    sizes = np.bincount(lists, minlength=NLIST)
    emptied = int(np.argmin(np.where(sizes > 0, sizes, sizes.max() + 1)))   # the smallest list that holds rows
    live = np.ones(40000, bool)

    def remove(ids):
        ids = np.asarray(ids, dtype=np.int64)
        assert ivf.remove_ids(ids + offset) == ids.size == flat.remove_ids(ids + offset)
        live[ids] = False

    remove(np.union1d(rng.choice(40000, 5000, replace=False), np.flatnonzero(lists == emptied)))
    assert ivf.list_sizes()[emptied] == 0
    U = np.sort(rng.choice(np.flatnonzero(live), 2000, replace=False))
    Y = mixture(2000, d, seed=22)
    ivf.update_rows(U + offset, dev(Y, dt))
    flat.update_rows(U + offset, dev(Y, dt))
    extra = mixture(500, d, seed=23)
    ivf.add(dev(extra, dt))
    flat.add(dev(extra, dt))
    live = np.concatenate([live, np.ones(500, bool)])
    remove(40000 + rng.choice(500, 100, replace=False))
    back = np.flatnonzero((row_lists(ivf) == emptied) & live)   # the emptied list is empty when the compaction comes
    if back.size:
        remove(back)
    assert ivf.list_sizes()[emptied] == 0 and ivf.ntotal == 40500 and ivf.nlive == int(live.sum())
    assert ivf.nlive >= 32768   # the compacted index stays above the filter-path threshold
    return ivf, flat, live


def _compact_and_check_map(ivf, live):
    cent = ivf.centroids
    old2new = ivf.compact()
    n = int(live.sum())
    assert old2new.dtype == np.int64 and old2new.shape == live.shape
    assert (old2new[~live] == -1).all() and np.array_equal(old2new[live], np.arange(n))
    assert ivf.ntotal == ivf.nlive == n
    assert np.array_equal(ivf.centroids.view(np.uint32), cent.view(np.uint32))
    return old2new


def _assert_same_index(a, b, q, ks=(1, 100, 1000, 3000), ps=(1, 4, NLIST)):
    assert a.ntotal == b.ntotal
    assert np.array_equal(a.list_sizes(), b.list_sizes())
    assert np.array_equal(a.reconstruct_n(), b.reconstruct_n())
    for k in ks:
        for p in ps:
            same(a.search(q, k, nprobe=p), b.search(q, k, nprobe=p))


# ------------------------------------------------------------------ 1. compacted equals fresh
@pytest.mark.parametrize("dt,d,offset", [("f16", 64, 0), ("f16", 64, 1000), ("bf16", 768, 0), ("f16", 1024, 0)])
def test_compacted_equals_fresh(dt, d, offset):
    import torch
    ivf, flat, live = _holey_pair(dt, d, offset)
    rec = ivf.reconstruct_n()
    _compact_and_check_map(ivf, live)
    fresh = _fresh_like(ivf, rec[live], dt, offset)
    q = dev(mixture(70, d, seed=24), dt)   # two passes, one partial
    _assert_same_index(ivf, fresh, q)
    # the same occupied blocks, and no more than the rows need
    for idx in (ivf, fresh):
        idx.search(q, 100, nprobe=NLIST)
        info = idx.last_search_info()
        assert info["filter_passes"] > 0 and info["live_blocks"] == _blocks(idx)
    ivf.search(q, 3000, nprobe=NLIST)
    assert ivf.last_search_info()["filter_passes"] == 0   # k > 2048: the dense path
    # the IVF identity against the flat index compacted alike
    flat.compact()
    assert flat.ntotal == ivf.ntotal
    lists = row_lists(ivf)
    assert np.array_equal(np.bincount(lists, minlength=NLIST), ivf.list_sizes())
    for p in (1, 4):
        masks = probed_masks(ivf, q, p, lists)
        for k in (100, 1000):
            same(ivf.search(q, k, nprobe=p), flat.search(q, k, allowed=masks))
    same(ivf.search(q, 100, nprobe=NLIST), flat.search(q, 100))
    for i in (ivf, flat, fresh):
        i.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. life goes on after compaction
def test_life_goes_on_after_compaction():
    import torch
    dt, d = "f16", 64
    ivf, flat, live = _holey_pair(dt, d)
    flat.close()
    rec = ivf.reconstruct_n()
    _compact_and_check_map(ivf, live)
    # a second compaction right after the first: the identity, and nothing changes
    after = ivf.reconstruct_n()
    sizes, blocks = ivf.list_sizes(), _blocks(ivf)
    assert np.array_equal(ivf.compact(), np.arange(ivf.ntotal))
    assert np.array_equal(ivf.reconstruct_n(), after) and np.array_equal(ivf.list_sizes(), sizes)
    fresh = _fresh_like(ivf, rec[live], dt)
    q = dev(mixture(70, d, seed=24), dt)
    ivf.search(q, 100, nprobe=NLIST)
    assert ivf.last_search_info()["live_blocks"] == blocks
    # the same add, removal and update on both
    n = ivf.ntotal
    rng = np.random.default_rng(5)
    extra, Y = mixture(1000, d, seed=25), mixture(700, d, seed=26)
    D = rng.choice(n + 1000, 3000, replace=False)
    for idx in (ivf, fresh):
        idx.add(dev(extra, dt))
        assert idx.remove_ids(D) == D.size
    alive = np.ones(n + 1000, bool)
    alive[D] = False
    U = np.sort(rng.choice(np.flatnonzero(alive), 700, replace=False))
    for idx in (ivf, fresh):
        idx.update_rows(U, dev(Y, dt))
        with pytest.raises(ValueError):
            idx.update_rows(D[:1], dev(Y[:1], dt))   # a removed id stays removed across the compaction
    assert ivf.nlive == fresh.nlive == int(alive.sum())
    _assert_same_index(ivf, fresh, q, ks=(100, 3000), ps=(4, NLIST))
    # and the next compaction of both gives the same index again
    assert np.array_equal(ivf.compact(), fresh.compact())
    _assert_same_index(ivf, fresh, q, ks=(100,), ps=(NLIST,))
    for i in (ivf, fresh):
        i.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. edges
def _small():
    d = 64
    ivf, _ = build(mixture(2000, d), d, 8, "f16")
    return ivf, d, dev(mixture(40, d, seed=31), "f16")


def test_compact_without_a_hole_moves_nothing():
    ivf, d, q = _small()
    rec = ivf.reconstruct_n()
    before = ivf.search(q, 50, nprobe=3)
    assert np.array_equal(ivf.compact(), np.arange(2000))
    assert ivf.ntotal == ivf.nlive == 2000 and np.array_equal(ivf.reconstruct_n(), rec)
    same(ivf.search(q, 50, nprobe=3), before)
    ivf.close()


def test_compact_after_updates_only_closes_their_holes():
    """The map is the identity and every search returns what it returned.  A 2 000-row index searches on the dense
    path, which reports no live blocks; the block count is therefore checked on a 36 000-row index (filter path)."""
    ivf, d, q = _small()
    U = np.arange(100, 1900, 6)
    ivf.update_rows(U, dev(mixture(U.size, d, seed=32), "f16"))
    rec = ivf.reconstruct_n()
    before = [ivf.search(q, k, nprobe=p) for k in (1, 50, 2000) for p in (1, 8)]
    assert np.array_equal(ivf.compact(), np.arange(2000))
    assert ivf.ntotal == ivf.nlive == 2000 and np.array_equal(ivf.reconstruct_n(), rec)
    for b, (k, p) in zip(before, [(k, p) for k in (1, 50, 2000) for p in (1, 8)]):
        same(ivf.search(q, k, nprobe=p), b)
    fresh = _fresh_like(ivf, rec, "f16")
    _assert_same_index(ivf, fresh, q, ks=(50,), ps=(8,))
    ivf.close()
    fresh.close()
    big, _ = build(mixture(36000, d, seed=33), d, 8, "f16")
    U = np.arange(0, 36000, 12)
    big.update_rows(U, dev(mixture(U.size, d, seed=34), "f16"))
    want = big.search(q, 100, nprobe=8)
    holey = big.last_search_info()
    assert holey["filter_passes"] > 0 and holey["live_blocks"] > _blocks(big)
    assert np.array_equal(big.compact(), np.arange(36000))
    same(big.search(q, 100, nprobe=8), want)
    assert big.last_search_info()["live_blocks"] == _blocks(big)
    big.close()


def test_compact_after_removing_everything_leaves_an_empty_trained_index():
    ivf, d, q = _small()
    cent = ivf.centroids
    assert ivf.remove_ids(np.arange(2000)) == 2000
    assert (ivf.compact() == -1).all()
    assert ivf.ntotal == 0 and ivf.nlive == 0 and ivf.is_trained
    assert np.array_equal(ivf.centroids.view(np.uint32), cent.view(np.uint32))
    assert ivf.compact().size == 0
    x = mixture(300, d, seed=35)
    ivf.add(dev(x, "f16"))
    fresh = _fresh_like(ivf, [], "f16")
    fresh.add(dev(x, "f16"))
    assert ivf.ntotal == 300
    _assert_same_index(ivf, fresh, q, ks=(1, 50), ps=(1, 8))
    D, I = ivf.search(q, 400, nprobe=8)
    I = I.cpu().numpy()
    assert np.array_equal(np.sort(I[:, :300], axis=1), np.tile(np.arange(300), (40, 1))) and (I[:, 300:] == -1).all()
    ivf.close()
    fresh.close()


def test_exact_ties_come_out_in_ascending_new_id():
    """Duplicate rows on both sides of removed ids, in two lists whose rows score alike."""
    from tristage_rag_amd.index import IVFFlatIndex
    from test_ivf_gpu import _axis
    d = 128
    A, B = _axis(d, 0, 1), _axis(d, 0, 2)   # e0 . A == e0 . B exactly
    x = np.stack([A if i % 2 == 0 else B for i in range(40)] + [_axis(d, 3)])
    ivf = IVFFlatIndex(d, 4, dtype="f16")
    ivf.set_centroids(np.stack([_axis(d, 1), _axis(d, 2), _axis(d, 3), _axis(d, 4)]))
    ivf.add(dev(x, "f16"))
    ivf.update_rows([11], dev(x[11:12], "f16"))   # the same row again: it moves behind its list's later rows
    assert ivf.remove_ids([7, 20, 21]) == 3
    old2new = ivf.compact()
    assert ivf.ntotal == 38 and old2new[11] == 10 and old2new[39] == 36
    q = dev(np.stack([_axis(d, 0)]), "f16")
    D, I = ivf.search(q, 50, nprobe=2)
    D, I = D.cpu().numpy()[0], I.cpu().numpy()[0]
    assert list(I[:37]) == list(range(37)) and np.all(I[37:] == -1)
    assert np.all(D[:37] == D[0])
    ivf.close()


# ------------------------------------------------------------------ 4. pipeline
PQ = ["neural networks attention", "language retrieval system", "gpu memory index", "token embedding search"]
STAGES = (("stage1_results", "stage1_score"), ("stage2_results", "stage2_score"), ("results", "stage3_score"))


def _ivf_pipeline(tmp_path, **extra):
    from test_update_gpu import _pipeline
    return _pipeline(tmp_path, ivf=True, **extra)


def _no_removed(results, gone):
    for res in results:
        for stage, _ in STAGES:
            assert not {r["doc_id"] for r in res[stage]} & set(gone), stage


@pytest.mark.parametrize("bm25", [False, True])
def test_pipeline_ivf_remove_then_compact(tmp_path, bm25):
    from test_pipeline_gpu import _corpus
    docs = _corpus()
    p = _ivf_pipeline(tmp_path, stage1_enable_bm25=bm25)
    p.add_documents(docs)
    assert type(p.stage1.faiss_index).__name__ == "IVFFlatIndex"
    first = p.search_many(PQ)
    gone = sorted({r["doc_id"] for res in first for r in res["stage1_results"][:10]} | {0, 5, len(docs) - 1})
    assert p.remove_documents(gone + gone[:3]) == len(gone)
    info = p.get_pipeline_info()["documents"]
    assert info == {"total": len(docs), "removed": len(gone), "live": len(docs) - len(gone)}
    assert p.stage1.faiss_index.nlive == len(docs) - len(gone)
    # no stage returns a removed document: arrays path (search_many), record path (search)
    _no_removed(p.search_many(PQ), gone)
    _no_removed([p.search(q) for q in PQ], gone)
    cent = p.stage1.faiss_index.centroids
    before = p.search_many(PQ)
    old2new = p.compact()
    assert type(p.stage1.faiss_index).__name__ == "IVFFlatIndex"   # compacted, not rebuilt and retrained
    assert np.array_equal(p.stage1.faiss_index.centroids.view(np.uint32), cent.view(np.uint32))
    assert (old2new[gone] == -1).all() and len(p.stage1.documents) == len(docs) - len(gone)
    assert p.stage1.faiss_index.ntotal == p.stage1.faiss_index.nlive == len(docs) - len(gone)
    after = p.search_many(PQ)
    for b in after:
        for stage, _ in STAGES:
            assert all(p.stage1.documents[r["doc_id"]] == r["document"] for r in b[stage])
    if bm25:   # (BM25 is refitted on the survivors: the fused scores change)
        return
    # the dense-only results before the compaction, renumbered, with bit-identical scores at every stage
    for a, b in zip(before, after):
        for stage, key in STAGES:
            assert [old2new[r["doc_id"]] for r in a[stage]] == [r["doc_id"] for r in b[stage]], stage
            assert [r[key] for r in a[stage]] == [r[key] for r in b[stage]], stage


def test_pipeline_ivf_save_load_keeps_tombstones(tmp_path):
    from test_pipeline_gpu import _corpus
    docs = _corpus(120)
    p = _ivf_pipeline(tmp_path, stage1_enable_bm25=True)
    p.add_documents(docs)
    assert p.remove_documents([1, 2, 3, 50]) == 4
    path = str(tmp_path / "i" / "pipe.json")
    p.save_index(path)
    q = _ivf_pipeline(tmp_path, stage1_enable_bm25=True)
    q.load_index(path)
    assert type(q.stage1.faiss_index).__name__ == "IVFFlatIndex"
    assert q.get_pipeline_info()["documents"]["removed"] == 4
    assert q.stage1.faiss_index.nlive == len(docs) - 4 and q.stage1.faiss_index.ntotal == len(docs)
    for a, b in zip(p.search_many(PQ), q.search_many(PQ)):
        for stage, key in STAGES:
            assert [r["doc_id"] for r in a[stage]] == [r["doc_id"] for r in b[stage]], stage
            assert [r[key] for r in a[stage]] == [r[key] for r in b[stage]], stage
        assert not {r["doc_id"] for r in b["stage1_results"]} & {1, 2, 3, 50}


def test_pipeline_auto_index_above_1000_documents_removes_and_compacts(tmp_path):
    from test_pipeline_gpu import _build
    p = _build("cuda", tmp_path, doubles=False, stage1_enable_bm25=False)
    c = p.stage1.config
    c.index_type, c.nlist, c.nprobe, c.index_dtype = "auto", 16, 16, "f16"
    docs = [f"document {i} about topic {i % 37} and item {i % 11}" for i in range(1001)]
    p.add_documents(docs)
    assert p.stage1.get_stats()["index_type"] == "ivf"
    queries = ["topic 3", "item 7", "document 500"]
    gone = sorted({r["doc_id"] for res in p.search_many(queries) for r in res["stage1_results"][:5]} | {0, 1000})
    assert p.remove_documents(gone) == len(gone)
    assert p.get_pipeline_info()["documents"] == {"total": 1001, "removed": len(gone), "live": 1001 - len(gone)}
    _no_removed(p.search_many(queries), gone)
    _no_removed([p.search(q) for q in queries], gone)
    old2new = p.compact()
    assert (old2new[gone] == -1).all() and p.stage1.faiss_index.ntotal == 1001 - len(gone)
    assert type(p.stage1.faiss_index).__name__ == "IVFFlatIndex"
    for res in p.search_many(queries):
        assert all(p.stage1.documents[r["doc_id"]] == r["document"] for r in res["results"])
