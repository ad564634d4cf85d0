"""IVFFlatIndex on the MI355X: deterministic spherical k-means, assignment and probing against float64, and searches
bit-identical to FlatIPIndex.search(allowed=<rows of the probed lists>)."""
import numpy as np
import pytest
import torch

from oracle import oracle

from ivf_train_model import mixture
from tristage_rag_amd.index import FlatIPIndex, IVFFlatIndex

pytestmark = pytest.mark.gpu

TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def dev(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().to(TORCH_DT[dt])


def build(x, d, nlist, dt, seed=7, chunks=1, offset=0):
    ivf = IVFFlatIndex(d, nlist, dtype=dt)
    ivf.train(dev(x, dt), seed=seed)
    flat = FlatIPIndex(d, dtype=dt)
    if offset:
        ivf.set_id_offset(offset)
        flat.set_id_offset(offset)
    for part in np.array_split(x, chunks):
        ivf.add(dev(part, dt))
    flat.add(dev(x, dt))
    return ivf, flat


def row_lists(ivf):
    """List of every stored row: the quantizer's top-1 of the stored row (what add assigned)."""
    rec = torch.from_numpy(ivf.reconstruct_n()).cuda()
    return ivf.probe(rec, 1)[1][:, 0].cpu().numpy()


def probed_masks(ivf, q, nprobe, lists):
    P = ivf.probe(q, nprobe)[1].cpu().numpy()
    return [np.isin(lists, P[i]) for i in range(P.shape[0])]


def same(a, b):
    (D0, I0), (D1, I1) = a, b
    assert torch.equal(I0.cpu(), I1.cpu())
    assert np.array_equal(D0.cpu().numpy().view(np.uint32), D1.cpu().numpy().view(np.uint32))


# ------------------------------------------------------------------ train
@pytest.mark.parametrize("dt,d", [("f16", 384), ("bf16", 768)])
def test_train_is_deterministic_and_the_objective_does_not_get_worse(dt, d):
    x = mixture(12000, d, seed=1)
    a = IVFFlatIndex(d, 48, dtype=dt)
    b = IVFFlatIndex(d, 48, dtype=dt)
    a.train(dev(x, dt), seed=3)
    b.train(dev(x, dt), seed=3)
    ca, cb = a.centroids, b.centroids
    assert np.array_equal(ca.view(np.uint32), cb.view(np.uint32))
    assert np.allclose(np.linalg.norm(ca, axis=1), 1.0, atol=1e-5)
    obj = np.array(a.objective)
    assert len(obj) == 25 and np.all(np.diff(obj) >= -1e-4 * np.abs(obj[:-1]))   # sum of best scores: non-decreasing
    c = IVFFlatIndex(d, 48, dtype=dt)
    c.train(dev(x, dt), seed=4)
    assert not np.array_equal(c.centroids, ca)


def test_train_errors_and_empty_cluster_reseeding():
    d = 128
    ivf = IVFFlatIndex(d, 16)
    with pytest.raises(RuntimeError):
        ivf.add(dev(mixture(100, d), "f16"))
    with pytest.raises(ValueError):
        ivf.train(dev(mixture(15, d), "f16"))
    # every training point equal: both initial centroids coincide, list 1 is empty after every assignment and is
    # re-seeded by splitting list 0 (FAISS's +-1/1024 perturbation on alternating dimensions); without the split the
    # two centroids would stay identical
    p = mixture(1, d, seed=5)
    x = np.repeat(p, 64, axis=0)
    ivf = IVFFlatIndex(d, 2)
    ivf.train(dev(x, "f16"))
    c = ivf.centroids
    assert np.all(np.isfinite(c)) and not np.array_equal(c[0], c[1])
    assert np.all(c.astype(np.float64) @ oracle.quantize(p, "f16")[0].astype(np.float64) > 0.999)


# ------------------------------------------------------------------ assignment and probing
@pytest.mark.parametrize("dt,d", [("f16", 768), ("bf16", 1024)])
def test_assignment_is_the_float64_argmax_and_incremental_adds_match(dt, d):
    x = mixture(20000, d, seed=2)
    one, _ = build(x, d, 40, dt)
    three = IVFFlatIndex(d, 40, dtype=dt)
    three.set_centroids(one.centroids)
    for part in np.array_split(x, 3):
        three.add(dev(part, dt))
    assert np.array_equal(one.list_sizes(), three.list_sizes())
    assert np.array_equal(one.reconstruct_n(), three.reconstruct_n())
    rec = one.reconstruct_n()
    S, L = one.probe(torch.from_numpy(rec).cuda(), 1)
    oracle.check_topk(S.cpu().numpy(), L.cpu().numpy(), one.centroids, rec, 1)
    assert np.array_equal(np.bincount(L.cpu().numpy()[:, 0], minlength=40), one.list_sizes())
    q = dev(mixture(64, d, seed=9), dt)
    for k, p in ((10, 5), (1000, 40)):
        same(one.search(q, k, nprobe=p), three.search(q, k, nprobe=p))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_probe_is_the_float64_top_nprobe(dt):
    d = 384
    ivf, _ = build(mixture(5000, d, seed=3), d, 64, dt)
    q = dev(mixture(50, d, seed=11), dt)
    qf = q.float().cpu().numpy()
    for p in (1, 10, 64):
        S, L = ivf.probe(q, p)
        oracle.check_topk(S.cpu().numpy(), L.cpu().numpy(), ivf.centroids, qf, p)


# ------------------------------------------------------------------ search
@pytest.mark.parametrize("dt,d", [("f16", 384), ("bf16", 768), ("f16", 1024)])
def test_search_equals_filtered_flat_search(dt, d):
    nlist = 50
    x = mixture(40000, d, seed=4)
    ivf, flat = build(x, d, nlist, dt)
    lists = row_lists(ivf)
    assert np.array_equal(np.bincount(lists, minlength=nlist), ivf.list_sizes())
    qs = dev(mixture(100, d, seed=12), dt)
    for B in (1, 31, 64, 100):
        q = qs[:B]
        for p in (1, 10, nlist):
            masks = probed_masks(ivf, q, p, lists)
            for k in (1, 10, 100, 1000, 2048):
                got = ivf.search(q, k, nprobe=p)
                same(got, flat.search(q, k, allowed=masks))
                if p == nlist:
                    same(got, flat.search(q, k))
    assert ivf.last_search_info()["filter_passes"] >= 1


def test_recall_never_decreases_with_nprobe():
    d, nlist = 384, 64
    x = mixture(40000, d, seed=6, spread=0.6)
    ivf, flat = build(x, d, nlist, "f16")
    q = dev(mixture(64, d, seed=13, spread=0.6), "f16")
    _, I0 = flat.search(q, 100)
    I0 = I0.cpu().numpy()
    prev = -1.0
    for p in (1, 2, 4, 8, 16, 32, 64):
        _, I = ivf.search(q, 100, nprobe=p)
        I = I.cpu().numpy()
        r = np.mean([len(set(a) & set(b)) / 100 for a, b in zip(I, I0)])
        assert r >= prev
        prev = r
    assert prev == 1.0


def _axis(d, *ix):
    v = np.zeros(d, np.float32)
    v[list(ix)] = 1.0
    return v / np.linalg.norm(v)


@pytest.mark.parametrize("big", [False, True])
def test_ties_padding_small_and_empty_lists_and_id_offset(big):
    """Equal scores in two lists ordered by original id (not by slot), lists of one row, empty lists, padding,
    an id offset; on the dense path (small index) and on the filter path (> 32768 slots)."""
    d = 128
    rng = np.random.default_rng(8)
    A, B = _axis(d, 0, 1), _axis(d, 0, 2)   # e0 . A == e0 . B exactly
    rows = [A if i % 2 == 0 else B for i in range(40)] + [_axis(d, 3)]   # list 2 holds one row
    if big:
        noise = rng.standard_normal((40000, d)).astype(np.float32) * 0.05
        noise[:, 4] += 1.0
        rows += list(noise / np.linalg.norm(noise, axis=1, keepdims=True))   # list 3
    x = np.stack(rows)
    cent = np.stack([_axis(d, 1), _axis(d, 2), _axis(d, 3), _axis(d, 4), _axis(d, 5), _axis(d, 6)])   # 4, 5 empty
    ivf = IVFFlatIndex(d, 6, dtype="f16")
    ivf.set_centroids(cent)
    flat = FlatIPIndex(d, dtype="f16")
    ivf.set_id_offset(1000)
    flat.set_id_offset(1000)
    ivf.add(dev(x, "f16"))
    flat.add(dev(x, "f16"))
    assert list(ivf.list_sizes()[:3]) == [20, 20, 1] and list(ivf.list_sizes()[4:]) == [0, 0]
    lists = row_lists(ivf)
    q = dev(np.stack([_axis(d, 0), _axis(d, 0, 3), _axis(d, 5), _axis(d, 0, 4)]), "f16")
    for p in (1, 2, 3, 6):
        masks = probed_masks(ivf, q, p, lists)
        for k in (1, 10, 50, 100):
            got = ivf.search(q, k, nprobe=p)
            same(got, flat.search(q, k, allowed=masks))
    D, I = ivf.search(q[:1], 50, nprobe=2)   # the A and B rows tie: ids in ascending order, then padding
    I = I.cpu().numpy()[0]
    assert list(I[:40]) == list(range(1000, 1040)) and np.all(I[40:] == -1)


def test_threshold_overflow_is_redone_exactly():
    d = 128
    rng = np.random.default_rng(10)
    A = _axis(d, 0, 1)
    other = rng.standard_normal((20000, d)).astype(np.float32) * 0.05
    other[:, 2] += 1.0
    x = np.concatenate([np.repeat(A[None], 20000, axis=0), other / np.linalg.norm(other, axis=1, keepdims=True)])
    x = x[rng.permutation(len(x))]
    ivf = IVFFlatIndex(d, 2, dtype="f16")
    ivf.set_centroids(np.stack([_axis(d, 1), _axis(d, 2)]))
    flat = FlatIPIndex(d, dtype="f16")
    ivf.add(dev(x, "f16"))
    flat.add(dev(x, "f16"))
    q = dev(np.stack([_axis(d, 0, 1), _axis(d, 1)]), "f16")
    lists = row_lists(ivf)
    for k in (10, 1000):
        got = ivf.search(q, k, nprobe=1)
        info = ivf.last_search_info()
        assert info["filter_passes"] == 1 and info["redone"] == 1   # 20000 equal scores > 16384 candidate slots
        same(got, flat.search(q, k, allowed=probed_masks(ivf, q, 1, lists)))


def test_ivf_errors():
    d = 64
    ivf, _ = build(mixture(2000, d), d, 8, "f16")
    q = dev(mixture(2, d), "f16")
    with pytest.raises(NotImplementedError):
        ivf.search(q, 10, allowed=np.ones(2000, bool))
    with pytest.raises(NotImplementedError):
        ivf.search(q, 20000)
    assert ivf.finish() == []
    D, I = ivf.search(q, 5, async_=True)
    same((D, I), ivf.search(q, 5))
    ivf.reset()
    assert ivf.ntotal == 0 and ivf.is_trained


# ------------------------------------------------------------------ retriever
def test_retriever_auto_switch_and_save_load(tmp_path):
    from tristage_rag_amd.encoders import SentenceEncoder
    from tristage_rag_amd.stage1_retriever import Stage1Config, Stage1Retriever
    enc = SentenceEncoder("random:tiny", device="cpu")
    docs = [f"document {i} about topic {i % 37} and item {i % 11}" for i in range(1001)]

    def s1(**kw):
        cfg = Stage1Config(model_name="random:tiny", device="cpu", cache_dir=str(tmp_path / "m"),
                           index_dir=str(tmp_path / "i"), enable_bm25=False, index_type="auto", nlist=16,
                           nprobe=4, index_dtype="f16", **kw)
        return Stage1Retriever(cfg, model=enc)

    small = s1()
    small.add_documents(docs[:1000])
    assert small.get_stats()["index_type"] == "flat" and type(small.faiss_index).__name__ == "FlatIPIndex"
    big = s1()
    big.add_documents(docs)
    assert big.get_stats()["index_type"] == "ivf" and big.faiss_index.nprobe == 4
    with pytest.raises(NotImplementedError):
        big.search("topic 3", top_k=5, filter={"a": 1})
    want = big.search_many(["topic 3", "item 7", "document 500"], top_k=20)
    path = str(tmp_path / "i" / "stage1_index.pkl")
    big.save_index(path)
    again = s1()
    again.load_index(path)
    assert again.get_stats()["index_type"] == "ivf"
    assert np.array_equal(again.faiss_index.centroids, big.faiss_index.centroids)
    assert again.search_many(["topic 3", "item 7", "document 500"], top_k=20) == want
