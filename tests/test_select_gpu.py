"""select_kernel in its three modes and the merges built on it, on the adversarial tables of tests/select_cases.py
("selection order"): ids with `np.array_equal`, scores by bit pattern (NaN positions with isnan) against
`canonical_topk`.  tests/test_select_host.py shows which branch of the kernel each case reaches."""
import numpy as np
import pytest

import exact_inputs as ex
import select_cases as sc
from helpers import make_corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _t(x, dtype):
    import torch
    dt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[dtype]
    return torch.tensor(np.asarray(x), device="cuda").to(dt)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _check(got, want, what):
    D, I = _np(got[0]), _np(got[1])
    D0, I0 = want
    assert D.shape == D0.shape and I.shape == I0.shape, what
    bad = np.argwhere(I != I0)
    assert bad.size == 0, (f"{what}: {bad.shape[0]} ids differ, first at {bad[0].tolist()}: got {I[tuple(bad[0])]} "
                           f"want {I0[tuple(bad[0])]}")
    nan = np.isnan(D0)
    assert np.array_equal(np.isnan(D), nan), f"{what}: NaN positions differ"
    bad = np.argwhere((D.view(np.uint32) != D0.view(np.uint32)) & ~nan)
    assert bad.size == 0, (f"{what}: scores differ first at {bad[0].tolist()}: got {D[tuple(bad[0])]!r} "
                           f"want {D0[tuple(bad[0])]!r}")
    assert sc.same_result((D, I), (D0, I0)), what


# ------------------------------------------------------------------------------------------------------------ merge
def _merge(torch, scores, ids):
    from tristage_rag_amd.index import merge_topk
    return merge_topk(torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda())


def _merge_packed(torch, scores, ids):
    from tristage_rag_amd.index import merge_topk_packed, packed_layout
    R, B, k = scores.shape
    ids_at, nbytes = packed_layout(B, k)
    buf = np.zeros((R, nbytes), np.uint8)
    for r in range(R):
        buf[r, : 4 * B * k] = scores[r].view(np.uint8).ravel()
        buf[r, ids_at:] = ids[r].view(np.uint8).ravel()
    return merge_topk_packed(torch.from_numpy(buf.ravel()).cuda(), R, B, k)


@pytest.mark.parametrize("R,k", sc.MERGE_SHAPES)
def test_merge_on_the_whole_table(torch_mod, R, k):
    """merge_topk on every (score set, id layout) of the table, B = 1 and B = 3 (a different entry per query); the
    entries in which more than 1024 entries can tie at rank k run twice and must repeat themselves bit for bit."""
    torch = torch_mod
    failed, unstable = [], []
    for cases, B in sc.merge_batches(R, k):
        scores, ids = sc.merge_batch(cases, R, k)
        want = sc.canonical_merge(scores, ids, k)
        got = _merge(torch, scores, ids)
        got = (_np(got[0]), _np(got[1]))
        for b, c in enumerate(cases):
            if not sc.same_result((got[0][b], got[1][b]), (want[0][b], want[1][b])):
                failed.append((c, B))
        if any(c[0] in sc.MANY_TIES for c in cases):
            again = _merge(torch, scores, ids)
            if not sc.same_result((_np(again[0]), _np(again[1])), got):
                unstable.append(cases)
    if failed or unstable:
        print(f"R={R} k={k}: wrong {sorted(set(failed))}; two runs differ {unstable}")
    assert not unstable
    if failed:
        cases = (failed[0][0],)
        scores, ids = sc.merge_batch(cases, R, k)
        _check(_merge(torch, scores, ids), sc.canonical_merge(scores, ids, k), f"R={R} k={k} {cases[0]} (of {len(failed)})")
    assert not failed


@pytest.mark.parametrize("R,k", [(3, 7), (8, 1001), (7, 2049), (17, 999)])
def test_merge_packed_with_the_id_pad(torch_mod, R, k):
    """merge_topk_packed, B = 1 and odd k: the score block of a rank is 4 k bytes, so its id block sits behind a 4-byte
    pad and the lists' score and id pitches differ."""
    from tristage_rag_amd.index import packed_layout
    assert packed_layout(1, k)[0] == 4 * k + 4
    for c in sc.MERGE_TABLE:
        scores, ids = sc.merge_batch((c,), R, k)
        _check(_merge_packed(torch_mod, scores, ids), sc.canonical_merge(scores, ids, k), f"{c}")


def test_merge_of_65_queries(torch_mod):
    R, k, B = 8, 1000, 65
    cases = tuple(sc.MERGE_TABLE[i % len(sc.MERGE_TABLE)] for i in range(B))
    scores, ids = sc.merge_batch(cases, R, k)
    want = sc.canonical_merge(scores, ids, k)
    _check(_merge(torch_mod, scores, ids), want, "B=65")
    _check(_merge_packed(torch_mod, scores, ids), want, "B=65 packed")


def test_merge_k_8193_is_unsupported(torch_mod):
    from tristage_rag_amd import _lib
    k = sc.MERGE_K_UNSUPPORTED
    s = np.zeros((2, 1, k), np.float32)
    with pytest.raises(_lib.TriStageNativeError, match="exceeds 8192"):
        _merge(torch_mod, s, np.zeros(s.shape, np.int64))


def test_merge_issue_example(torch_mod):
    """Eight lists of k = 1000, one repeated score, ids j * R + r: ids 0..999, twice the same."""
    scores, ids = sc.merge_batch((("all_equal", "interleaved"),), 8, 1000)
    for _ in range(2):
        D, I = _merge(torch_mod, scores, ids)
        assert np.array_equal(_np(I)[0], np.arange(1000)) and (_np(D) == 0.75).all()


# ----------------------------------------------------------------------------------------- SEL_DENSE through an index
def _flat(d, dtype, corpus):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(_t(corpus, dtype))
    return idx


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("n", sc.PLANT_N)
def test_dense_select_on_planted_scores(torch_mod, n, dtype):
    """The identity queries read the planted columns back, so SEL_DENSE ranks exactly sc.PLANTED: every k of the list
    the kernel serves at this n, 17 distributions per search."""
    corpus, queries, units = sc.planted(n)
    ex.assert_exactly_summable(corpus, queries, sc.UNIT)
    idx = _flat(sc.PLANT_D, dtype, corpus)
    tq = _t(queries, dtype)
    assert np.array_equal(_np(idx.scores(tq)), sc.planted_scores(units))
    kmax = max(sc.plant_ks(n))
    want = sc.planted_topk(units, kmax)
    for k in sc.plant_ks(n):
        got = idx.search(tq, k, exact_dense=True)
        assert idx.last_search_info()["path"] == "dense"
        wD, wI = want[0][:, :k].copy(), want[1][:, :k].copy()
        _check(got, (wD, wI), f"n={n} k={k}")
    idx.close()


def test_dense_select_with_an_id_offset_above_2_32(torch_mod):
    n, off = 1061, (1 << 32) + 12345
    corpus, queries, units = sc.planted(n)
    idx = _flat(sc.PLANT_D, "f16", corpus)
    idx.set_id_offset(off)
    for k in (3, 1000, n + 3):
        _check(idx.search(_t(queries, "f16"), k, exact_dense=True), sc.planted_topk(units, k, id_offset=off), f"k={k}")
    idx.close()


def test_chunked_dense_select(torch_mod):
    """2^20 + 40 rows: two chunks of the dense path, the second one's list of 100 holds 40 rows and 60 paddings; the
    SEL_PAIRS32 select over the two lists returns none of them."""
    corpus, queries, units = sc.chunked()
    idx = _flat(sc.PLANT_D, "f16", corpus)
    got = idx.search(_t(queries, "f16"), sc.K_CHUNKED, exact_dense=True)
    assert idx.last_search_info()["path"] == "dense"
    want = sc.planted_topk(units, sc.K_CHUNKED)
    assert (want[1] >= 0).all()
    _check(got, want, "chunked")
    idx.close()


# ------------------------------------------------------------------------------------ SEL_PAIRS32 with -1 ids (masks)
def test_masked_dense_select(torch_mod):
    """Allowed sets of 0, 5, k - 1, k and k + 1 rows of 20011 (below the filter path's floor: the dense path with
    mask_ids_kernel), each on another distribution; and half of 16384 rows, which SEL_PAIRS32 takes without a global
    pass."""
    corpus, queries, units = sc.planted(sc.N_MASKED, sc.MASKED_NAMES)
    allowed = sc.masked_sets()
    idx = _flat(sc.PLANT_D, "f16", corpus)
    got = idx.search(_t(queries, "f16"), sc.K_MASKED, allowed=allowed)
    info = idx.last_filter_info()
    assert info["dense_passes"] >= 1 and info["filter_passes"] == 0, info
    want = sc.planted_topk(units, sc.K_MASKED, allowed=allowed)
    for q, c in enumerate(sc.MASKED_COUNTS):
        assert (want[1][q] >= 0).sum() == min(c, sc.K_MASKED)
    _check(got, want, "masked")
    idx.close()
    n, k = sc.MASKED_DIRECT
    corpus, queries, units = sc.planted(n)
    half = sc.masked_direct_set()
    idx = _flat(sc.PLANT_D, "bf16", corpus)
    _check(idx.search(_t(queries, "bf16"), k, allowed=half), sc.planted_topk(units, k, allowed=half), "half of 16384")
    idx.close()


# ------------------------------------------------------------------------------------------ filter path (n_per_q lists)
@pytest.fixture(scope="module")
def filter_indexes():
    made = {}
    def get(n):
        if n not in made:
            corpus, queries, units = sc.planted(n)
            ex.assert_exactly_summable(corpus, queries, sc.UNIT)
            made[n] = (_flat(sc.PLANT_D, "f16", corpus), queries, units)
        return made[n]
    yield get
    for idx, _, _ in made.values():
        idx.close()


def _rows(names):
    return [list(sc.PLANTED).index(x) for x in names]


def test_filter_path_select_on_planted_scores(torch_mod, filter_indexes):
    """SEL_PAIRS32 over the candidate lists of the filter path (n_per_q counts): distinct scores and scores that share
    three key bytes must stay on it, with a threshold from tau_kernel<1> (sample rank <= 64) and from tau_kernel<4>.
    k = 2048 needs 32 k rows to be a filter search at all (ts_index_filter_path): at ex.N_FILTER it is a dense search,
    asserted as such, and the filter form of it runs at 32 * 2048 + 37 rows."""
    ranks = []
    for n, ks in ((ex.N_FILTER, sc.FILTER_K), (sc.N_FILTER_2048, (2048,))):
        idx, queries, units = filter_indexes(n)
        rows = _rows(sc.FILTER_ON_PATH)
        tq = _t(queries[rows], "f16")
        for k in ks:
            got = idx.search(tq, k, classic=True)
            info = idx.last_search_info()
            print(f"n={n} k={k}: {info}")
            if sc.filter_path_expected(n, k):
                assert info["path"] == "filter", info
                assert info["sample_rank"] == sc.sample_rank(n, k), info
                ranks.append(info["sample_rank"])
            else:
                assert (n, k) == (ex.N_FILTER, 2048) and info["path"] == "dense", info
            _check(got, sc.planted_topk(units[rows], k), f"n={n} k={k}")
    assert min(ranks) <= 64 < max(ranks), ranks            # both tau_kernel instantiations


def test_filter_path_select_on_tied_scores(torch_mod, filter_indexes):
    """all_equal and two_level: thousands of rows tie at the threshold, so a dense fallback is legitimate — the result
    is asserted, the path only recorded."""
    idx, queries, units = filter_indexes(ex.N_FILTER)
    rows = _rows(sc.FILTER_ANY_PATH)
    tq = _t(queries[rows], "f16")
    for k in sc.FILTER_K:
        got = idx.search(tq, k, classic=True)
        print(f"k={k}: path {idx.last_search_info()['path']}")
        _check(got, sc.planted_topk(units[rows], k), f"k={k}")


# -------------------------------------------------------------------------------------------------------------- IVF
def test_ivf_select_on_a_two_level_set(torch_mod):
    """Every list probed at 32768 + 37 rows, where scan_ivf_kernel runs (test_exact_scores_gpu.py): 1001 rows at the
    high level, k = 1000, 1001 and 1002."""
    from tristage_rag_amd.index import IVFFlatIndex
    n, d = ex.N_FILTER, 96
    rng = np.random.default_rng(9)
    units = np.full((2, n), -768, np.int64)
    units[0, rng.permutation(n)[:1001]] = 1280
    units[1] = sc.PLANTED["ties(1025)"](n, rng)
    corpus = np.zeros((n, d), np.float32)
    corpus[:, 0], corpus[:, 1] = units[0] * sc.UNIT, units[1] * sc.UNIT
    corpus[:, 2:] = rng.integers(-3, 4, size=(n, d - 2))        # what spreads the rows over the lists
    queries = np.zeros((2, d), np.float32)
    queries[0, 0] = queries[1, 1] = 1.0
    ex.assert_exactly_summable(corpus, queries, sc.UNIT)
    ivf = IVFFlatIndex(d, 8, dtype="f16", nprobe=8)
    ivf.set_centroids(make_corpus(8, d, seed=3, dtype="f16"))
    ivf.add(_t(corpus, "f16"))
    for k in (1000, 1001, 1002):
        got = ivf.search(_t(queries, "f16"), k)
        info = ivf.last_search_info()
        print(f"k={k}: {info}")
        assert info["filter_passes"] >= 1, info
        _check(got, sc.planted_topk(units, k), f"k={k}")
    ivf.close()
