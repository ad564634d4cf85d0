"""Stage-2 MaxSim against exact results ("exact inputs for MaxSim"): on the exactly scored inputs of
tests/exact_maxsim_inputs.py every entry point, in every store type, must return the integer reference of ``maxsim``
mode bit for bit — `np.array_equal`, no tolerance — and ``colbert`` mode within 2e-6 of float64.  The table reaches
every instantiation of maxsim16_kernel and maxsim_kernel the dispatch can select (tests/test_exact_maxsim_host.py);
further tests follow a launch whose maxima are all 1 by one whose maxima are all negative on the same scratch cells,
and go beyond what one launch takes."""
import functools

import numpy as np
import pytest

import exact_maxsim_inputs as em

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _num_cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tdt(torch, name):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]


def _query(torch, q, store):
    """The query as the store type takes it (an e4m3 store: the f16 / bf16 query of the store's name)."""
    name = store.split("_")[1] if store.startswith("e4m3") else store
    t = torch.from_numpy(np.array(q)).cuda().to(_tdt(torch, name))
    assert np.array_equal(t.float().cpu().numpy(), q)
    return t


def _rows(torch, x, store, quantizer=False):
    """float32 rows -> the store type, on the GPU; nothing is rounded on the way (checked)."""
    x = torch.from_numpy(np.array(x))
    if not store.startswith("e4m3"):
        t = x.cuda().to(_tdt(torch, store))
        assert torch.equal(t.float().cpu(), x)
        return t
    if quantizer:                                   # scales every row by a power of two: the cosines do not change
        from tristage_rag_amd.index import quantize_rows_fp8
        return quantize_rows_fp8(x.cuda())
    t = x.to(torch.float8_e4m3fn)
    assert torch.equal(t.float(), x)
    return t.cuda()


def _lay_out(data, cls, seed):
    """The candidates as a token store: three filler rows first, the candidates in a permuted order, a filler row
    between neighbours.  A filler row is a copy of a query token (cosine 1 with it) or, where every cosine is
    negative, an all-zero row (cosine 0): a kernel that reads a row outside its candidate returns a higher score."""
    rng = np.random.default_rng([seed, 13])
    n, Lq = len(data.docs), data.q.shape[0]
    H = data.q.shape[1]
    filler = lambda i: np.zeros((1, H), np.float32) if cls == "neg" else data.q[i % Lq][None]
    parts, starts, at = [filler(0), filler(1), filler(2)], np.zeros(n, np.int64), 3
    for c in rng.permutation(n):
        starts[c] = at
        parts += [data.docs[c], filler(int(c))]
        at += data.docs[c].shape[0] + 1
    return np.concatenate(parts, 0), starts


@functools.lru_cache(maxsize=2)
def _prepared(case):
    """Everything of a case that does not depend on the store type: guarded data, store layout, expected results."""
    d = em.generate(case)
    em.assert_exactly_scored(d.q, d.docs, d.plants)           # nothing reaches the GPU that is not exactly scored
    rows, starts = _lay_out(d, case.cls, case.seed)
    plan = em.batch_plan(case)
    batch_want = [(em.expected_maxsim(d.q[a:b], [d.docs[i] for i in pick]),
                   em.expected_colbert(d.q[a:b], [d.docs[i] for i in pick])) for (a, b), pick in plan]
    return d, rows, starts, em.expected_maxsim(d.q, d.docs), em.expected_colbert(d.q, d.docs), plan, batch_want


def _exact(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        i = int(bad[0])
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        print(f"\n{what}: {bad.size} of {got.size} differ; first at {i}: got {got[i]!r} want {want[i]!r}; "
              f"largest distance {int(ulps.max())} ulp, at most one ulp on {(ulps[bad] == 1).sum()} of them")
    assert np.array_equal(got, want), what
    return got


def _close(got, want64, what):
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - want64)
    print(f"\n{what}: colbert max |error| {err.max():.3e}")
    np.testing.assert_allclose(got, want64, atol=em.COLBERT_ATOL, rtol=0, err_msg=what)


_BITS = {}          # case name -> (store type, scores of both modes) of the first store type that ran it


@pytest.mark.parametrize("case,store", em.CASE_STORES, ids=em.CASE_STORE_IDS)
def test_every_entry_point_is_bit_exact(torch_mod, case, store):
    """`maxsim` (packed), `maxsim_indexed`, `maxsim_indexed_batch` with one query and with a ragged batch (an empty
    candidate list among them), both modes; the e4m3 store cast directly and built by quantize_rows_fp8."""
    torch = torch_mod
    from tristage_rag_amd.index import maxsim, maxsim_indexed, maxsim_indexed_batch
    d, rows, starts, want, want_c, plan, batch_want = _prepared(case)
    Lq, n = case.Lq, case.n
    assert em.kernel_path(case.H, store, Lq, "single") is not None
    if case.n == em.N_MANY:          # the equal-slice rule of the single-query launch, on this device
        assert em.slice_facts([d.lens.tolist()], "single", 1, _num_cus(torch))["eq_taken"]
    tq = _query(torch, d.q, store)
    stores = [_rows(torch, rows, store)]
    if store.startswith("e4m3"):
        stores.append(_rows(torch, rows, store, quantizer=True))
    t_starts = torch.from_numpy(starts).cuda()
    t_lens = torch.from_numpy(d.lens.astype(np.int32)).cuda()
    empty = d.lens == 0
    for ts in stores:
        got = _exact(maxsim_indexed(tq, ts, t_starts, t_lens), want, "maxsim_indexed")
        assert (got[empty] == 0.0).all()
        _exact(maxsim_indexed_batch(tq, [0, Lq], ts, t_starts, t_lens, [0, n]), want, "batch of one query")
        _close(maxsim_indexed(tq, ts, t_starts, t_lens, mode="colbert"), want_c, "maxsim_indexed")
        _close(maxsim_indexed_batch(tq, [0, Lq], ts, t_starts, t_lens, [0, n], mode="colbert"), want_c, "batch of one")
        # the ragged batch: a small grid, one wave walks several tiles across several candidates
        q_off = np.concatenate([[0], np.cumsum([b - a for (a, b), _ in plan])])
        c_off = np.concatenate([[0], np.cumsum([len(p) for _, p in plan])])
        bq = torch.cat([tq[a:b] for (a, b), _ in plan])
        pk = torch.from_numpy(np.concatenate([p for _, p in plan]).astype(np.int64)).cuda()
        got_b = maxsim_indexed_batch(bq, q_off, ts, t_starts[pk], t_lens[pk], c_off)
        got_bc = maxsim_indexed_batch(bq, q_off, ts, t_starts[pk], t_lens[pk], c_off, mode="colbert")
        assert any(len(p) == 0 for _, p in plan)
        for j, ((a, b), pick) in enumerate(plan):
            if len(pick) == 0:
                continue
            sl = slice(int(c_off[j]), int(c_off[j + 1]))
            _exact(got_b[sl], batch_want[j][0], f"ragged batch, query {j}")
            one = maxsim_indexed(tq[a:b], ts, t_starts[pk[sl]], t_lens[pk[sl]])
            assert torch.equal(one, got_b[sl]), f"batch against single, query {j}"
            _close(got_bc[sl], batch_want[j][1], f"ragged batch, query {j}")
            assert (got_b[sl].cpu().numpy()[d.lens[pick] == 0] == 0.0).all()
    if not store.startswith("e4m3"):                 # the packed form (no e4m3 form of it exists)
        packed = _rows(torch, np.concatenate([x for x in d.docs if x.shape[0]] or [rows[:0]], 0), store)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(d.lens)]).astype(np.int32)).cuda()
        got = _exact(maxsim(tq, packed, off), want, "maxsim (packed)")
        assert (got[empty] == 0.0).all()
        _close(maxsim(tq, packed, off, mode="colbert"), want_c, "maxsim (packed)")
    # the same case gives the same bits in every store type
    both = np.stack([maxsim_indexed(tq, stores[-1], t_starts, t_lens, mode=m).cpu().numpy() for m in ("maxsim", "colbert")])
    first = _BITS.setdefault(case.name, (store, both))
    assert np.array_equal(both[0], first[1][0]), (store, first[0])
    np.testing.assert_allclose(both[1], first[1][1], atol=2 * em.COLBERT_ATOL, rtol=0)     # (each within 2e-6 of float64)


STALE = [(c, s, f) for c in em.STALE for s in c.stores for f in ("single", "batch")]


@pytest.mark.parametrize("case,store,form", STALE, ids=[f"{c.name}-{s}-{f}" for c, s, f in STALE])
def test_a_launch_of_ones_leaves_nothing_for_a_launch_of_negatives(torch_mod, case, store, form):
    """Launch A: every candidate holds every query token (all maxima 1) and Lq = 65 takes two passes, so every
    candidate goes through the scratch cells.  Launch B, on the same stream: the same candidate count and lengths,
    every cosine <= 0.  A key A left behind would win B's atomicMax.  Then B again with fewer candidates and a
    shorter query (another lq_pad: other cells)."""
    torch = torch_mod
    from tristage_rag_amd.index import maxsim_indexed, maxsim_indexed_batch
    a = em.generate(case)
    em.assert_exactly_scored(a.q, a.docs)
    lens = tuple(a.lens.tolist())
    n2, lq2 = em.STALE_B2
    followers = [em.generate(case, "neg", lens), em.generate(case._replace(Lq=lq2, n=n2), "neg", lens[:n2])]
    assert em.m16_shape(case.H, store, case.Lq).passes >= 2

    def run(data, cls):
        rows, starts = _lay_out(data, cls, case.seed)
        tq, ts = _query(torch, data.q, store), _rows(torch, rows, store)
        t_s, t_l = torch.from_numpy(starts).cuda(), torch.from_numpy(data.lens.astype(np.int32)).cuda()
        n, Lq = len(data.docs), data.q.shape[0]
        if form == "single":
            return lambda: maxsim_indexed(tq, ts, t_s, t_l)
        h = n // 2                                   # two queries (the same tokens) on the two halves of the candidates
        return lambda: maxsim_indexed_batch(torch.cat([tq, tq]), [0, Lq, 2 * Lq], ts, t_s, t_l, [0, h, n])

    launch_a = run(a, "ones")
    for b in followers:
        em.assert_exactly_scored(b.q, b.docs)
        launch_b = run(b, "neg")
        got_a = launch_a()                           # enqueued back to back on the current stream
        got_b = launch_b()
        got_b2 = launch_b()
        assert (got_a.cpu().numpy() == 1.0).all()
        want = em.expected_maxsim(b.q, b.docs)
        assert (want <= 0).all() and (want < 0).any()
        _exact(got_b, want, "the launch after the ones")
        _exact(got_b2, want, "and once more")


def test_more_candidates_and_more_queries_than_one_launch_takes(torch_mod):
    """4100 one-token candidates (chunks of 4096 in the single form, the per-query fallback of the batch form) and
    70 queries of 3..20 candidates each (more than M16_MAX_BATCH: two launches, the second of six queries)."""
    torch = torch_mod
    from tristage_rag_amd.index import maxsim_indexed, maxsim_indexed_batch
    case = em.beyond_case()
    d = em.generate(case)
    em.assert_exactly_scored(d.q, d.docs, d.plants)
    assert case.n > em.M16_MAX_DOCS and em.BEYOND_QUERIES > em.M16_MAX_BATCH
    rows, starts = _lay_out(d, case.cls, case.seed)
    tq, ts = _query(torch, d.q, "bf16"), _rows(torch, rows, "bf16")
    t_s, t_l = torch.from_numpy(starts).cuda(), torch.from_numpy(d.lens.astype(np.int32)).cuda()
    want = em.expected_maxsim(d.q, d.docs)
    _exact(maxsim_indexed(tq, ts, t_s, t_l), want, "4100 candidates, single form")
    _exact(maxsim_indexed_batch(tq, [0, case.Lq], ts, t_s, t_l, [0, case.n]), want, "4100 candidates, batch form")
    # 70 ragged queries over a case of candidates of several tiles
    case = next(c for c in em.CASES if c.cls == "plant" and c.H == 64 and c.Lq == 33 and c.n == em.N_CAND)
    d = em.generate(case)
    em.assert_exactly_scored(d.q, d.docs, d.plants)
    rows, starts = _lay_out(d, case.cls, case.seed)
    tq, ts = _query(torch, d.q, "bf16"), _rows(torch, rows, "bf16")
    rng = np.random.default_rng(70)
    a = rng.integers(0, case.Lq, size=em.BEYOND_QUERIES)
    b = np.array([rng.integers(x + 1, case.Lq + 1) for x in a])
    picks = [rng.permutation(case.n)[: int(k)] for k in rng.integers(3, 21, size=em.BEYOND_QUERIES)]
    q_off = np.concatenate([[0], np.cumsum(b - a)])
    c_off = np.concatenate([[0], np.cumsum([len(p) for p in picks])])
    pk = np.concatenate(picks)
    got = maxsim_indexed_batch(torch.cat([tq[x:y] for x, y in zip(a, b)]), q_off, ts, torch.from_numpy(starts[pk]).cuda(),
                               torch.from_numpy(d.lens[pk].astype(np.int32)).cuda(), c_off)
    want = np.concatenate([em.expected_maxsim(d.q[x:y], [d.docs[i] for i in p]) for x, y, p in zip(a, b, picks)])
    _exact(got, want, "70 queries")
