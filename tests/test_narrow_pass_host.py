"""The case table of the narrow-pass tests (tests/narrow_pass_cases.py) checked without a GPU: every
index is in the 32-query regime by the documented border, the inputs are exactly summable and stored exactly, the
models agree with a brute-force float64 sort, the radii stay inside the candidate slots, and the rescore cases are
chunked by the host's own formula where no earlier case was."""
import numpy as np
import pytest

import bias_model as bm
import exact_inputs as ex
import handle_reuse_cases as hc
import narrow_pass_cases as nc
import range_model as rm

# one index per distinct (rows of the corpus, d): bf16 shares f16's rows
KINDS = tuple({(("ints" if ix.storage in ("f16", "bf16", "f32") else ix.storage), ix.d, ix.rows): ix
               for ix in nc.INDEXES}.values())
IDS = [ix.id for ix in KINDS]


def test_every_index_is_in_the_regime_and_the_control_is_not():
    for ix in nc.INDEXES:
        assert nc.queries_per_pass(ix.storage, ix.d) == 32, ix
    assert nc.queries_per_pass(*nc.CONTROL[:2]) == 64
    assert {ix.d for ix in nc.INDEXES if ix.storage in ("f16", "bf16")} == {1100, 2176}
    assert {ix.d for ix in nc.INDEXES if ix.storage == "f32"} == {600, 776}
    assert {ix.d for ix in nc.INDEXES if ix.storage in ("fp8", "fp4")} == {1280, 2048}
    assert all(ix.d == 1100 for ix in nc.INDEXES if ix.rows == "one")
    for s in ("f16", "bf16", "f32", "fp8", "fp4"):       # both widths dense, one of them on the filter path
        assert len({ix.d for ix in nc.INDEXES if ix.storage == s and ix.rows == "dense"}) == 2
        assert sum(ix.storage == s and ix.rows == "filter" for ix in nc.INDEXES) == 1
    assert nc.n_rows(nc.Ix("f16", 1100, "one"), 256) == ex.one_launch_rows(256) > nc.TIE0 + nc.TIE_N
    assert nc.TIE_N > nc.CAND_CAP and nc.SYNC_B == (32, 33, 64, 65) and nc.ASYNC_B == (128, 129)
    assert nc.IVF_CASES == (("f16", 1030), ("bf16", 1088)) and nc.NLIST == 8
    assert all(1024 < d <= 1088 < nc.IVF_REFUSED_D for _, d in nc.IVF_CASES)     # 16-bit lists in 32-query passes


@pytest.mark.parametrize("ix", KINDS, ids=IDS)
def test_inputs_are_exactly_summable_and_stored_exactly(ix):
    dat = nc.data(ix)
    n = nc.n_rows(ix)
    assert dat.corpus.shape == (n, ix.d) and dat.queries.shape[0] == nc.NQ + (nc.tie0_of(ix) is not None) and n % 32 != 0
    for r0 in range(0, n, 8192):
        ex.assert_exactly_summable(dat.corpus[r0:r0 + 8192], dat.queries, dat.unit)
    assert np.array_equal(dat.S.astype(np.float32).astype(np.float64), dat.S)
    assert np.abs(dat.S).max() + 2000 < 2 ** 24                      # score + bias stays an exact f32 integer
    b = nc.aux("b", n)
    assert np.array_equal(b, np.rint(b)) and np.abs(b).max() <= 2000
    c, q = dat.corpus, dat.queries
    if ix.storage in ("f16", "bf16", "f32"):
        assert np.array_equal(c.astype(np.float16).astype(np.float32), c)
        assert np.array_equal((c.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32), c)          # bf16 too
        assert np.array_equal(q.astype(np.float16).astype(np.float32), q)
    assert np.array_equal((q.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32), q)       # the bf16 query image
    if ix.storage in ("fp8", "fp4"):
        from tristage_rag_amd import index as ix_mod
        rows = c[:2000]
        if ix.storage == "fp8":
            got = ix_mod.decode_rows_e4m3_fixed(ix_mod.quantize_rows_e4m3_fixed_reference(rows, hc.FP8_SCALE_LOG2),
                                                hc.FP8_SCALE_LOG2)
        else:
            got = ix_mod.decode_rows_mxfp4(*ix_mod.quantize_rows_mxfp4_reference(rows), rows.shape[1])
        assert np.array_equal(got, rows)


def test_the_generalised_rows_are_those_of_the_handle_reuse_table():
    """gen_rows(storage, n, d) draws the value sets of handle_reuse_cases._rows (whose own host test pins them)."""
    for kind, storage in (("fp8", "fp8"), ("fp4", "fp4")):
        old = hc._rows(kind)[0][:4000]
        new = nc.gen_rows(storage, 4000, 256, 4)[0]
        assert set(np.unique(np.abs(new))) <= set(np.unique(np.abs(old))) and np.abs(new).max() == np.abs(old).max()
        if kind == "fp4":
            assert (np.abs(new[:, 0::64]) == 6).all() and (np.abs(new[:, 8::64]) == 6).all()


TIE_INDEXES = tuple(ix for ix in nc.INDEXES if nc.tie0_of(ix) is not None and ix.storage != "bf16")


def test_where_the_tie_blocks_are():
    """f16 / bf16: the one-launch corpus; fp32, fp8, fp4: the filter corpus.  Every storage type has one."""
    got = {ix.id: nc.tie0_of(ix) for ix in nc.INDEXES if nc.tie0_of(ix) is not None}
    assert got == {"f16-1100-one": nc.TIE0, "bf16-1100-one": nc.TIE0, "f32-776-filter": nc.TIE0_FILTER,
                   "fp8-2048-filter": nc.TIE0_FILTER, "fp4-1280-filter": nc.TIE0_FILTER}
    assert nc.TIE0_FILTER + nc.TIE_N < nc.N_FILTER and nc.TIE0_FILTER % 32 != 0
    for ix in nc.INDEXES:
        assert ("async_tie" in {v.name for v in nc.supported(ix)}) == (nc.tie0_of(ix) is not None), ix


@pytest.mark.parametrize("ix", TIE_INDEXES, ids=[ix.id for ix in TIE_INDEXES])
def test_copied_row_is_below_every_ordinary_threshold(ix):
    dat = nc.data(ix)
    t0 = nc.tie0_of(ix)
    assert dat.tie0 == t0
    c, S = dat.corpus, dat.S
    assert (c[t0:t0 + nc.TIE_N] == c[t0]).all() and np.array_equal(dat.queries[nc.TIE_Q], c[t0])
    tie = S[:nc.NQ, t0]
    assert (tie < 0).all()
    other = np.delete(S[nc.TIE_Q], np.arange(t0, t0 + nc.TIE_N))
    assert S[nc.TIE_Q, t0] > other.max()          # the copies are the tie query's best rows: every list overflows
    if ix.storage == "f16":
        assert (dat.Sp(1024)[:, t0] == 0).all()
    v = {x.name: x for x in nc.supported(ix)}["async_tie"]
    assert bool(v.opt.get("one_launch")) == (ix.rows == "one") and bool(v.opt.get("classic")) == (ix.rows != "one")
    qi, k = v.opt["subs"][nc.TIE_SUB]
    assert 32 <= qi.index(nc.TIE_Q) < 64 and len(qi) <= 64 and v.opt["failed"] == (nc.TIE_SUB,)     # its second pass
    assert [nc.TIE_Q in s[0] for s in v.opt["subs"]].count(True) == 1
    outs, failed = nc.expected(v, dat)
    assert np.array_equal(outs[2 * nc.TIE_SUB + 1][qi.index(nc.TIE_Q)], np.arange(t0, t0 + k))
    # every list an ordinary query asks for ends above the copied row's (boosted) score
    checked = 0
    for x in nc.supported(ix):
        lists = []
        if x.kind in ("search", "biased") and x.opt.get("allowed") != "few":
            lists = [(x.qi, nc.expected(x, dat)[0])]
        elif x.kind in ("grouped", "mmr"):
            lists = [(x.qi, nc._topk(S[list(x.qi)], x.opt["fetch_k"], None, None)[0])]
        elif x.kind == "async":
            want = nc.expected(x, dat)[0]
            lists = [(qi, want[2 * j]) for j, (qi, _) in enumerate(x.opt["subs"])]
        for qi, D in lists:
            for row, q in enumerate(qi):
                if q == nc.TIE_Q or D[row, -1] == -nc.FLT_MAX:
                    continue
                assert D[row, -1] > tie[q] + (5.0 if x.kind == "biased" else 0.0), (x.name, q)
                checked += 1
        if x.kind == "prefix":
            assert (nc.expected(x, dat)[0][:, -1] > 0).all(), x.name
    assert checked > 100


def test_table_sizes_and_batches():
    got = {ix.id: len(nc.supported(ix)) for ix in nc.INDEXES}
    assert got == nc.TABLE_SIZE, got
    for ix in nc.INDEXES:
        vs = nc.supported(ix)
        assert len({v.name for v in vs}) == len(vs)
        assert all(v.like in hc.BY_NAME for v in nc.variants(ix))
        sync = {len(v.qi) for v in vs if v.kind != "async"}
        assert sync == set(nc.SYNC_B), (ix, sync)                         # every synchronous batch size, nothing else
        assert {len(v.qi) for v in vs if v.kind == "search" and "allowed" not in v.opt} >= {33, 64, 65}
        for v in vs:
            if v.kind == "async":
                sizes = {len(qi) for qi, _ in v.opt["subs"]}
                assert len(v.opt["subs"]) == hc.BLOCK and set(nc.ASYNC_B) <= sizes and {33, 64, 65} <= sizes
                if v.opt.get("one_launch"):
                    assert max(k for _, k in v.opt["subs"]) <= 100
            for spec in ("tail", "head", "mix"):
                if v.opt.get("allowed") == spec and v.kind != "async":
                    names = nc.allowed_names(spec, len(v.qi))
                    assert len(set(names[:32])) != len(set(names)) or spec == "mix"
        if ix.storage in ("f16", "bf16"):
            dims = {v.opt["dims"] for v in vs if v.kind == "prefix"}
            assert dims == ({128, 1024, 2048} if ix.d == 2176 else {128, 1024})
            assert {v.opt["fetch_k"] for v in vs if v.kind == "funnel"} == {None, 4000}
        # the refusals: what the storage type does not take and the binding refuses
        kinds = {v.kind for v in nc.refused(ix)}
        want = {"f16": set(), "bf16": set(), "f32": {"biased", "prefix", "funnel"},
                "fp8": {"biased", "range", "prefix", "funnel"}, "fp4": {"biased", "range", "prefix", "funnel", "mmr"}}
        assert kinds == want[ix.storage], (ix, kinds)
    t = nc.allowed_names("tail", 64)
    assert t[:32] == [None] * 32 and t[32:] == ["m30"] * 32
    h = nc.allowed_names("head", 65)
    assert h[:32] == ["m50"] * 32 and h[32:] == [None] * 33
    assert set(nc.allowed_names("mix", 33)) == {"m30", "m50", "mod5", None}
    assert nc.aux("few", nc.N_DENSE).sum() == 37


@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("ix", KINDS, ids=IDS)
def test_models_agree_with_a_brute_force_sort_on_a_cut(ix, live):
    """The first 200 rows of every case: each model against a per-query Python sort of the float64 scores."""
    full = nc.data(ix)
    n = 200
    S = full.S[:, :n]
    lv = nc.aux("live", n) if live else None
    for spec, nq, k in ((None, 33, 7), ("tail", 64, 20), ("mix", 33, 300), ("few", 33, 50)):
        allowed = nc.allowed_of(spec, nq, n)
        ok = np.ones((nq, n), dtype=bool) if lv is None else np.tile(lv, (nq, 1))
        for b in range(nq):
            m = allowed[b] if isinstance(allowed, list) else allowed
            if m is not None:
                ok[b] &= m
        want = nc.brute_force_topk(S[:nq], k, ok)
        got = nc._topk(S[:nq], k, lv, allowed)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), spec
        # boosted: the same sort over score + bias
        b32 = nc.aux("b", n)
        gb = bm.topk_model(S[:nq].astype(np.float32), b32, k, live=lv, allowed=allowed)
        wb = nc.brute_force_topk(S[:nq] + b32.astype(np.float64)[None, :], k, ok)
        assert np.array_equal(gb[0], wb[0]) and np.array_equal(gb[1], wb[1]), spec
        # range: every row at or above the radius, ascending ids
        if spec != "few":
            rad = rm.rank_radius(*hc._as_inputs(S[:nq]), 3 + np.arange(nq) % 5, live=lv, allowed=allowed)
            lims, D, I = rm.expected_range(*hc._as_inputs(S[:nq]), rad, live=lv, allowed=allowed)
            for b in range(nq):
                rows = [r for r in range(n) if ok[b, r] and S[b, r] >= float(rad[b])]
                assert I[lims[b]:lims[b + 1]].tolist() == rows and len(rows) >= 3
                assert np.array_equal(D[lims[b]:lims[b + 1]], S[b, rows].astype(np.float32))


@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("ix", KINDS, ids=IDS)
def test_references_are_well_defined(ix, live):
    dat = nc.data(ix)
    n = dat.n
    lv = nc.aux("live", n) if live else None
    vs = [v for v in nc.supported(ix) if not live or v.name in nc.TOMBSTONE]
    assert not live or len(vs) >= 3
    for v in vs:
        if v.kind == "range":
            lims, D, I = nc.expected(v, dat, live=lv)
            counts = np.diff(lims)
            ranks = nc.ranks_of(len(v.qi))
            assert len(set(ranks[:32])) > 1 and (len(ranks) == 33 or len(set(ranks[32:])) > 1)   # on both sides of the border
            assert ranks[32] != ranks[0]
            every = v.opt.get("all_at")
            n_live = n if lv is None else int(lv.sum())
            for b, c in enumerate(counts):
                if b == every:           # every live row: above the slots on the filter corpora (a dense redo)
                    assert c == n_live and (c > nc.CAND_CAP) == (ix.rows != "dense")
                else:                    # the rank, plus ties at the radius: no limit error, no redo from the inputs
                    assert ranks[b] <= c < ranks[b] + 20 and 1 <= c <= nc.CAND_CAP
            if every is not None:
                assert every == 32       # the first query of the second pass
        elif v.kind == "async":
            outs, failed = nc.expected(v, dat, live=lv)
            assert len(outs) == 2 * len(v.opt["subs"])
            for j, (qi, k) in enumerate(v.opt["subs"]):
                assert outs[2 * j].shape == (len(qi), k)
        elif v.kind in ("search", "biased", "prefix", "funnel"):
            D, I = nc.expected(v, dat, live=lv)
            assert D.shape == I.shape == (len(v.qi), v.k)
            if lv is not None:
                assert lv[I[I >= 0]].all()
            if v.opt.get("allowed") == "few":
                assert ((I >= 0).sum(axis=1) == 37).all() and v.k > 37
            elif v.k <= n // 8:
                assert (I >= 0).all(), v.name
            else:
                assert v.k == n + 3 and ((I >= 0).sum(axis=1) == n).all()           # the padding behind the last row
        elif v.kind == "grouped":
            D, I, G = nc.expected(v, dat, live=lv)
            assert all(len(set(g[g >= 0])) == v.k for g in G)
        elif v.kind == "mmr":                 # (hc._mmr asserts mmr_model's own 2^22 bound on the gram and scores)
            D, I = nc.expected(v, dat, live=lv)
            assert (I >= 0).all() and all(len(set(r)) == v.k for r in I.tolist())
        elif v.kind == "scores":
            assert nc.expected(v, dat, live=lv)[0].shape == (65, n)
        else:
            raise AssertionError(v.kind)


# ------------------------------------------------------------------------------------------------ rescore chunk rule
def test_rescore_cases_are_chunked_and_no_earlier_case_was():
    for storage, d, B, C in nc.RESCORE_CHUNKED:
        qc, qp = nc.rescore_chunk(storage, d, B, C)
        assert qc < min(B, qp), (d, B, C, qc)
        starts = nc.chunk_starts(storage, d, B, C)
        assert any(c0 > 0 for _, c0, _ in starts)                              # col0 > 0 is launched
        first_pass = [s for s in starts if s[0] == 0]
        assert first_pass[-1][2] < qc and sum(s[2] for s in starts) == B       # a last chunk shorter than qc
    # the figures of the cases, by the formula
    assert nc.rescore_chunk("f16", 768, 64, 4096) == (63, 64)
    assert [s[1:] for s in nc.chunk_starts("f16", 768, 64, 4096)] == [(0, 63), (63, 1)]
    assert nc.rescore_chunk("bf16", 768, 64, 16384) == (15, 64)
    assert (30, 15) in [s[1:] for s in nc.chunk_starts("bf16", 768, 64, 16384)]     # columns 30..44: both image halves
    assert nc.rescore_chunk("f16", 1100, 33, 8192) == (21, 32)
    assert nc.chunk_starts("f16", 1100, 33, 8192) == [(0, 0, 21), (0, 21, 11), (32, 0, 1)]
    assert nc.rescore_chunk("bf16", 1100, 33, 16384) == (10, 32)
    assert nc.rescore_chunk("f16", 2176, 32, 4096) == (22, 32)
    for d, B, C in nc.RESCORE_BEFORE:                                          # the gap was real
        qc, qp = nc.rescore_chunk("f16", d, B, C)
        assert qc >= min(B, qp), (d, B, C)


def test_rescore_inputs():
    for d in sorted({c[1] for c in nc.RESCORE_CHUNKED}):
        dat = nc.rescore_data(d)
        ex.assert_exactly_summable(dat.corpus, dat.queries, dat.unit)
    live = nc.aux("live", nc.RESCORE_N)
    ids = nc.rescore_candidates(33, 4096, nc.RESCORE_N, live, 1)
    for b in range(33):
        row = ids[b]
        assert (row == -1).any() and (row == nc.RESCORE_N + 5).any() and (row == -9).any() and row[0] == row[-1]
        ok = (row >= 0) & (row < nc.RESCORE_N)
        assert (~live[row[ok]]).any()
