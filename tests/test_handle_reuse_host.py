"""The case table of the handle-reuse tests (tests/handle_reuse_cases.py) checked without a GPU: the
inputs are exactly summable and stored exactly, the copied row stays below every ordinary query's threshold, every
variant's reference is well defined and has the counts its name claims, and the block sequence holds every ordered pair
of variants."""
import numpy as np
import pytest

import exact_inputs as ex
import handle_reuse_cases as hc

KINDS = ("f16", "f32", "fp8", "fp4")       # bf16 shares f16's rows


@pytest.mark.parametrize("storage", KINDS)
def test_inputs_are_exactly_summable_and_stored_exactly(storage):
    dat = hc.data(storage)
    assert dat.corpus.shape == (hc.N, hc.STORAGE_D[storage]) and dat.queries.shape[0] == hc.NQ + 1
    assert hc.N >= ex.one_launch_rows(256) and hc.N >= 32 * 2048 and hc.N % 32 != 0
    for r0 in range(0, hc.N, 8192):        # the condition is one per row: in chunks, without a float64 corpus
        ex.assert_exactly_summable(dat.corpus[r0:r0 + 8192], dat.queries, dat.unit)
    assert np.array_equal(dat.S, hc.chunked_scores(dat.corpus, dat.queries, step=5000))
    assert np.array_equal(dat.S.astype(np.float32).astype(np.float64), dat.S)
    c = dat.corpus
    if storage == "f16":
        assert np.array_equal(c.astype(np.float16).astype(np.float32), c)
        assert np.array_equal((c.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32), c)          # bf16 too
    if storage in ("fp8", "fp4"):
        from tristage_rag_amd import index as ix
        q = dat.queries
        assert np.array_equal((q.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32), q)   # bf16 query image
        if storage == "fp8":
            rows = np.concatenate([c[:3000], c[hc.TIE0:hc.TIE0 + 2]])
            got = ix.decode_rows_e4m3_fixed(ix.quantize_rows_e4m3_fixed_reference(rows, hc.FP8_SCALE_LOG2), hc.FP8_SCALE_LOG2)
        else:
            rows = c
            got = ix.decode_rows_mxfp4(*ix.quantize_rows_mxfp4_reference(rows), rows.shape[1])
        assert np.array_equal(got, rows)


@pytest.mark.parametrize("storage", KINDS)
def test_copied_row_is_below_every_ordinary_threshold(storage):
    dat = hc.data(storage)
    c, S = dat.corpus, dat.S
    assert (c[hc.TIE0:hc.TIE0 + hc.TIE_N] == c[hc.TIE0]).all() and hc.TIE_N > hc.CAND_CAP
    assert np.array_equal(dat.queries[hc.TIE_Q], c[hc.TIE0])
    tie_score = S[:hc.NQ, hc.TIE0]
    assert (tie_score < 0).all()
    # the tie query: the copies are its best rows by far, so any threshold lets all 20 000 through
    other = np.delete(S[hc.TIE_Q], np.arange(hc.TIE0, hc.TIE0 + hc.TIE_N))
    assert S[hc.TIE_Q, hc.TIE0] > other.max()
    if dat.Sp is not None:
        assert (dat.Sp[:, hc.TIE0] == 0).all()
    # every list an ordinary query asks for, with the k it asks for, ends above the copied row's (boosted) score
    checked = 0
    for v in hc.variants_of(storage):
        lists = []
        if v.kind == "async":
            want, _ = hc.expected(v, dat)
            lists = [(qi, want[2 * j]) for j, (qi, _) in enumerate(v.opt["subs"])]
        elif v.kind in ("search", "biased", "prefix"):
            lists = [(v.qi, hc.expected(v, dat)[0])]
        elif v.kind in ("funnel", "grouped", "mmr"):
            which = "Sp" if v.kind == "funnel" else "S"
            lists = [(v.qi, hc._topk_of(dat, which, v.qi, v.opt["fetch_k"], None, v.opt.get("allowed"))[0])]
        for qi, D in lists:
            for row, q in enumerate(qi):
                if q == hc.TIE_Q or D[row, -1] == -hc.FLT_MAX:      # (a mask that leaves fewer than k rows has no k-th score)
                    continue
                bound = 0.0 if v.kind in ("prefix", "funnel") else tie_score[q] + (5.0 if v.kind == "biased" else 0.0)
                if v.kind == "biased" and v.opt["bias"] == "b":
                    bound = tie_score[q] + 2000.0
                assert D[row, -1] > bound, (v.name, q)
                checked += 1
    assert checked > 100


def _sorted_desc_then_id(D, I):
    ok = I >= 0
    assert (ok[:, :-1] >= ok[:, 1:]).all()                           # padding only at the end
    assert (D[~ok] == -hc.FLT_MAX).all()
    d, i = D.astype(np.float64), I.astype(np.float64)
    pair = ok[:, :-1] & ok[:, 1:]
    assert ((d[:, :-1] > d[:, 1:]) | ((d[:, :-1] == d[:, 1:]) & (i[:, :-1] < i[:, 1:])) | ~pair).all()


@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("storage", KINDS)
def test_references_are_well_defined(storage, live):
    dat = hc.data(storage)
    lv = hc.aux("live") if live else None
    names = hc.TOMBSTONE if live else None
    for v in hc.variants_of(storage, names):
        want = hc.expected(v, dat, live=lv)
        allowed = hc.allowed_of(v.opt.get("allowed"), len(v.qi))
        if v.kind == "async":
            outs, failed = want
            assert len(outs) == 2 * hc.BLOCK == 2 * len(v.opt["subs"])
            for j, (qi, k) in enumerate(v.opt["subs"]):
                assert outs[2 * j].shape == (len(qi), k)
                _sorted_desc_then_id(outs[2 * j], outs[2 * j + 1])
            assert failed == tuple(j for j, (qi, _) in enumerate(v.opt["subs"]) if hc.TIE_Q in qi)
        elif v.kind in ("search", "biased", "prefix", "rescore", "funnel"):
            D, I = want
            assert D.shape == I.shape == (len(v.qi), v.k)
            if v.kind != "rescore":
                _sorted_desc_then_id(D, I)
            if lv is not None:
                assert lv[I[I >= 0]].all()
            if v.opt.get("allowed") == "few":
                assert hc.aux("few").sum() == 37 < v.k and ((I >= 0).sum(axis=1) == 37).all()
            elif v.kind != "rescore":
                assert (I >= 0).all()
            if hc.TIE_Q in v.qi and lv is None:                      # equal scores: ascending ids, nothing else
                row = v.qi.index(hc.TIE_Q)
                assert np.array_equal(I[row], np.arange(hc.TIE0, hc.TIE0 + v.k))
        elif v.kind == "range":
            counts = want[0] if v.opt.get("raises") else np.diff(want[0])
            if "rank" in v.opt:            # a few hundred per query (ties at the radius add a few), far below the cap
                assert (counts >= v.opt["rank"]).all() and (counts < v.opt["rank"] + 50).all()
            else:                          # every live row: above the cap, so the pass is redone densely
                n_live = hc.N if lv is None else int(lv.sum())
                assert (counts == n_live).all() and n_live > hc.CAND_CAP and counts.sum() <= v.opt["max_results"]
            if v.opt.get("raises"):
                assert counts.sum() > v.opt["max_results"] and counts.max() <= hc.CAND_CAP
            else:
                lims, D, I = want
                for b in range(len(v.qi)):
                    d, i = D[lims[b]:lims[b + 1]], I[lims[b]:lims[b + 1]]
                    if v.opt.get("sort"):
                        _sorted_desc_then_id(d[None, :], i[None, :])
                    else:
                        assert (np.diff(i) > 0).all()
                    if allowed is not None:
                        assert hc.aux(v.opt["allowed"])[i].all()
        elif v.kind == "scores":
            assert want[0].shape == (len(v.qi), hc.N) and want[0].dtype == np.float32
        elif v.kind == "grouped":
            D, I, G = want
            assert D.shape == (len(v.qi), v.k * v.opt["group_size"])
            assert np.array_equal(G[I >= 0], hc.aux("groups")[I[I >= 0]]) and (G[I < 0] == -1).all()
            assert all(len(set(g[g >= 0])) == v.k for g in G)        # k distinct groups: one round is enough
        elif v.kind == "mmr":
            D, I = want
            assert D.shape == (len(v.qi), v.k) and (I >= 0).all()
            assert all(len(set(r)) == v.k for r in I.tolist())
        else:
            raise AssertionError(v.kind)


def test_masks_leave_what_they_say():
    m30, m05, m97, few = (hc.aux(n) for n in ("m30", "m05", "mod97", "few"))
    assert 0.29 < m30.mean() < 0.31 and 0.04 < m05.mean() < 0.06 and m97.sum() == -(-hc.N // 97) and few.sum() == 37
    per = hc.allowed_of("perq", 33)
    assert sum(m is None for m in per) == 8 and len({id(m) for m in per if m is not None}) == 3
    live = hc.aux("live")
    assert live.sum() == hc.N - -(-hc.N // 3)
    assert live[hc.TIE0:hc.TIE0 + hc.TIE_N].sum() < hc.CAND_CAP      # after the removal nothing overflows
    b, bt = hc.aux("b"), hc.aux("btie")
    assert np.array_equal(b, np.rint(b)) and np.array_equal(bt, np.rint(bt)) and np.abs(b).max() <= 2000
    for storage in ("f16",):                                         # score + bias stays an exact f32 integer
        assert np.abs(hc.data(storage).S).max() + 2000 < 2 ** 24


def test_table_sizes_and_shapes():
    for storage, size in hc.TABLE_SIZE.items():
        vs = hc.variants_of(storage)
        assert len(vs) == size
        assert set(hc.TOMBSTONE) <= set(hc.SUPPORTED["f16"]) and set(hc.CONCURRENT) <= set(hc.SUPPORTED["f16"])
        assert len(hc.CONCURRENT) == 9
        # neighbours differ in (nq, k), and both orders occur: large then small, small then large
        shapes = [(len(v.qi), v.k) for v in vs if v.kind != "async"]
        assert all(a != b for a, b in zip(shapes[:-1], shapes[1:]))
        steps = [np.sign(a[0] * max(a[1], 1) - b[0] * max(b[1], 1)) for a, b in zip(shapes[:-1], shapes[1:])]
        assert 1 in steps and -1 in steps
    for v in hc.VARIANTS:
        if v.kind == "async":
            assert len(v.opt["subs"]) == hc.BLOCK
            if v.opt.get("one_launch"):
                assert max(k for _, k in v.opt["subs"]) <= 100
        elif v.opt.get("one_launch"):
            assert v.k <= 100


@pytest.mark.parametrize("storage", sorted(hc.SUPPORTED))
def test_block_sequences_hold_every_ordered_pair(storage):
    names = list(hc.SUPPORTED[storage])
    want = {(a, b) for a in names for b in names if a != b}
    for parts in (1, 2, 3):
        got = set()
        for a in names:
            seqs = hc.split_sequence(names, a, parts)
            assert all(s[0] == a and s[::2] == [a] * (len(s) // 2) for s in seqs)
            assert sorted(b for s in seqs for b in s[1::2]) == sorted(n for n in names if n != a)
            for s in seqs:
                got |= hc.pairs_of(s)
        assert got == want
    assert hc.split_sequence(names, names[0], 1) == [hc.sequence(names, names[0])]
    assert hc.pairs_of(["a", "b", "a", "c"]) == {("a", "b"), ("b", "a"), ("a", "c")}
