"""Best passage per hit, without a GPU: the float64 model against a brute-force loop and against the
MaxSim oracle, the planted expectations, the exactness claim of the exact inputs, the argument refusals of both C
entry points and of the Python wrappers, and HashTokenizer.offsets."""
import ctypes
import re

import numpy as np
import pytest

import exact_maxsim_inputs as X
import passage_model as pm


def _brute(q, d, w):
    """triple loop, float64"""
    Lq, Ld = q.shape[0], d.shape[0]
    c = pm.cosines(q, d)
    we = min(w, Ld)
    best, best_p = None, -1
    scores = []
    for p in range(Ld - we + 1):
        s = 0.0
        for t in range(Lq):
            m = c[t, p]
            for j in range(p, p + we):
                if c[t, j] > m:
                    m = c[t, j]
            s += m
        scores.append(s)
        if best is None or s > best:
            best, best_p = s, p
    align = []
    for t in range(Lq):
        bj = best_p
        for j in range(best_p, best_p + we):
            if c[t, j] > c[t, bj]:
                bj = j
        align.append(bj)
    return best_p, we, best / Lq, np.array(align), np.array(scores)


def test_model_equals_a_brute_force_triple_loop_for_every_window():
    rng = np.random.default_rng(5)
    for Ld in range(1, 13):
        for Lq in range(1, 6):
            q = rng.integers(-2, 3, size=(Lq, 6)).astype(np.float64)       # small integers: ties and zero rows occur
            d = rng.integers(-2, 3, size=(Ld, 6)).astype(np.float64)
            for w in range(1, Ld + 3):
                got = pm.passage(q, d, w)
                p, we, sc, al, S = _brute(q, d, w)
                # (sums of the same float64 terms in the same order of t: equal, not merely close)
                assert (got.start, got.length) == (p, we), (Ld, Lq, w)
                assert np.allclose(got.window_scores, S, rtol=0, atol=1e-12)
                assert abs(got.score - sc) <= 1e-12
                assert np.array_equal(got.align, al)


def test_a_window_of_the_whole_document_reproduces_the_maxsim_oracle():
    from oracle import oracle
    rng = np.random.default_rng(6)
    for Ld, Lq in ((1, 1), (7, 3), (40, 12), (192, 32)):
        q = rng.standard_normal((Lq, 16)).astype(np.float32)
        d = rng.standard_normal((Ld, 16)).astype(np.float32)
        for w in (Ld, Ld + 1, 4096):
            got = pm.passage(q, d, w)
            assert (got.start, got.length) == (0, Ld)
            assert abs(got.score - oracle.maxsim_numpy(q, d)) <= 1e-12


def test_empty_candidate_list_and_batch_forms():
    rng = np.random.default_rng(7)
    q = rng.standard_normal((3, 8))
    docs = [rng.standard_normal((5, 8)), np.zeros((0, 8)), rng.standard_normal((2, 8))]
    got = pm.passages(q, docs, 2)
    assert (got[1].start, got[1].length, got[1].score) == (-1, 0, -pm.FLT_MAX) and (got[1].align == -1).all()
    assert got[0].start == pm.passage(q, docs[0], 2).start and got[2].length == 2
    flat = pm.passages_batch([q, q[:1]], [docs, docs[:1]], 2)
    assert len(flat) == 4 and flat[3].start == pm.passage(q[:1], docs[0], 2).start
    assert pm.passage_valid((-1, 0, -pm.FLT_MAX, None), got[1], pm.TOL_F32)
    assert not pm.passage_valid((0, 0, -pm.FLT_MAX, None), got[1], pm.TOL_F32)


@pytest.mark.parametrize("case", pm.planted_cases(), ids=lambda c: c.name)
def test_planted_expectations_hold_in_the_model(case):
    X.assert_exactly_scored(case.q, [case.doc])
    got = pm.passage(case.q, case.doc, case.w)
    assert got.start == case.want_start and got.length == case.w
    S = got.window_scores
    assert S[case.want_start] == 4.0                                   # the m = 4 tokens of the cluster, cosine 1 each
    if "duplicate" in case.name:
        assert (S == S.max()).sum() == 2 and np.flatnonzero(S == S.max())[0] == case.want_start
    else:
        assert (S == S.max()).sum() == 1, "the best start is not unique"
    assert (np.delete(S, np.flatnonzero(S == S.max())) <= 3.0).all()   # no other window holds more than m - 1
    # every cluster token is aligned to its own copy
    c = got.cos
    assert (c[np.arange(4), got.align[:4]] == 1.0).all()


def test_passage_valid_accepts_a_near_tie_and_rejects_a_wrong_span():
    q = np.eye(2)
    d = np.array([[1.0, 0.0], [1.0, 1e-7], [0.0, 1.0], [0.3, 0.3]])
    m = pm.passage(q, d, 1)
    ok = (m.start, 1, m.score, m.align)
    assert pm.passage_valid(ok, m, pm.TOL_F32)
    far = int(np.argmin(m.window_scores))
    assert not pm.passage_valid((far, 1, m.window_scores[far] / 2, np.array([far, far])), m, pm.TOL_F32)
    assert not pm.passage_valid((m.start, 1, m.score + 1e-4, m.align), m, pm.TOL_16)          # score off
    assert not pm.passage_valid((m.start, 1, m.score, m.align + 1), m, pm.TOL_F32)            # alignment outside
    assert not pm.passage_valid((m.start, 2, m.score, m.align), m, pm.TOL_F32)                # wrong length
    near = pm.passage(np.eye(2), np.array([[1.0, 1.0], [1.0, 1.0 + 1e-9]]), 1)                # two windows 1e-9 apart
    other = 1 - near.start
    assert pm.passage_valid((other, 1, near.window_scores[other] / 2, np.array([other, other])), near, pm.TOL_F32)


def _f32_sums(c32, we, order):
    """S[p] in float32, adding the window maxima in the given order of t"""
    win = np.lib.stride_tricks.sliding_window_view(c32, we, axis=1).max(axis=2)     # [Lq, npos] float32, exact maxima
    s = np.zeros(win.shape[1], np.float32)
    for t in order:
        s = (s + win[t]).astype(np.float32)
    return s


def test_window_sums_of_the_exact_inputs_do_not_depend_on_the_order_of_summation():
    """The exactness claim: every cosine is a multiple of 2^-10, so every window sum of every exact launch and
    planted case gives the same fp32 bits added in ascending and in descending t, and those are the float64 sums."""
    work = [(c.q, [c.doc], (c.w,)) for c in pm.planted_cases()]
    work += [(*pm.launch_data(L), L.windows) for L in pm.exact_launches() if max(L.lens) <= 192]
    for q, docs, windows in work:
        X.assert_exactly_scored(q, docs)
        Lq = q.shape[0]
        assert Lq <= 192
        for d in docs:
            if d.shape[0] == 0:
                continue
            c = pm.cosines(q, d)
            c32 = c.astype(np.float32)
            assert np.array_equal(c32.astype(np.float64), c) and np.array_equal(np.rint(c * 1024), c * 1024)
            for w in windows:
                we = min(w, d.shape[0])
                up = _f32_sums(c32, we, range(Lq))
                down = _f32_sums(c32, we, range(Lq - 1, -1, -1))
                assert np.array_equal(up.view(np.uint32), down.view(np.uint32))
                assert np.array_equal(up.astype(np.float64), pm.passage(q, d, w).window_scores)


def test_exact_launch_table_covers_the_issue_s_sizes():
    Ls = pm.exact_launches()
    assert {L.H for L in Ls} == {64, 72, 768}
    assert {1, 2, 31, 32, 33, 63, 64, 65, 192, 1024} <= {x for L in Ls for x in L.lens}
    assert {1, 31, 32, 33, 64, 65, 192} <= {L.Lq for L in Ls}
    assert {1, 2, 31, 32, 33, 191, 192, 193, 4096} <= {w for L in Ls for w in L.windows}
    assert all(len(L.lens) <= 40 for L in Ls)
    for L in Ls:                                      # a zero-length candidate between two real ones
        z = L.lens.index(0) if 0 in L.lens else None
        assert z is None or (0 < z < len(L.lens) - 1 and L.lens[z - 1] > 0 and L.lens[z + 1] > 0)
    assert sum(0 in L.lens for L in Ls) >= 2


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_library_exports_the_entry_points():
    from tristage_rag_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    for name in ("ts_maxsim_passages_indexed", "ts_maxsim_passages_indexed_batch"):
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "src/stage2_rescorer.py:167-183" in text and "no `colbert` form" in text


def test_entry_points_validate_arguments_without_a_gpu():
    from tristage_rag_amd import _lib
    lib = _lib.load()
    INV, UNS, OK = _lib.TS_ERR_INVALID, _lib.TS_ERR_UNSUPPORTED, _lib.TS_OK
    p = ctypes.c_void_p(4096)            # aligned, never dereferenced: the calls fail first
    odd = ctypes.c_void_p(4100)
    BF, F32, E4 = _lib.TS_BF16, _lib.TS_F32, _lib.TS_FP8_E4M3
    one = lib.ts_maxsim_passages_indexed

    def single(q=p, Lq=4, store=p, starts=p, lens=p, n=3, H=64, dt=BF, w=8, o1=p, o2=p, o3=p, al=None):
        return one(q, Lq, store, starts, lens, n, H, dt, w, o1, o2, o3, al, 0, None)
    for kw in ({"q": None}, {"store": None}, {"starts": None}, {"lens": None}, {"o1": None}, {"o2": None}, {"o3": None}):
        assert single(**kw) == INV, kw
        assert b"null pointer" in lib.ts_last_error()
    assert single(w=0) == INV and b"window" in lib.ts_last_error()
    assert single(w=-3) == INV
    assert single(n=-1) == INV
    assert single(Lq=0) == INV and single(Lq=-1) == INV
    assert single(H=0) == INV and single(dt=9) == INV
    assert single(Lq=257) == UNS and b"256" in lib.ts_last_error()
    assert single(H=60, dt=BF) == UNS and b"multiple of 16" in lib.ts_last_error()        # 120 bytes
    assert single(H=6, dt=F32) == UNS                                                      # 24 bytes
    assert single(dt=E4) == UNS and b"e4m3" in lib.ts_last_error()
    assert single(q=odd) == UNS and single(store=odd) == UNS
    assert single(n=0) == OK and single(n=0, al=p) == OK       # nothing to do is not an error

    many = lib.ts_maxsim_passages_indexed_batch
    off = (ctypes.c_int32 * 3)(0, 4, 9)
    co = (ctypes.c_int32 * 3)(0, 2, 5)
    none = (ctypes.c_int32 * 3)(0, 0, 0)
    dec = (ctypes.c_int32 * 3)(0, 4, 3)
    late = (ctypes.c_int32 * 3)(1, 4, 9)
    long_q = (ctypes.c_int32 * 3)(0, 4, 261)

    def batch(q=p, qo=off, nq=2, store=p, starts=p, lens=p, c=co, H=64, dt=BF, w=8, o1=p, o2=p, o3=p, al=None, ld=5):
        return many(q, qo, nq, store, starts, lens, c, H, dt, w, o1, o2, o3, al, ld, 0, None)
    for kw in ({"q": None}, {"qo": None}, {"store": None}, {"starts": None}, {"lens": None}, {"c": None},
               {"o1": None}, {"o2": None}, {"o3": None}):
        assert batch(**kw) == INV, kw
    assert batch(w=0) == INV and batch(nq=-1) == INV
    assert batch(qo=dec) == INV and b"non-decreasing" in lib.ts_last_error()
    assert batch(c=dec) == INV
    assert batch(qo=late) == INV and b"start at 0" in lib.ts_last_error()
    assert batch(qo=none) == INV and b"no tokens" in lib.ts_last_error()      # candidates, but an empty query
    assert batch(al=p, ld=4) == INV and b"align_ld" in lib.ts_last_error()     # the longest query has 5 tokens
    assert batch(qo=long_q) == UNS
    assert batch(H=60) == UNS and batch(dt=E4) == UNS and batch(q=odd) == UNS
    assert batch(nq=0) == OK and batch(c=none) == OK


def test_python_argument_errors_are_raised_before_anything_is_launched():
    """The wrappers refuse on the host (CPU tensors here: nothing could be launched)."""
    import torch
    from tristage_rag_amd.index import maxsim_passages_indexed, maxsim_passages_indexed_batch, passage_check
    q = torch.zeros((4, 64), dtype=torch.bfloat16)
    store = torch.zeros((10, 64), dtype=torch.bfloat16)
    starts, lens = torch.tensor([0, 5]), torch.tensor([5, 5], dtype=torch.int32)
    for w in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            maxsim_passages_indexed(q, store, starts, lens, w)
    with pytest.raises(ValueError, match="1024"):
        maxsim_passages_indexed(q, store, starts, torch.tensor([5, 1025], dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="1024"):
        maxsim_passages_indexed(q, store, starts, lens, 8, max_len=2000)
    with pytest.raises(ValueError, match="256"):
        maxsim_passages_indexed(torch.zeros((257, 64), dtype=torch.bfloat16), store, starts, lens, 8)
    with pytest.raises(ValueError, match="16 bytes"):
        maxsim_passages_indexed(torch.zeros((4, 60), dtype=torch.bfloat16), torch.zeros((10, 60), dtype=torch.bfloat16),
                                starts, lens, 8)
    with pytest.raises(NotImplementedError):
        maxsim_passages_indexed(q, torch.zeros((10, 64), dtype=torch.uint8).view(torch.float8_e4m3fn), starts, lens, 8)
    with pytest.raises(ValueError):
        maxsim_passages_indexed(q[:0], store, starts, lens, 8)
    with pytest.raises(ValueError):
        maxsim_passages_indexed_batch(q, [0, 4], store, starts, lens, [0, 1], 8)             # offsets vs starts / lens
    with pytest.raises(ValueError):
        maxsim_passages_indexed_batch(q, [0, 0, 4], store, starts, lens, [0, 1, 2], 8)       # candidates, no tokens
    passage_check(8, 64, store, 256, 1024)


def test_pipeline_refusals_and_config_defaults(tmp_path):
    from tristage_rag_amd.parallel_pipeline import ShardedRetrievalPipeline
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    from tristage_rag_amd.stage2_rescorer import Stage2Config
    assert PipelineConfig().passage_window is None and Stage2Config().passage_window is None
    p = RetrievalPipeline(config=PipelineConfig(log_file=str(tmp_path / "log")))
    for bad in (0, -2, 1.5, True, "8"):
        with pytest.raises(ValueError):
            p._passage_window(bad)
    assert p._passage_window(None) is None and p._passage_window(8) == 8
    sp = ShardedRetrievalPipeline(config=PipelineConfig(log_file=str(tmp_path / "log2")))
    with pytest.raises(NotImplementedError):
        sp.search("q", passages=8)
    with pytest.raises(NotImplementedError):
        sp.search_many(["q"], passages=8)
    with pytest.raises(NotImplementedError):
        sp.batch_search(["q"], passages=8)
    sp.config.passage_window = 4
    with pytest.raises(NotImplementedError):
        sp.search("q")
    with pytest.raises(NotImplementedError):
        sp.batch_search(["q"])


# --------------------------------------------------------------------------------------------------------- offsets
def test_hash_tokenizer_offsets_reproduce_the_pieces():
    from tristage_rag_amd.encoders import HashTokenizer, token_offsets
    tok = HashTokenizer()
    text = "Hello, World!  It's 2024 -- naive cafe\tx_y"
    for L in (None, 64, 9, 3, 2):
        ids = tok(text, truncation=True, max_length=L)["input_ids"][0]
        off = tok.offsets(text, L)
        assert len(off) == len(ids)
        assert off[0] == (0, 0) and off[-1] == (0, 0)
        pieces = [text.lower()[a:b] for a, b in off[1:-1]]
        assert pieces == re.findall(r"[a-z0-9]+|[^\sa-z0-9]", text.lower())[: len(pieces)]
        assert list(tok._ids_np("".join(p + " " for p in pieces))) == ids[1:-1]      # the same pieces, hence the same ids
        assert all(b > a for a, b in off[1:-1]) and all(x[1] <= y[0] for x, y in zip(off[1:-2], off[2:-1]))
    assert len(tok.offsets(text, 9)) == 9
    spans, src = token_offsets(tok, text, 64)
    assert src == text                                   # lowering kept the length: cut from the original
    assert src[spans[1][0]: spans[1][1]] == "Hello"
    odd = "İstanbul x"                              # lower() of U+0130 is two characters: cut from the lowered string
    spans, src = token_offsets(tok, odd, 64)
    assert src == odd.lower() and len(src) != len(odd)
    assert [src[a:b] for a, b in spans[1:-1]] == re.findall(r"[a-z0-9]+|[^\sa-z0-9]", odd.lower())

    class NoOffsets:
        pass
    assert token_offsets(NoOffsets(), text, 64) is None
