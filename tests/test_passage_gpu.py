"""Best passage per hit on the GPU (ts_passage.hip): the kernels EQUAL the float64 model on exactly
summable inputs (tests/passage_model.py) at every size where they take another path, pass the near-tie rule on random
rows, and RetrievalPipeline / ColBERTScorer report spans that are valid for the rows they scored."""
import ctypes

import numpy as np
import pytest

import passage_model as pm

pytestmark = pytest.mark.gpu

STORES = ("f16", "bf16", "f32")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _tdt(torch, store):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[store]


def _pack(torch, docs, store, H):
    """docs (list of [len, H] float arrays) -> (store tensor, starts, lens) on the GPU; 7 unused rows in front"""
    lens = np.array([d.shape[0] for d in docs], np.int64)
    pad = 8                                                     # (rows in front: a start is not an index of the list)
    rows = np.concatenate([np.zeros((pad, H), np.float32)] + [np.asarray(d, np.float32).reshape(-1, H) for d in docs])
    starts = pad + np.cumsum(lens) - lens
    return (torch.from_numpy(rows).cuda().to(_tdt(torch, store)), torch.from_numpy(starts).cuda(),
            torch.from_numpy(lens.astype(np.int32)).cuda())


def _call(torch, q, docs, w, store, align=True):
    from tristage_rag_amd.index import maxsim_passages_indexed
    H = q.shape[1]
    ts, t_s, t_l = _pack(torch, docs, store, H)
    tq = torch.from_numpy(np.array(q, np.float32)).cuda().to(_tdt(torch, store))       # (a copy: the cases are read-only)
    out = maxsim_passages_indexed(tq, ts, t_s, t_l, w, align=align)
    return [o.cpu().numpy() for o in out]


def _rows(out, i):
    return (out[0][i], out[1][i], out[2][i], out[3][i] if len(out) > 3 else None)


def _assert_equal_model(out, models, what):
    for i, m in enumerate(models):
        msg = pm.equal_exact(_rows(out, i), m)
        assert msg is None, f"{what}, candidate {i} (Ld = {m.cos.shape[1]}): {msg}"


# ---------------------------------------------------------------------------------------------------- exact equality
@pytest.fixture(scope="module")
def exact_models():
    """(q, docs, {w: models}) per launch of the table: computed once, shared, never changed"""
    out = {}
    for L in pm.exact_launches():
        q, docs = pm.launch_data(L)
        out[L.name] = (q, docs, {w: pm.passages(q, docs, w) for w in L.windows})
    return out


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("L", pm.exact_launches(), ids=lambda L: L.name)
def test_exact_inputs_equal_the_model(torch_mod, exact_models, L, store):
    q, docs, models = exact_models[L.name]
    for w in L.windows:
        out = _call(torch_mod, q, docs, w, store, align=True)
        _assert_equal_model(out, models[w], f"{L.name} {store} w={w}")
    # without the alignment: the same start, length and score bits
    w = L.windows[len(L.windows) // 2]
    a, b = _call(torch_mod, q, docs, w, store, align=False), _call(torch_mod, q, docs, w, store, align=True)
    assert len(a) == 3
    for x, y in zip(a, b[:3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("store", STORES)
def test_planted_passages_are_found(torch_mod, store):
    for case in pm.planted_cases():
        out = _call(torch_mod, case.q, [case.doc], case.w, store)
        assert int(out[0][0]) == case.want_start and int(out[1][0]) == case.w, case.name
        _assert_equal_model(out, [pm.passage(case.q, case.doc, case.w)], case.name)


@pytest.mark.parametrize("store", STORES)
def test_no_candidate_and_one_candidate(torch_mod, store):
    L = pm.exact_launches()[1]
    q, docs = pm.launch_data(L)
    out = _call(torch_mod, q, [], 4, store)
    assert [o.shape[0] for o in out] == [0, 0, 0, 0] and out[3].shape == (0, L.Lq)
    for d in (docs[3], docs[1], np.zeros((0, L.H), np.float32)):
        _assert_equal_model(_call(torch_mod, q, [d], 4, store), [pm.passage(q, d, 4)], "one candidate")


@pytest.mark.parametrize("store", STORES)
def test_a_window_of_the_whole_document_gives_the_bits_of_maxsim_indexed(torch_mod, exact_models, store):
    from tristage_rag_amd.index import maxsim_indexed
    torch = torch_mod
    for L in pm.exact_launches():
        q, docs, _ = exact_models[L.name]
        ts, t_s, t_l = _pack(torch, docs, store, L.H)
        tq = torch.from_numpy(np.array(q)).cuda().to(_tdt(torch, store))
        want = maxsim_indexed(tq, ts, t_s, t_l).cpu().numpy()
        for w in (max(L.lens), 4096):
            out = _call(torch, q, docs, w, store, align=False)
            live = np.array(L.lens) > 0
            assert np.array_equal(out[0][live], np.zeros(live.sum(), np.int32))
            assert np.array_equal(out[1][live], np.array(L.lens, np.int32)[live])
            assert np.array_equal(out[2][live].view(np.uint32), want[live].view(np.uint32)), (L.name, w)
            assert (out[2][~live] == -pm.FLT_MAX).all() and (want[~live] == 0.0).all()


# ------------------------------------------------------------------------------------------------------- batch form
@pytest.mark.parametrize("nq", (1, 2, 33))
def test_batch_form_equals_per_query_calls(torch_mod, nq):
    from tristage_rag_amd import _lib
    from tristage_rag_amd.index import maxsim_passages_indexed, maxsim_passages_indexed_batch
    torch = torch_mod
    L = pm.Launch("batch", 64, 65, (33, 0, 192, 1, 64, 31, 2, 65, 32, 63, 200), (7,), 300)
    q, docs = pm.launch_data(L)
    ts, t_s, t_l = _pack(torch, docs, "bf16", L.H)
    tq = torch.from_numpy(q).cuda().bfloat16()
    rng = np.random.default_rng(nq)
    spans = [(0, 65)] + [tuple(sorted(rng.choice(66, 2, replace=False))) for _ in range(nq - 1)]     # ragged Lq
    picks = [rng.permutation(len(docs))[: int(rng.integers(0 if j else 3, 8))] for j in range(nq)]
    q_off = np.concatenate([[0], np.cumsum([b - a for a, b in spans])])
    c_off = np.concatenate([[0], np.cumsum([len(p) for p in picks])])
    pk = torch.from_numpy(np.concatenate(picks).astype(np.int64)).cuda()
    qp = torch.cat([tq[a:b] for a, b in spans])
    got = maxsim_passages_indexed_batch(qp, q_off, ts, t_s[pk], t_l[pk], c_off, 7, align=True)
    max_lq = max(b - a for a, b in spans)
    assert got[3].shape == (int(c_off[-1]), max_lq)
    for j, ((a, b), p) in enumerate(zip(spans, picks)):
        sl = slice(int(c_off[j]), int(c_off[j + 1]))
        pj = torch.from_numpy(p.astype(np.int64)).cuda()
        one = maxsim_passages_indexed(tq[a:b], ts, t_s[pj], t_l[pj], 7, align=True)
        for x, y in zip(got[:3], one[:3]):
            assert torch.equal(x[sl].view(torch.int32), y.view(torch.int32)), f"query {j}"
        assert torch.equal(got[3][sl, : b - a], one[3])
        assert (got[3][sl, b - a:] == -1).all()                                   # -1 beyond each Lq_j
        _assert_equal_model([o.cpu().numpy() for o in one], pm.passages(q[a:b], [docs[i] for i in p], 7), f"query {j}")
    no_align = maxsim_passages_indexed_batch(qp, q_off, ts, t_s[pk], t_l[pk], c_off, 7)
    for x, y in zip(no_align, got[:3]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # align_ld > max Lq through the C entry point: the same rows, -1 in the extra columns
    lib = _lib.load()
    n, ld = int(c_off[-1]), max_lq + 3
    o1, o2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    o3 = torch.empty(n, dtype=torch.float32, device="cuda")
    al = torch.full((n, ld), 7777, dtype=torch.int32, device="cuda")
    qo, co = np.ascontiguousarray(q_off, np.int32), np.ascontiguousarray(c_off, np.int32)
    s_sel, l_sel = t_s[pk].contiguous(), t_l[pk].contiguous()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.ts_maxsim_passages_indexed_batch(P(qp), qo.ctypes.data_as(ctypes.c_void_p), nq, P(ts), P(s_sel), P(l_sel),
                                                    co.ctypes.data_as(ctypes.c_void_p), L.H, _lib.TS_BF16, 7, P(o1), P(o2),
                                                    P(o3), P(al), ld, 0,
                                                    ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))))
    torch.cuda.synchronize()
    assert torch.equal(o1, got[0]) and torch.equal(o2, got[1]) and torch.equal(o3.view(torch.int32), got[2].view(torch.int32))
    assert torch.equal(al[:, :max_lq], got[3]) and (al[:, max_lq:] == -1).all()


def test_long_documents_among_more_pairs_than_long_workgroups(torch_mod):
    """1100 pairs of one call: the long-document kernel has 1024 workgroups, workgroup b owns pairs b and b + 1024, so
    the long documents at positions >= 1024 are second pairs of their workgroups; a call of 40 pairs beside it."""
    from tristage_rag_amd.index import maxsim_passages_indexed
    torch = torch_mod
    L = pm.Launch("many", 64, 33, (200, 64, 0, 1024, 31, 193), (9,), 301)
    q, docs = pm.launch_data(L)
    models = pm.passages(q, docs, 9)
    ts, t_s, t_l = _pack(torch, docs, "bf16", L.H)
    tq = torch.from_numpy(q).cuda().bfloat16()
    for n in (40, 1100):
        pick = np.arange(n) % len(docs)
        pk = torch.from_numpy(pick).cuda()
        out = [o.cpu().numpy() for o in maxsim_passages_indexed(tq, ts, t_s[pk], t_l[pk], 9, align=True)]
        _assert_equal_model(out, [models[i] for i in pick], f"{n} pairs")


def test_two_runs_give_the_same_bits_on_any_stream(torch_mod):
    from tristage_rag_amd.index import maxsim_passages_indexed
    torch = torch_mod
    rng = np.random.default_rng(11)
    docs = [rng.standard_normal((n, 128)).astype(np.float32) for n in (150, 64, 33, 300)]
    ts, t_s, t_l = _pack(torch, docs, "bf16", 128)
    tq = torch.from_numpy(rng.standard_normal((40, 128)).astype(np.float32)).cuda().bfloat16()
    first = maxsim_passages_indexed(tq, ts, t_s, t_l, 16, align=True)
    again = maxsim_passages_indexed(tq, ts, t_s, t_l, 16, align=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = maxsim_passages_indexed(tq, ts, t_s, t_l, 16, align=True)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
        assert a.is_cuda


# -------------------------------------------------------------------------------------------------------- random rows
@pytest.mark.parametrize("store", STORES)
def test_random_unit_norm_rows_pass_the_near_tie_rule(torch_mod, store):
    torch = torch_mod
    rng = np.random.default_rng(21)
    H = 768
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    tdt = _tdt(torch, store)
    rnd = lambda x: torch.from_numpy(x.astype(np.float32)).to(tdt).to(torch.float64).numpy()     # the values stored
    # Lq = 32: the workload's query; Lq = 256: the longest query taken (8 rounds, 16 for the document of 300 rows)
    for Lq, lens, w in ((32, [64, 192, 100, 65, 128, 191, 77, 160], 32), (32, None, 8), (256, [64, 192, 300], 32)):
        if lens is not None:
            q = rnd(unit(rng.standard_normal((Lq, H))))
            docs = [rnd(unit(rng.standard_normal((n, H)))) for n in lens]
        out = _call(torch, q, docs, w, store)
        for i, d in enumerate(docs):
            m = pm.passage(q, d, w)
            got = _rows(out, i)
            print(f"{store} Lq={Lq} w={w} cand {i}: start {int(got[0])} model {m.start}, score err "
                  f"{abs(float(got[2]) - m.window_scores[int(got[0])] / Lq):.3e}, "
                  f"gap to best {m.window_scores.max() - m.window_scores[int(got[0])]:.3e}")
            assert pm.passage_valid(got, m, pm.tol_of(store)), (store, Lq, w, i)


# ------------------------------------------------------------------------------------------- scorer and the pipeline
WORDS = ("neural network attention transformer language retrieval index vector query document "
         "learning model data system search rank score token embedding gpu memory").split()
QUERIES = ["marginal relevance picks results", "gpu memory index", "language retrieval system"]
N_DOCS = 120


def _docs(n=N_DOCS):
    rng = np.random.default_rng(3)
    docs = [" ".join(rng.choice(WORDS, size=int(rng.integers(4, 30)))) for _ in range(n)]
    docs[5] = "GPU Memory, index!  And a Longer tail: of other words."          # punctuation and capitals
    docs[9] = "   "                                                             # blank: stage 2 encodes "empty"
    meta = [{"source": f"s{i // 3}", "i": i} for i in range(n)]
    return docs, meta


def _pipeline(tmp_path, name, **extra):
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig, RetrievalPipeline
    pc = PipelineConfig(stage1_model="random:tiny", stage2_model="random:tiny", stage3_model="random:tiny",
                        device="cuda", cache_dir=str(tmp_path / "m"), index_dir=str(tmp_path / "i"),
                        log_file=str(tmp_path / f"{name}.log"), stage1_top_k=40, stage2_top_k=30, stage3_top_k=20,
                        stage1_use_fp16=False, stage2_use_fp16=False, stage3_use_fp16=False,
                        stage1_enable_bm25=False, save_intermediate_results=True, **extra)
    p = RetrievalPipeline(config=pc)
    p.initialize_stages()
    p.add_documents(*_docs())
    return p


def _f64(t):
    return t.detach().to("cpu").double().numpy()


def test_best_passages_with_and_without_a_token_store(torch_mod, tmp_path):
    arr = _pipeline(tmp_path, "arr", stage2_precompute_document_embeddings=True, stage3_cache_document_tokens=True)
    sc = arr.stage2
    docs, _ = _docs()
    ids = [5, 17, 3, 64, 9]
    query = QUERIES[1]
    qrows = _f64(sc.encode_queries_batch([query])[0])
    from_store = sc.best_passages(query, ids, 6, align=True)
    by_text = sc.best_passages(query, [docs[i] for i in ids], 6, align=True)
    store = sc.token_store
    rows_store = [_f64(store.data[store.starts[sc._store_slot[i]]: store.starts[sc._store_slot[i]] + store.lens[sc._store_slot[i]]])
                  for i in ids]
    rows_text = [_f64(e) for e in sc.encode_documents_batch([docs[i] for i in ids])]
    for got, rows in ((from_store, rows_store), (by_text, rows_text)):
        assert len(got) == len(ids)
        for g, d in zip(got, rows):
            m = pm.passage(qrows, d, 6)
            assert pm.passage_valid((g["token_start"], g["token_end"] - g["token_start"], g["score"], np.array(g["align"])),
                                    m, pm.TOL_F32)
    many = sc.best_passages([query, QUERIES[0]], [ids, ids[:2]], 6)
    q2 = [_f64(e) for e in sc.encode_queries_batch([query, QUERIES[0]])]          # the rows of the two-query forward
    assert [len(x) for x in many] == [len(ids), 2]
    for qr, lst, rows in zip(q2, many, (rows_store, rows_store[:2])):
        for g, d in zip(lst, rows):
            assert "align" not in g
            assert pm.passage_valid((g["token_start"], g["token_end"] - g["token_start"], g["score"], None),
                                    pm.passage(qr, d, 6), pm.TOL_F32)
    with pytest.raises(ValueError):
        sc.best_passages(query, [10 ** 6], 6)                     # no slot
    with pytest.raises(ValueError):
        sc.best_passages(query, ids, 0)
    with pytest.raises(ValueError):
        sc.best_passages(query, ids)                              # no window anywhere
    sc.config.passage_window = 6                                  # Stage2Config's value is the default window
    assert sc.best_passages(query, ids) == sc.best_passages(query, ids, 6)


def _check_records(p, res, window, rows, qrows):
    """every record's span is valid against the model on the rows stage 2 scored for it (`rows`, one per record), and
    its text is the substring from the first to the last non-special piece of the span"""
    import re
    sc = p.stage2
    assert res["results"] and len(rows) == len(res["results"])
    for r, d in zip(res["results"], rows):
        psg = r["passage"]
        assert set(psg) == {"token_start", "token_end", "score", "char_start", "char_end", "text"}
        m = pm.passage(qrows, d, window)
        assert pm.passage_valid((psg["token_start"], psg["token_end"] - psg["token_start"], psg["score"], None), m, pm.TOL_F32)
        doc = r["document"]
        if not doc.strip():
            assert psg["text"] == "" and (psg["char_start"], psg["char_end"]) == (0, 0)
            continue
        spans = [(0, 0)] + [x.span() for x in re.finditer(r"[a-z0-9]+|[^\sa-z0-9]", doc.lower())][: sc.config.max_seq_length - 2] + [(0, 0)]
        assert len(spans) == d.shape[0]
        real = [s for s in spans[psg["token_start"]: psg["token_end"]] if s != (0, 0)]
        want = doc[real[0][0]: real[-1][1]] if real else ""
        assert psg["text"] == want and (not real or (psg["char_start"], psg["char_end"]) == (real[0][0], real[-1][1]))


def _strip(res):
    return [{k: v for k, v in r.items() if k != "passage"} for r in res["results"]]


def _scored_rows(p, group):
    """The token rows the post-step scored for the records of `group` (the outputs of ONE call), per output: the
    rows of the token store where every document has a slot, else the texts of the whole call re-encoded together;
    and the query rows of the call's one query forward."""
    sc = p.stage2
    st = sc.token_store
    flat = [r for o in group for r in o["results"]]
    if len(st) and all(r["doc_id"] in sc._store_slot for r in flat):
        rows = [_f64(st.data[st.starts[s]: st.starts[s] + st.lens[s]]) for s in (sc._store_slot[r["doc_id"]] for r in flat)]
    else:
        rows = [_f64(e) for e in sc.encode_documents_batch([r["document"] for r in flat])]
    out, at = [], 0
    for o in group:
        out.append(rows[at: at + len(o["results"])])
        at += len(o["results"])
    return out, [_f64(e) for e in sc.encode_queries_batch([o["query"] for o in group])]


def test_pipeline_reports_passages_on_both_paths(torch_mod, tmp_path):
    rec = _pipeline(tmp_path, "rec")
    arr = _pipeline(tmp_path, "arr", stage2_precompute_document_embeddings=True, stage3_cache_document_tokens=True)
    assert arr._arrays_ready() and not rec._arrays_ready()
    W = 8
    for name, p in (("rec", rec), ("arr", arr)):
        plain = [p.search(q) for q in QUERIES]
        plain_many = p.search_many(QUERIES)
        assert all("passage" not in r for o in plain + plain_many for r in o["results"])   # unset: no record has the key
        calls = [("search", [p.search(q, passages=W)], [b]) for q, b in zip(QUERIES, plain)]
        calls.append(("batch_search", p.batch_search(QUERIES, passages=W), plain))
        calls.append(("search_many", p.search_many(QUERIES, passages=W), plain_many))
        for how, group, base in calls:
            for res, b, rows, qrows in zip(group, base, *_scored_rows(p, group)):
                assert _strip(res) == b["results"], (name, how)                             # rankings and scores identical
                _check_records(p, res, W, rows, qrows)
        # together with MMR and with grouping: the same lists as without passages, every record with a span
        for kw in ({"mmr_lambda": 0.5}, {"group_by": "source", "group_size": 1}):
            a, b = p.search(QUERIES[1], passages=W, **kw), p.search(QUERIES[1], **kw)
            assert _strip(a) == b["results"] and a["results"]
            m = p.search_many(QUERIES, passages=W, **kw)
            for group in ([a], m):
                for res, rows, qrows in zip(group, *_scored_rows(p, group)):
                    _check_records(p, res, W, rows, qrows)
        # a blank document (stage 2 encodes "empty") and one with capitals and punctuation, through the post-step
        docs, _ = _docs()
        outs = [{"query": QUERIES[1], "results": [{"doc_id": i, "document": docs[i]} for i in (9, 5)]}]
        p._add_passages(outs, 4)
        (rows,), (qrows,) = _scored_rows(p, outs)
        _check_records(p, outs[0], 4, rows, qrows)
        blank, mixed = (r["passage"] for r in outs[0]["results"])
        assert blank["text"] == "" and (blank["token_start"], blank["token_end"]) == (0, 3)     # [CLS] empty [SEP]
        assert mixed["text"] and mixed["text"] in docs[5]                                       # cut from the original text
    cfg = _pipeline(tmp_path, "cfg", passage_window=W, stage2_precompute_document_embeddings=True)    # the config's value
    got = cfg.search(QUERIES[0])
    assert got["results"] and all(0 < r["passage"]["token_end"] - r["passage"]["token_start"] <= W for r in got["results"])


def test_sharded_pipeline_refuses(tmp_path):
    from tristage_rag_amd.parallel_pipeline import ShardedRetrievalPipeline
    from tristage_rag_amd.retrieval_pipeline import PipelineConfig
    sp = ShardedRetrievalPipeline(config=PipelineConfig(log_file=str(tmp_path / "s.log")))
    with pytest.raises(NotImplementedError):
        sp.search("q", passages=8)
    with pytest.raises(NotImplementedError):
        sp.search_many(["q"], passages=8)
    with pytest.raises(NotImplementedError):
        sp.batch_search(["q"], passages=8)


def test_refusals_before_any_launch(torch_mod):
    from tristage_rag_amd.index import maxsim_passages_indexed, quantize_rows_fp8
    torch = torch_mod
    q = torch.zeros((4, 64), dtype=torch.bfloat16, device="cuda")
    store = torch.zeros((2048, 64), dtype=torch.bfloat16, device="cuda")
    starts = torch.tensor([0, 5], device="cuda")
    lens = torch.tensor([5, 5], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        maxsim_passages_indexed(q, store, starts, lens, 0)
    with pytest.raises(ValueError, match="1024"):
        maxsim_passages_indexed(q, store, starts, torch.tensor([5, 1025], dtype=torch.int32, device="cuda"), 8)
    with pytest.raises(ValueError, match="256"):
        maxsim_passages_indexed(torch.zeros((257, 64), dtype=torch.bfloat16, device="cuda"), store, starts, lens, 8)
    with pytest.raises(NotImplementedError):
        maxsim_passages_indexed(q, quantize_rows_fp8(store), starts, lens, 8)
    with pytest.raises(ValueError, match="16 bytes"):
        maxsim_passages_indexed(q[:, :60].contiguous(), store[:, :60].contiguous(), starts, lens, 8)


def test_c_entry_point_marks_a_candidate_of_more_than_1024_rows(torch_mod):
    """The lengths live on the device and the call does not synchronise: TS_OK, and that candidate gets start -2,
    length 0, score -FLT_MAX, alignment -1 (an empty one: start -1); its neighbours are scored."""
    from tristage_rag_amd import _lib
    torch = torch_mod
    lib = _lib.load()
    rng = np.random.default_rng(4)
    store = torch.from_numpy(rng.standard_normal((2048, 64)).astype(np.float32)).cuda().bfloat16()
    q = torch.from_numpy(rng.standard_normal((4, 64)).astype(np.float32)).cuda().bfloat16()
    starts = torch.tensor([0, 0, 7, 100], dtype=torch.int64, device="cuda")
    lens = torch.tensor([5, 1025, 0, 300], dtype=torch.int32, device="cuda")
    o1, o2 = (torch.full((4,), 99, dtype=torch.int32, device="cuda") for _ in range(2))
    o3 = torch.zeros(4, dtype=torch.float32, device="cuda")
    al = torch.full((4, 4), 99, dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.ts_maxsim_passages_indexed(P(q), 4, P(store), P(starts), P(lens), 4, 64, _lib.TS_BF16, 3, P(o1), P(o2),
                                              P(o3), P(al), 0, ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))))
    torch.cuda.synchronize()
    assert o1.tolist()[1:3] == [-2, -1] and o2.tolist() == [3, 0, 0, 3]
    assert o3.tolist()[1:3] == [-pm.FLT_MAX, -pm.FLT_MAX] and (al[1:3] == -1).all()
    assert 0 <= o1[0] <= 2 and 0 <= o1[3] <= 297 and (al[0] >= o1[0]).all() and (al[3] < o1[3] + 3).all()
