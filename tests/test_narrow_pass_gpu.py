"""Every stage-1 entry point where a pass holds only 32 queries.

Above d = 1024 (f16 / bf16 / fp8 / fp4 storage) and d = 512 (fp32) the host cuts a call into passes of 32 queries, not
64: query 32 starts a new pass, a new workspace set and a new slice of the masks, radii, limits, outputs and counters.
One index per (storage, d, rows) of tests/narrow_pass_cases.py is alive at a time (its steps are consecutive); every
variant of that file runs on it twice (the second call lands in another workspace set) and both results equal the exact model's: ids and
score bits, padding included.  Each index first proves that it is in the regime at all: the pass counters of a
filtered, a boosted and a range call report ceil(B / 32) passes where the d = 1024 control reports ceil(B / 64).

``ts_index_rescore`` cuts a pass into chunks of queries when its scratch cap binds; the cases here are the first in
which it does (narrow_pass_cases.rescore_chunk), so the first that launch the rescore kernel at a column other than 0."""
import numpy as np
import pytest

import exact_inputs as ex
import funnel_model as fu
import mutation_model as mm
import narrow_pass_cases as nc
import range_model as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dtype(torch, storage):
    return {"f16": torch.float16, "bf16": torch.bfloat16}.get(storage, torch.float32)


class _State:
    """One index: the handle, the device copies of its inputs, the model's outputs."""

    def __init__(self, torch, ix, live=None, corpus_dev=None):
        self.torch, self.ix, self.live = torch, ix, live
        self.dat = nc.data(ix, _cus(torch))
        if corpus_dev is None:
            corpus_dev = torch.tensor(self.dat.corpus).cuda().to(_dtype(torch, ix.storage))
        self.corpus_dev = corpus_dev
        self.env = nc.Env(torch, ix.storage, self.dat, live)
        from tristage_rag_amd.index import FlatIPIndex
        kw = {"fp8_scale_log2": 0} if ix.storage == "fp8" else {}
        self.idx = FlatIPIndex(ix.d, dtype=ix.storage, **kw)
        self.idx.add(corpus_dev)
        assert self.idx.ntotal == self.dat.n
        if live is None:
            assert np.array_equal(self.idx.reconstruct_n(), self.dat.corpus)      # stored exactly, before anything else
        else:
            assert self.idx.remove_ids(np.flatnonzero(~live)) == int((~live).sum())
        self.qp = nc.queries_per_pass(ix.storage, ix.d)
        self.nblk = -(-self.dat.n // 32)

    def close(self):
        self.idx.close()


@pytest.fixture(scope="module")
def st(request, torch_mod):
    """The index of the steps that follow: built at its first step, closed after its last (the steps of one index are
    consecutive, so one index, its corpus and its score matrix are alive at a time)."""
    state = _State(torch_mod, request.param)
    yield state
    state.close()


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _equal(got, want, what):
    """Every output equals the model's: shapes, types, ids, and float outputs by their bits (-0 taken as +0)."""
    assert len(got) == len(want), f"{what}: {len(got)} outputs for {len(want)}"
    for j, (g, w) in enumerate(zip(got, want)):
        g = _host(g)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: output {j} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        if g.dtype == np.float32:
            g, w = (g + np.float32(0.0)).view(np.uint32), (w + np.float32(0.0)).view(np.uint32)
        if not np.array_equal(g, w):
            rows = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[:6].tolist() if g.ndim > 1 else \
                np.flatnonzero(g != w)[:6].tolist()
            raise AssertionError(f"{what}: output {j} differs from the model, first at rows {rows}")


def _check(st, v, live=None, reps=2):
    want = nc.expected(v, st.dat, live=live)
    for rep in range(reps):
        what = f"{st.ix.id}: {v.name}, call {rep}"
        got = nc.run(v, st.idx, st.env)
        if v.kind == "async":
            outs, failed = got
            assert failed == want[1], f"{what}: finish() reported submissions {failed}, the model {want[1]}"
            _equal(outs, want[0], what)
        else:
            _equal(got, want, what)
        _path(st, v, what)


def _path(st, v, what):
    """The call took the path its name says."""
    o = v.opt
    if v.kind == "search" and "path" in o:
        info = st.idx.last_search_info()
        # (fp32 storage with removed rows: every pass is a masked one, and a masked fp32 pass is a dense one)
        path = "dense" if st.ix.storage == "f32" and st.live is not None else o["path"]
        assert info["path"] == path, f"{what}: {info}"
        if o.get("one"):
            assert info["one_launch"], f"{what}: {info}"
    if v.kind == "funnel":
        info = st.idx.last_funnel_info()
        path = o.get("prefix_path", "dense" if st.ix.rows == "dense" else "filter")
        assert info["prefix_path"] == path and info["dims"] == o["dims"], f"{what}: {info}"
    if v.kind == "biased":
        assert st.idx.last_bias_info()["passes"] == -(-len(v.qi) // st.qp), what
    if v.kind == "range":
        info = st.idx.last_range_info()
        assert info["passes"] == -(-len(v.qi) // st.qp), f"{what}: {info}"
        if "all_at" in o and st.ix.rows != "dense" and st.live is None and "allowed" not in o \
                and st.ix.storage != "f32":
            assert info["dense_redo"] == 1, f"{what}: {info}"      # only the pass of the query that takes every row


# ------------------------------------------------------------------------------------------------------ regime proof
def _regime(st, qp):
    """The pass counters of a filtered, a boosted and a range call, each with a masked query in every pass."""
    idx, env, ix = st.idx, st.env, st.ix
    for B in (64, 65):
        passes = -(-B // qp)
        qi = tuple(range(B))
        q = env.q(qi)
        want = nc._topk(st.dat.S[list(qi)], 10, None, nc.aux("m30", st.dat.n))
        _equal(idx.search(q, 10, allowed=env.masks["m30"]), want, f"{ix.id}: filtered, B={B}")
        f = idx.last_filter_info()
        assert f["filter_passes"] + f["dense_passes"] == passes, f"{ix.id} B={B}: {f}"
        assert f["total_blocks"] == passes * st.nblk, f"{ix.id} B={B}: {f}"
        if ix.storage in ("f16", "bf16"):
            idx.search_biased(q, 10, env.bias, allowed=env.masks["m30"])
            assert idx.last_bias_info()["passes"] == passes, f"{ix.id} B={B}: {idx.last_bias_info()}"
        if ix.storage in ("f16", "bf16", "f32"):
            rad = rm.rank_radius(st.dat.S[list(qi)].T, np.eye(B), 5, allowed=nc.aux("m30", st.dat.n))
            lims = idx.range_search(q, rad, allowed=env.masks["m30"])[0]
            assert (np.diff(_host(lims)) >= 5).all()
            assert idx.last_range_info()["passes"] == passes, f"{ix.id} B={B}: {idx.last_range_info()}"


def test_the_control_at_d_1024_reports_64_query_passes(torch_mod):
    st = _State(torch_mod, nc.CONTROL)
    try:
        _regime(st, 64)
    finally:
        st.close()


# ------------------------------------------------------------------------------------------------- the steps of an index
def _refused(st):
    """What the storage type refuses raises as before, and the handle stays usable."""
    for v in nc.refused(st.ix):
        with pytest.raises(NotImplementedError):
            nc.run(v, st.idx, st.env)
    st.idx.search(st.env.q((0, 1)), 3)


def _removed(st, torch):
    """Tombstones: every pass of every entry point is a masked one through the live bitmap."""
    live = nc.aux("live", st.dat.n)
    rm_st = _State(torch, st.ix, live=live, corpus_dev=st.corpus_dev)
    try:
        assert rm_st.idx.nlive == int(live.sum())
        ran = 0
        for v in nc.supported(st.ix):
            if v.name in nc.TOMBSTONE:
                _check(rm_st, v, live=live, reps=1)
                ran += 1
        assert ran >= 3
    finally:
        rm_st.close()


def _steps():
    """Per index, consecutively: the regime proof, every variant, the refusals, the tombstones."""
    out = []
    for ix in nc.INDEXES:
        names = ["regime"] + [v.name for v in nc.supported(ix)] + (["refused"] if nc.refused(ix) else []) + ["removed"]
        out += [pytest.param(ix, n, id=f"{ix.id}-{n}") for n in names]
    return out


@pytest.mark.parametrize("st,step", _steps(), indirect=["st"])
def test_index_step(st, torch_mod, step):
    """``regime``: the library's own pass counters report 32-query passes (the Python mirror only chose the shapes).
    A variant's name: two calls on the handle, each equal to the model, on the path the variant names.  ``refused``,
    ``removed``: see above."""
    if step == "regime":
        _regime(st, 32)
    elif step == "refused":
        _refused(st)
    elif step == "removed":
        _removed(st, torch_mod)
    else:
        _check(st, {v.name: v for v in nc.supported(st.ix)}[step])


# ----------------------------------------------------------------------------------------------------- rescore chunks
@pytest.mark.parametrize("storage,d,B,C", nc.RESCORE_CHUNKED)
def test_rescore_in_chunks_of_queries(torch_mod, storage, d, B, C):
    """The scratch cap binds: chunks after the first launch the rescore kernel at col0 > 0, and at d = 768 one chunk
    reads both halves of the 64-query image.  Removed rows and an id offset, k = C and k < C, each call twice."""
    torch = torch_mod
    from tristage_rag_amd.index import FlatIPIndex
    qc, qp = nc.rescore_chunk(storage, d, B, C)
    assert qc < min(B, qp)
    dat = nc.rescore_data(d)
    n, off = nc.RESCORE_N, nc.RESCORE_OFFSET
    live = nc.aux("live", n)
    idx = FlatIPIndex(d, dtype=storage)
    try:
        dt = _dtype(torch, storage)
        idx.add(torch.tensor(dat.corpus).cuda().to(dt))
        idx.set_id_offset(off)
        assert idx.remove_ids(np.flatnonzero(~live) + off) == int((~live).sum())
        ids = nc.rescore_candidates(B, C, n, live, C + d)
        ids = np.where(ids >= 0, ids + off, ids)
        q = torch.tensor(dat.queries[:B]).cuda().to(dt)
        S = dat.S[:B].astype(np.float32)
        ids_dev = torch.from_numpy(ids).cuda()
        for k in (C, C // 3):
            want = fu.rescore_model(S, ids, k, live=live, id_offset=off)
            assert (want[1][:, 0] >= 0).all() and (k < C or (want[1][:, -1] == -1).all())
            for rep in range(2):
                _equal(idx.rescore(q, ids_dev, k), want, f"{storage} d={d} B={B} C={C} k={k}, call {rep}")
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------------------- IVF
def _ivf_check(ivf, S, lists, tq, B, passes, what):
    """nprobe 1, 3, 8 against the model restricted to the rows of the probed lists; 8 also against the flat model."""
    for p in nc.IVF_NPROBE:
        P = ivf.probe(tq, p)[1].cpu().numpy()
        allowed = [np.isin(lists, P[i]) for i in range(B)]
        want = ex.expected_topk(S.T, np.eye(B), 100, allowed=allowed)
        for rep in range(2):
            _equal(ivf.search(tq, 100, nprobe=p), want, f"{what} nprobe={p}, call {rep}")
            info = ivf.last_search_info()
            assert info["passes"] == passes, f"{what} nprobe={p}: {info}"
    _equal(ivf.search(tq, 100, nprobe=nc.NLIST), ex.expected_topk(S.T, np.eye(B), 100), f"{what} every list")


def test_ivf_refuses_wider_rows_as_before():
    """The quantizer is an fp32 index: above d = 1088 its 32-query image does not fit the LDS."""
    from tristage_rag_amd._lib import TriStageNativeError
    from tristage_rag_amd.index import IVFFlatIndex
    with pytest.raises(TriStageNativeError, match="LDS"):
        IVFFlatIndex(nc.IVF_REFUSED_D, nc.NLIST, dtype="f16")


@pytest.mark.parametrize("n", nc.IVF_N)
@pytest.mark.parametrize("storage,d", nc.IVF_CASES)
def test_ivf_in_32_query_passes(torch_mod, storage, d, n):
    torch = torch_mod
    from tristage_rag_amd.index import IVFFlatIndex
    dat = nc._data("ints", d, n)
    B = 65
    S = dat.S[:B]
    dt = _dtype(torch, storage)
    ivf = IVFFlatIndex(d, nc.NLIST, dtype=storage, nprobe=nc.NLIST)
    try:
        c = mm.rows_for(nc.NLIST, d, seed=777).astype(np.float64)
        ivf.set_centroids((c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32))
        ivf.add(torch.tensor(dat.corpus).cuda().to(dt))
        assert ivf.ntotal == n
        tq = torch.tensor(dat.queries[:B]).cuda().to(dt)
        lists = ivf.probe(torch.from_numpy(ivf.reconstruct_n()).cuda(), 1)[1][:, 0].cpu().numpy()
        assert np.array_equal(np.bincount(lists, minlength=nc.NLIST), ivf.list_sizes())
        _ivf_check(ivf, S, lists, tq, B, 3, f"ivf {storage} d={d} n={n}")
        live = nc.aux("live", n)
        assert ivf.remove_ids(np.flatnonzero(~live)) == int((~live).sum())
        new = ivf.compact()
        assert np.array_equal(new[live], np.arange(int(live.sum()))) and (new[~live] == -1).all()
        _ivf_check(ivf, S[:, live], lists[live], tq, B, 3, f"ivf {storage} d={d} n={n} compacted")
    finally:
        ivf.close()
