"""Every stage-1 entry point on reused workspace sets of ONE handle.

A handle hands its eight workspace sets out round robin, so what a call leaves in a set (counts, thresholds, candidate
lists, the one-launch search's keys and arrival counter) is met by the ninth acquisition after it.  Here one index per
storage type lives for the whole module; a **block** is one variant of tests/handle_reuse_cases.py called eight times
in a row, and for every variant A one test runs A, B1, A, B2, ... over all other variants, so that every ordered pair
(A, B) runs back to back and a failing id names the predecessor.

After every call the outputs equal the exact model's (ids and score bits, padding included, the tickets finish()
reports), and the call took the path it takes on a clean handle: the counters of last_search_info() /
last_filter_info() / last_bias_info() / last_range_info() equal those recorded as the first call on a fresh handle of
the same corpus.  The second assertion is what keeps the exact fallback from hiding a stale count.  Then the same with
every third row removed.  Nine host threads on one handle at once: tests/test_threads_on_reused_handle_gpu.py (a module
collected after test_stream_order_gpu.py, whose self check depends on how many torch side streams were taken before)."""
import collections

import numpy as np
import pytest

import handle_reuse_cases as hc

pytestmark = pytest.mark.gpu

STORAGES = ("f16", "bf16", "f32", "fp8", "fp4")
PARTS = 1                 # tests per variant A (split_sequence); every test stays at a few seconds with one
_PLANNED = collections.Counter()   # (storage, phase, predecessor, variant) blocks the tests that started have to run
_RAN = collections.Counter()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


class _State:
    """One storage type: the long-lived handle, the device copies of inputs and expected outputs."""

    def __init__(self, torch, storage, live=None):
        self.torch, self.storage, self.live = torch, storage, live
        self.dat = hc.data(storage)
        dt = {"f16": torch.float16, "bf16": torch.bfloat16}.get(storage, torch.float32)
        self.corpus_dev = torch.tensor(self.dat.corpus).cuda().to(dt)      # (a copy: the shared arrays are read-only)
        self.env = hc.Env(torch, storage, self.dat, live)
        self.idx = self.new_index()
        assert np.array_equal(self.idx.reconstruct_n(), self.dat.corpus)      # stored exactly, before anything else
        self._want = {}
        self.fresh = {}

    def new_index(self):
        from tristage_rag_amd.index import FlatIPIndex
        kw = {"fp8_scale_log2": hc.FP8_SCALE_LOG2} if self.storage == "fp8" else {}
        idx = FlatIPIndex(hc.STORAGE_D[self.storage], dtype=self.storage, **kw)
        idx.add(self.corpus_dev)
        assert idx.ntotal == hc.N
        if self.live is not None:
            assert idx.remove_ids(np.flatnonzero(~self.live)) == int((~self.live).sum())
        return idx

    def want(self, v):
        """The model's outputs of ``v``: on the device for device calls (float zeros canonical), and on the host."""
        if v.name not in self._want:
            torch = self.torch
            w = hc.expected(v, self.dat, live=self.live)
            outs, extra = (w if v.kind == "async" else (w, None))
            outs = tuple(a + np.float32(0.0) if a.dtype == np.float32 else a for a in outs)
            on_host = bool(v.opt.get("host") or v.opt.get("raises"))
            dev = outs if on_host else tuple(torch.tensor(a).cuda() for a in outs)
            self._want[v.name] = (dev, extra)
        return self._want[v.name]

    def close(self):
        self.idx.close()


def _equal(torch, got, want, what):
    """One host round trip: every output equals the model's, float outputs by their bits (with -0 taken as +0)."""
    assert len(got) == len(want), f"{what}: {len(got)} outputs for {len(want)}"
    if isinstance(want[0], np.ndarray):
        for j, (g, w) in enumerate(zip(got, want)):
            g = np.asarray(g)
            assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: output {j} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
            same = np.array_equal((g + np.float32(0.0)).view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 \
                else np.array_equal(g, w)
            assert same, f"{what}: output {j} differs"
        return
    ok = None
    for j, (g, w) in enumerate(zip(got, want)):
        assert tuple(g.shape) == tuple(w.shape) and g.dtype == w.dtype, \
            f"{what}: output {j} is {g.dtype}{tuple(g.shape)}, want {w.dtype}{tuple(w.shape)}"
        e = ((g + 0.0).view(torch.int32) == w.view(torch.int32)).all() if g.is_floating_point() else (g == w).all()
        ok = e if ok is None else ok & e
    if not bool(ok):
        bad = [j for j, (g, w) in enumerate(zip(got, want))
               if not torch.equal((g + 0.0).view(torch.int32) if g.is_floating_point() else g,
                                  w.view(torch.int32) if w.is_floating_point() else w)]
        j = bad[0]
        rows = (got[j] != want[j]).reshape(got[j].shape[0], -1).any(dim=1).nonzero().flatten()[:5].tolist()
        raise AssertionError(f"{what}: outputs {bad} differ from the model (output {j}: first rows {rows})")


def _call(st, v, what):
    got = hc.run(v, st.idx, st.env)
    want, extra = st.want(v)
    if v.kind == "async":
        outs, failed = got
        assert failed == extra, f"{what}: finish() reported submissions {failed}, the model {extra}"
        got = outs
    _equal(st.torch, got, want, what)
    return hc.path_info(v, st.idx)


def _fresh_info(st, v):
    """The counters of ``v`` as the first call on a fresh handle of the same corpus: recorded once, on two handles,
    which must agree (what is compared later has to be reproducible)."""
    if v.name not in st.fresh:
        infos = []
        for _ in range(2):
            main, st.idx = st.idx, st.new_index()
            try:
                infos.append(_call(st, v, f"{st.storage}: {v.name} on a fresh handle"))
            finally:
                st.idx.close()
                st.idx = main
        assert infos[0] == infos[1], f"{st.storage}: {v.name} on two fresh handles: {infos[0]} != {infos[1]}"
        st.fresh[v.name] = infos[0]
    return st.fresh[v.name]


def _block(st, v, pred, phase="pairs"):
    clean = _fresh_info(st, v)
    for rep in range(hc.BLOCK):
        what = f"{st.storage}: {v.name}, call {rep} of the block after {pred}"
        info = _call(st, v, what)
        assert info == clean, f"{what}: took {info}, on a clean handle {clean}"
    _RAN[(st.storage, phase, pred, v.name)] += 1


def _run_sequence(st, seq, phase="pairs"):
    for pred, name in zip([None] + seq[:-1], seq):
        _PLANNED[(st.storage, phase, pred, name)] += 1
    for pred, name in zip([None] + seq[:-1], seq):
        _block(st, hc.BY_NAME[name], pred, phase)


@pytest.fixture(scope="module")
def states(torch_mod):
    """The long-lived handles, one per storage type, built at first use and never recreated."""
    made = {}

    def get(storage):
        if storage not in made:
            made[storage] = _State(torch_mod, storage)
        return made[storage]

    yield get
    for st in made.values():
        st.close()


def _cases():
    return [pytest.param(s, n, p, id=f"{s}-{n}" + (f"-{p}" if PARTS > 1 else ""))
            for s in STORAGES for n in hc.SUPPORTED[s] for p in range(PARTS)]


@pytest.mark.parametrize("storage,a,part", _cases())
def test_every_successor_of(states, storage, a, part):
    """A, B1, A, B2, ... : every variant B behind A and A behind it, one block each, on the long-lived handle."""
    st = states(storage)
    seqs = hc.split_sequence(list(hc.SUPPORTED[storage]), a, PARTS)
    if part < len(seqs):
        _run_sequence(st, seqs[part])


@pytest.mark.parametrize("storage", STORAGES)
def test_every_pair_again_with_every_third_row_removed(states, torch_mod, storage):
    """Every search is now a filtered one through the handle's live bitmap; the reduced table, every ordered pair."""
    st = _State(torch_mod, storage, live=hc.aux("live"))
    try:
        assert st.idx.nlive == int(hc.aux("live").sum())
        names = [v.name for v in hc.variants_of(storage, hc.TOMBSTONE)]
        for a in names:
            _run_sequence(st, hc.sequence(names, a), "tombstones")
    finally:
        st.close()


def test_every_planned_block_ran():
    """No block of a test that started was left out, and where every variant's test of a storage type ran, every
    ordered pair of its variants was back to back."""
    assert _PLANNED, "this test closes the file: run it with the others"
    assert _RAN == _PLANNED, sorted((_PLANNED - _RAN).items(), key=str)[:10]
    for storage in STORAGES:
        names = hc.SUPPORTED[storage]
        firsts = {k[3] for k in _PLANNED if k[0] == storage and k[1] == "pairs" and k[2] is None}
        if firsts == set(names):
            ran = {(k[2], k[3]) for k in _RAN if k[0] == storage and k[1] == "pairs"}
            missing = {(a, b) for a in names for b in names if a != b} - ran
            assert not missing, sorted(missing)[:10]
