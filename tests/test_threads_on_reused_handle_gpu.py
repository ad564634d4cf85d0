"""The concurrent phase of the handle-reuse tests (tests/test_handle_reuse_gpu.py): nine host threads,
each on a stream of its own, on ONE handle whose eight workspace sets have all been used before.

A module of its own, named so that it is collected after test_stream_order_gpu.py: it takes 45 torch side streams, and
that module's self check depends on the place its own side stream gets in torch's stream pool (see
test_stream_order_of_funnel_gpu.py)."""
import threading

import pytest

import handle_reuse_cases as hc
import test_handle_reuse_gpu as hr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("storage", hr.STORAGES)
def test_nine_threads_on_one_handle(torch_mod, storage):
    """Each thread repeats one entry point ten times against the model: five-launch, one-launch, filtered and boosted
    searches, range search, prefix search, rescore, scores and a host-pointer search.  Boosted, range and rescore calls
    are serialised inside the handle (bias_mu, range_mu, rescore_mu), host-pointer calls too; that is the library's
    job, so all of them run here.  No thread submits asynchronously: the header allows one such thread, but
    FlatIPIndex.range_search finishes pending searches first, which only their submitter may do."""
    torch = torch_mod
    st = hr._State(torch, storage)
    try:
        warm = [n for n in ("one_tie_8x100", "classic_64x100", "one_64x100") if n in hc.SUPPORTED[storage]]
        hr._run_sequence(st, warm, "before-threads")          # every set has had a user, one of them a failed pass
        vs = hc.variants_of(storage, hc.CONCURRENT)
        jobs = [vs[t % len(vs)] for t in range(9)]
        for v in vs:
            st.want(v)
            if v.kind == "range":
                st.env.radius(v)
        torch.cuda.synchronize()
        errors = []

        def worker(t):
            v = jobs[t]
            try:
                with torch.cuda.stream(torch.cuda.Stream()):
                    for rep in range(10):
                        got = hc.run(v, st.idx, st.env)
                        hr._equal(torch, got, st.want(v)[0], f"{storage}: thread {t} ({v.name}), repetition {rep}")
            except Exception as e:  # noqa: BLE001
                errors.append((t, v.name, repr(e)))

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(9)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        torch.cuda.synchronize()
        assert not errors, errors
        # the handle serves the next callers on every set as a clean one would
        hr._run_sequence(st, warm[-2:] * 2, "after-threads")
    finally:
        st.close()
