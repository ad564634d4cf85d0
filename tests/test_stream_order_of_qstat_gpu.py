"""The coalesced queue with query-stationary passes forced on, held to its stream contract on a side stream with the
harness of tests/stream_order.py as it is.

A module of its own, named so that it is collected after test_stream_order_gpu.py, for the reason
test_stream_order_of_funnel_gpu.py gives: the harness takes side streams from torch's pool, and streams taken before
that module's self check would move its side stream onto the null stream's hardware queue."""
import pytest

import stream_order as so
from helpers import check_topk, make_corpus
from qstat_helpers import corpus_of as _corpus, index_of as _index, scan_launches, tq as _tq

pytestmark = pytest.mark.gpu


def test_stream_contract_of_the_forced_path():
    """The queries are written late on a non-blocking side stream, the held passes are flushed, a consumer reads the
    outputs in stream order."""
    import torch
    assert torch.cuda.is_available()
    d, n, K = 640, 40_960, 10
    h = so.Harness(torch)
    corpus = _corpus(n, d, "f16", seed=11)
    idx = _index(torch, d, "f16", corpus=corpus)
    real = {"q": _tq(torch, make_corpus(128, d, seed=1, dtype="f16"), "f16").contiguous()}
    decoy = {"q": _tq(torch, make_corpus(128, d, seed=2, dtype="f16"), "f16").contiguous()}

    def call(st, b):
        idx.coalesce = True
        D = torch.full((128, K), so.SENT_F, dtype=torch.float32, device="cuda")
        I = torch.full((128, K), so.SENT_I, dtype=torch.int64, device="cuda")
        for i in range(0, 128, 32):   # four batches of 32: a stationary pass of 4 groups at the flush
            idx.search(b["q"][i:i + 32], K, async_=True, out=(D[i:i + 32], I[i:i + 32]))
        idx.flush()
        return D, I

    def anchor(r, outs):
        check_topk(outs[0].cpu().numpy(), outs[1].cpu().numpy(), corpus, r["q"].float().cpu().numpy(), K)
    case = so.Case("queue_stationary", lambda: (real, decoy), call, after=lambda st, o: idx.finish(), anchor=anchor,
                   early=True)
    fails = h.run(case)
    assert fails == [], "; ".join(fails)
    # what the harness flushed each time: four groups in ONE filter scan (above the three of an LDS-resident pass, so
    # with the flag forced the stationary kernel's).  Counted apart from the harness: timing puts events on the stream.
    _, n_scan = scan_launches(torch, idx, [(real["q"][i:i + 32], K) for i in range(0, 128, 32)])
    assert n_scan == 1
    idx.close()
