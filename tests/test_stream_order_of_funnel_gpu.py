"""The funnel calls held to the synchronous stream contract on a side stream, with the harness of
tests/stream_order.py as it is.

A module of its own, named so that it is collected after test_stream_order_gpu.py: torch hands out side streams from a
pool in turn and the HIP runtime maps them onto its hardware queues in turn, and that module's self check needs its
side stream on another hardware queue than the null stream.  Streams taken before it would move its place in the
pool."""
import numpy as np
import pytest

import stream_order as so
from helpers import make_corpus
from test_funnel_gpu import N_FILTER, _dev, _index, _same, _torch

pytestmark = pytest.mark.gpu


def test_the_three_calls_keep_the_synchronous_contract_on_a_side_stream():
    """Inputs that arrive late on a non-blocking side stream, a consumer right behind the call (the harness of
    tests/stream_order.py as it is): the results equal the default-stream run bit for bit and are final on return."""
    torch = _torch()
    dtype, d, dims, B, k = "f16", 384, 256, 33, 10
    ix = _index(make_corpus(N_FILTER, d, seed=81, dtype=dtype), dtype)
    try:
        real_q, decoy_q = _dev(make_corpus(B, d, seed=82, dtype=dtype), dtype), _dev(make_corpus(B, d, seed=83, dtype=dtype), dtype)
        rng = np.random.default_rng(84)
        ids = [torch.from_numpy(rng.integers(0, N_FILTER, size=(B, 200)).astype(np.int64)).cuda() for _ in range(2)]
        h = so.Harness(torch)
        cases = (
            so.Case("search_funnel", lambda: ({"q": real_q}, {"q": decoy_q}),
                    lambda st, b: ix.search_funnel(b["q"], k, dims), final=True),
            so.Case("search_prefix", lambda: ({"q": real_q}, {"q": decoy_q}),
                    lambda st, b: ix.search_prefix(b["q"], k, dims), final=True),
            so.Case("rescore", lambda: ({"q": real_q, "ids": ids[0]}, {"q": decoy_q, "ids": ids[1]}),
                    lambda st, b: ix.rescore(b["q"], b["ids"], k), final=True),
        )
        for case in cases:
            assert h.run(case) == [], case.name
        with torch.cuda.stream(h.S):
            side = ix.search_funnel(real_q, k, dims)
        _same(side, ix.search_funnel(real_q, k, dims), "side stream against the default stream")
    finally:
        ix.close()
