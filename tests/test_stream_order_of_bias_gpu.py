"""The boosted search held to the synchronous stream contract on a side stream, with the harness of
tests/stream_order.py as it is: the queries, the bias and the masks are written late on the side stream, the outputs are
consumed on it right behind the call.

A module of its own, named so that it is collected after test_stream_order_gpu.py: torch hands out side streams from a
pool in turn and the HIP runtime maps them onto its hardware queues in turn, and that module's self check needs its
side stream on another hardware queue than the null stream.  Streams taken before it would move its place in the
pool."""
import numpy as np
import pytest

import bias_model as bm
import stream_order as so
from helpers import make_corpus
from test_bias_gpu import N, _bias_dev, _dev, _index, _torch

pytestmark = pytest.mark.gpu


def test_search_biased_keeps_the_synchronous_contract_on_a_side_stream():
    """Inputs that arrive late on a non-blocking side stream, a consumer right behind the call: the results equal the
    default-stream run bit for bit and are final on return; the filter path and the dense path both."""
    from tristage_rag_amd.index import pack_allowed
    torch = _torch()
    dtype, d, B, k = "f16", 384, 33, 10
    ix = _index(make_corpus(N, d, seed=81, dtype=dtype), dtype)
    try:
        rng = np.random.default_rng(84)
        real_q, decoy_q = _dev(make_corpus(B, d, seed=82, dtype=dtype), dtype), _dev(make_corpus(B, d, seed=83, dtype=dtype), dtype)
        biases = [(0.1 * rng.standard_normal(N)).astype(np.float32) for _ in range(2)]
        real_b, decoy_b = (_bias_dev(b) for b in biases)
        masks = [rng.random(N) < 0.3 for _ in range(2)]
        real_m, decoy_m = (torch.from_numpy(pack_allowed(m, N).view(np.int32)).cuda() for m in masks)
        h = so.Harness(torch)
        inputs = lambda: ({"q": real_q, "bias": real_b, "mask": real_m}, {"q": decoy_q, "bias": decoy_b, "mask": decoy_m})
        cases = (
            so.Case("search_biased", inputs, lambda st, b: ix.search_biased(b["q"], k, b["bias"]), final=True),
            so.Case("search_biased masked", inputs,
                    lambda st, b: ix.search_biased(b["q"], k, b["bias"], allowed=b["mask"]), final=True),
            so.Case("search_biased dense", inputs,
                    lambda st, b: ix.search_biased(b["q"], k, b["bias"], allowed=b["mask"], exact_dense=True), final=True),
        )
        for case in cases:
            assert h.run(case) == [], case.name
        with torch.cuda.stream(h.S):
            side = ix.search_biased(real_q, k, real_b, allowed=real_m)
        want = bm.topk_model(ix.scores(real_q).cpu().numpy(), biases[0], k, allowed=masks[0])
        bm.same(side, want, "side stream against the model")
        bm.same(ix.search_biased(real_q, k, real_b, allowed=real_m), want, "default stream against the model")
    finally:
        ix.close()
