"""Stream contracts of include/tristage.h: the table of every entry point with a ``stream`` parameter, and the harness
of tests/test_stream_order_gpu.py that holds each one to its kind.

The harness is a LATE PRODUCER and an EARLY CONSUMER on a non-blocking side stream S.  Every device input of a call
starts out holding a decoy (another fully valid input of the same shape).  On S: a delay, then the copies that
overwrite the decoys with the real inputs (an event ``produced`` behind them), then the call under test, then at once
a consumer that clones the outputs.  After ``S.synchronize()`` the clones and the outputs themselves must equal, bit
for bit, what the same call gave beforehand on the default stream with everything synchronised.

  - work leaked to the null stream, or moved to an internal stream that does not wait for S, reads the decoy;
  - a result S is not made to wait for reaches the consumer as the sentinel (or as the decoy's result, which the
    warm-up run on S left in the allocator's blocks);
  - an "enqueue only" call that waits for the GPU finds ``produced`` complete when it returns.

A non-blocking stream does not synchronise with the null stream, which is why the default stream of the other GPU
tests (the legacy null stream, where everything is serialised implicitly) cannot show any of this.
"""
import os
import re
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tristage.h")

# ------------------------------------------------------------------------------------------------ the contract table
SYNC, ENQ, FINISH, FLUSH = "synchronous", "enqueue", "finish", "flush"
KINDS = (SYNC, ENQ, FINISH, FLUSH)
#   synchronous  the call returns with its results final: host outputs can be read, device outputs can be read from any
#                other stream; device inputs are read in stream order
#   enqueue      the call returns without waiting for the GPU; inputs are read and results are final in stream order
#   finish       synchronises the stream and completes every asynchronous search
#   flush        launches held work and orders the stream's later work behind it, without a host synchronisation

_S_CONV_SYNC = ("ts_index_add, ts_index_reconstruct, ts_index_range_fetch, ts_index_live_words, ts_index_compact, "
                "ts_index_remove and ts_index_update return after a synchronisation of `stream` behind their last step")
_S_CONV_IVF = "so does every IVF call that takes a stream, ts_mmr_ivf excepted"
_S_CONV_BM25 = "so do the ts_bm25_search calls, whose results are host memory"
_S_CONV_ENQ = ("ts_maxsim, ts_maxsim_indexed(_batch)(_fp8), ts_quantize_rows_fp8 and the forward kernels only enqueue on "
               "`stream` and return without a host synchronisation")
_S_SEARCH = "Synchronous with respect to `stream` on return."
_S_ORDER = "the update is ordered on `stream` behind every search submitted before it"
_S_PASSAGE = "Both run on the caller's stream without host synchronisation."
_S_MMR = "With device pointers the call only enqueues three kernels per chunk of queries on `stream`"

# name -> (kind, the header sentence the kind rests on, the case of tests/test_stream_order_gpu.py that covers it)
CONTRACT = {
    "ts_index_add": (SYNC, _S_CONV_SYNC, "flat_add"),
    "ts_index_search": (SYNC, _S_SEARCH, "flat_search_dense"),
    "ts_index_search_filtered": (SYNC, "Flags as for ts_index_search", "flat_search_allowed"),
    "ts_index_range_search": (SYNC, "Synchronous only; held coalesced passes are flushed first.", "flat_range_search"),
    "ts_index_range_fetch": (SYNC, _S_CONV_SYNC, "flat_range_search"),
    "ts_index_scores": (SYNC, _S_SEARCH, "flat_scores"),
    "ts_index_finish": (FINISH, "ts_index_finish synchronises the stream once and checks every unfinished search",
                        "flat_async_finish"),
    "ts_index_flush": (FLUSH, "`stream`'s later work is ordered behind it.  No host sync.", "queue_narrow"),
    "ts_index_remove": (SYNC, _S_ORDER, "order_remove_dense_B"),
    "ts_index_live_words": (SYNC, _S_CONV_SYNC, "flat_remove_compact"),
    "ts_index_compact": (SYNC, _S_CONV_SYNC, "flat_remove_compact"),
    "ts_index_update": (SYNC, _S_ORDER, "order_update_dense_B"),
    "ts_index_mmr": (ENQ, _S_MMR, "flat_mmr"),
    "ts_index_reconstruct": (SYNC, _S_CONV_SYNC, "flat_reconstruct"),
    "ts_merge_topk": (ENQ, "The stateless calls ts_merge_topk(_strided)", "merge_topk"),
    "ts_merge_topk_strided": (ENQ, "The stateless calls ts_merge_topk(_strided)", "merge_topk_packed"),
    "ts_group_topk": (ENQ, "the call enqueues one kernel", "group_topk"),
    "ts_maxsim": (ENQ, _S_CONV_ENQ, "maxsim"),
    "ts_maxsim_indexed": (ENQ, _S_CONV_ENQ, "maxsim_indexed"),
    "ts_maxsim_indexed_batch": (ENQ, _S_CONV_ENQ, "maxsim_indexed_batch"),
    "ts_quantize_rows_fp8": (ENQ, _S_CONV_ENQ, "quantize_rows_fp8"),
    "ts_maxsim_indexed_fp8": (ENQ, _S_CONV_ENQ, "maxsim_indexed_fp8"),
    "ts_maxsim_indexed_batch_fp8": (ENQ, _S_CONV_ENQ, "maxsim_indexed_batch_fp8"),
    "ts_maxsim_passages_indexed": (ENQ, _S_PASSAGE, "passages_indexed"),
    "ts_maxsim_passages_indexed_batch": (ENQ, _S_PASSAGE, "passages_indexed_batch"),
    "ts_bm25_search": (SYNC, _S_CONV_BM25, "bm25_search"),
    "ts_bm25_search_batch": (SYNC, "The same for nq queries with ONE synchronisation", "bm25_first_batch_on_side_stream"),
    "ts_bm25_search_batch_filtered": (SYNC, _S_CONV_BM25, "bm25_filtered"),
    "ts_add_layernorm": (ENQ, _S_CONV_ENQ, "add_layernorm"),
    "ts_add_prenorm": (ENQ, _S_CONV_ENQ, "add_prenorm"),
    "ts_embed_layernorm": (ENQ, _S_CONV_ENQ, "embed_layernorm"),
    "ts_attention_varlen": (ENQ, _S_CONV_ENQ, "attention_varlen"),
    "ts_rope_inplace": (ENQ, _S_CONV_ENQ, "rope_inplace"),
    "ts_geglu": (ENQ, _S_CONV_ENQ, "geglu"),
    "ts_linear_tile_weight": (ENQ, _S_CONV_ENQ, "linear_tile_weight"),
    "ts_linear_act": (ENQ, _S_CONV_ENQ, "linear_act"),
    "ts_linear_add_layernorm": (ENQ, _S_CONV_ENQ, "linear_add_layernorm"),
    "ts_mlp_add_layernorm": (ENQ, _S_CONV_ENQ, "mlp_add_layernorm"),
    "ts_ivf_train": (SYNC, _S_CONV_IVF, "ivf_train"),
    "ts_ivf_set_centroids": (SYNC, _S_CONV_IVF, "ivf_centroids"),
    "ts_ivf_get_centroids": (SYNC, _S_CONV_IVF, "ivf_centroids"),
    "ts_ivf_add": (SYNC, _S_CONV_IVF, "ivf_add"),
    "ts_ivf_search": (SYNC, "synchronous with respect to `stream`", "ivf_search"),
    "ts_ivf_probe": (SYNC, _S_CONV_IVF, "ivf_probe"),
    "ts_ivf_reconstruct": (SYNC, _S_CONV_IVF, "ivf_reconstruct"),
    "ts_remove_ivf": (SYNC, _S_CONV_IVF, "ivf_mutations_B"),
    "ts_update_ivf": (SYNC, _S_CONV_IVF, "ivf_mutations_B"),
    "ts_compact_ivf": (SYNC, "Ordered on `stream`, synchronous.", "ivf_mutations_B"),
    "ts_mmr_ivf": (ENQ, _S_MMR, "ivf_mmr"),
}

# name -> why no GPU case holds it to a kind (at most MAX_EXEMPT)
MAX_EXEMPT = 5
EXEMPT = {
    "ts_index_read_probe": "a measurement aid of bench.py: it returns timings of a read-only pass, which have no "
                           "expected bits; it writes nothing a caller reads in stream order",
}


def header_text() -> str:
    return open(HEADER).read()


def header_prose(text=None) -> str:
    """The header with comment decoration and line breaks folded away: what a quoted sentence is looked up in."""
    text = header_text() if text is None else text
    text = re.sub(r"^\s*\*(?!/)", " ", text, flags=re.M)
    return re.sub(r"\s+", " ", text)


def stream_prototypes(text=None):
    """The names of all prototypes of the header that take ``void* stream``, in header order."""
    text = header_text() if text is None else text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = []
    for m in re.finditer(r"\b(ts_\w+)\s*\(([^;{}()]*)\)\s*;", code):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def table_problems(contract=None, exempt=None, header=None, case_names=None):
    """Everything that is wrong with the table, as a list of messages (empty: the table covers the header)."""
    contract = CONTRACT if contract is None else contract
    exempt = EXEMPT if exempt is None else exempt
    protos = stream_prototypes(header)
    prose = header_prose(header)
    bad = []
    for name in protos:
        if name in contract and name in exempt:
            bad.append(f"{name}: both classified and exempt")
        elif name not in contract and name not in exempt:
            bad.append(f"{name}: takes a stream and is neither classified nor exempt")
    for name in list(contract) + list(exempt):
        if name not in protos:
            bad.append(f"{name}: not a prototype with a stream parameter")
    if len(exempt) > MAX_EXEMPT:
        bad.append(f"{len(exempt)} exemptions, at most {MAX_EXEMPT}")
    for name, why in exempt.items():
        if len(str(why).split()) < 5:
            bad.append(f"{name}: an exemption needs a written reason")
    for name, row in contract.items():
        if len(row) != 3:
            bad.append(f"{name}: a row is (kind, sentence, case)")
            continue
        kind, sentence, case = row
        if kind not in KINDS:
            bad.append(f"{name}: unknown kind {kind!r}")
        if not sentence or re.sub(r"\s+", " ", sentence) not in prose:
            bad.append(f"{name}: the header does not contain the sentence {sentence!r}")
        if not case:
            bad.append(f"{name}: no covering case")
        elif case_names is not None and case not in case_names:
            bad.append(f"{name}: the covering case {case!r} does not exist")
    return bad


# ------------------------------------------------------------------------------------------------------- the harness
DELAY_MS = 60.0          # chosen from the probe below: >= 10 x the slowest enqueue-only call, <= 250 ms
DELAY_MAX_MS = 250.0
SENT_F = -7.25e33        # no score, relevance or normalised value of any case
SENT_I = -0x5A5A5A5A


def bits(outs):
    """Outputs (CUDA tensors of any dtype, numpy arrays, None) -> a list of (shape, raw bytes).  Synchronises."""
    res = []
    for o in outs:
        if o is None:
            res.append(None)
        elif isinstance(o, np.ndarray):
            res.append((tuple(o.shape), np.ascontiguousarray(o).view(np.uint8).reshape(-1).copy()))
        else:
            import torch
            t = o.detach().contiguous()
            res.append((tuple(t.shape), t.reshape(-1).view(torch.uint8).cpu().numpy().copy()))
    return res


def same_bits(a, b) -> bool:
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if (x is None) != (y is None):
            return False
        if x is not None and (x[0] != y[0] or not np.array_equal(x[1], y[1])):
            return False
    return True


class Case:
    """One call under test.

    inputs()          -> (real, decoy): dicts of CUDA tensors with the same keys, shapes and dtypes; every mixture of
                         the two is a valid call.  Offsets and lengths are not in here: they are never decoyed.
    call(state, bufs) -> the outputs (CUDA tensors / numpy arrays), made on the current stream from ``bufs``
    setup()           -> fresh state for one invocation (an index the call changes), before anything is timed
    after(state, outs)   what completes the call (finish()), on the current stream
    cleanup(state)       after the stream is synchronised
    anchor(real, outs)   the family's oracle, applied once to the synchronous expected value
    early             the call is enqueue-only: it must return while the delay is still pending
    final             the call is synchronous: its outputs are final when it returns
    late              False: the inputs are complete before the call (TS_FLAG_PIPELINE): the early consumer only
    consume_after     the consumer reads after ``after`` (results that only finish() completes)
    """

    def __init__(self, name, inputs, call, setup=None, after=None, cleanup=None, anchor=None, early=False,
                 final=False, late=True, consume_after=False):
        self.name, self.inputs, self.call = name, inputs, call
        self.setup, self.after, self.cleanup, self.anchor = setup, after, cleanup, anchor
        self.early, self.final, self.late, self.consume_after = early, final, late, consume_after


class Harness:
    def __init__(self, torch):
        self.torch = torch
        self.S = torch.cuda.Stream()      # non-blocking with respect to the null stream: checked by self_check()
        self.S2 = torch.cuda.Stream()
        self.enqueue_ms = {}              # case -> host milliseconds of the call under test
        self.delay_ms = DELAY_MS
        self._calibrate()

    # -- the delay -------------------------------------------------------------------------------------------------
    def _timed(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def _calibrate(self):
        torch = self.torch
        torch.cuda.synchronize()
        if hasattr(torch.cuda, "_sleep"):
            cycles = 1_000_000
            torch.cuda._sleep(cycles)
            ms = self._timed(lambda: torch.cuda._sleep(cycles))
            if ms < 5.0:      # a fast counter: measure a longer spin
                cycles *= 20
                ms = self._timed(lambda: torch.cuda._sleep(cycles))
            self._cycles = max(1, int(cycles / ms * self.delay_ms))
            self._chain = None
            self.delay_kind = "torch.cuda._sleep"
        else:
            a = torch.eye(1024, device="cuda") * 0.5
            self._a = a
            n = 16

            def chain(steps=n):
                x = a
                for _ in range(steps):
                    x = x @ a
                return x
            chain()
            ms = self._timed(chain)
            self._chain = max(1, int(n / ms * self.delay_ms))
            self.delay_kind = "matmul chain"
        self.delay_measured_ms = self._timed(self.delay)

    def delay(self, scale=1.0):
        """Keeps the current stream busy for about ``scale * delay_ms``."""
        if self._chain is None:
            self.torch.cuda._sleep(max(1, int(self._cycles * scale)))
        else:
            x = self._a
            for _ in range(max(1, int(self._chain * scale))):
                x = x @ self._a
            self._keep = x

    # -- one case --------------------------------------------------------------------------------------------------
    def _invoke(self, case, bufs):
        st = case.setup() if case.setup else None
        outs = case.call(st, bufs)
        if case.after:
            case.after(st, outs)
        self.torch.cuda.synchronize()
        got = bits(outs)
        if case.cleanup:
            case.cleanup(st)
        return outs, got

    def run(self, case):
        """-> the list of failures of ``case`` (empty: it keeps its contract)."""
        torch = self.torch
        real, decoy = case.inputs()
        assert set(real) == set(decoy)
        for k in real:
            assert real[k].is_cuda and real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype, k
            assert real[k].is_contiguous() and decoy[k].is_contiguous(), k
        clone = lambda d: {k: v.clone() for k, v in d.items()}
        fails = []
        torch.cuda.synchronize()
        # the expected value and the decoy's: the default stream, everything synchronised
        outs, want = self._invoke(case, clone(real))
        if case.anchor:
            case.anchor(real, outs)
        del outs
        if case.late and real:
            _, want_decoy = self._invoke(case, clone(decoy))
            assert not same_bits(want, want_decoy), f"{case.name}: the decoy gives the real result: the case proves nothing"
        else:
            want_decoy = want
        bufs = clone(decoy if case.late else real)
        torch.cuda.synchronize()
        S = self.S
        keep = []
        with torch.cuda.stream(S):
            # warm-up on S itself: per-stream scratch, lazily made streams and events, the allocator's blocks
            _, warm = self._invoke(case, bufs)
            if not same_bits(warm, want_decoy):
                fails.append("the warm-up on the side stream differs from the default stream's result")
            if case.late:   # (a call that works in place has changed the buffers)
                for k in bufs:
                    bufs[k].copy_(decoy[k])
            torch.cuda.synchronize()
            st = case.setup() if case.setup else None
            self.delay()
            if case.late:
                for k in bufs:
                    bufs[k].copy_(real[k], non_blocking=True)
            produced = torch.cuda.Event()
            produced.record(S)
            t0 = time.perf_counter()
            outs = case.call(st, bufs)
            host_ms = (time.perf_counter() - t0) * 1e3
            returned_early = not produced.query()
            finals = None
            if case.final:   # a stream that waits for nothing reads the device outputs
                with torch.cuda.stream(self.S2):
                    finals = [o.clone() if hasattr(o, "is_cuda") else (None if o is None else o.copy()) for o in outs]
            if case.after and case.consume_after:
                case.after(st, outs)
            consumed = [o.clone() if hasattr(o, "is_cuda") else (None if o is None else o.copy()) for o in outs]
            if case.after and not case.consume_after:
                case.after(st, outs)
            keep.append((outs, consumed, finals, bufs, produced))
        S.synchronize()
        self.S2.synchronize()
        if case.early:
            self.enqueue_ms[case.name] = host_ms
            if not returned_early:
                fails.append(f"the call returned after its inputs were produced ({host_ms:.2f} ms on the host, a delay of "
                             f"{self.delay_measured_ms:.0f} ms): it waited for the GPU")
        if not same_bits(bits(consumed), want):
            fails.append("the stream-order consumer " + ("read the decoy's result" if same_bits(bits(consumed), want_decoy)
                                                          and want_decoy is not want else "did not read the expected result"))
        if not same_bits(bits(outs), want):
            fails.append("the outputs " + ("hold the decoy's result" if same_bits(bits(outs), want_decoy)
                                           and want_decoy is not want else "do not hold the expected result"))
        if finals is not None and not same_bits(bits(finals), want):
            fails.append("the outputs were not final when the call returned")
        if case.cleanup:
            case.cleanup(st)
        del keep
        return fails

    # -- the harness held to itself --------------------------------------------------------------------------------
    def self_check(self):
        """-> a dict of what the harness found about itself; the test asserts on it."""
        torch = self.torch
        S = self.S
        rep = {}
        # 1. S does not block against the null stream
        torch.cuda.synchronize()
        x = torch.ones(1, dtype=torch.int32, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32).pin_memory()
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            self.delay()
            s_ev = torch.cuda.Event()
            s_ev.record(S)
        flag.copy_(x, non_blocking=True)              # a tiny op on the default stream, seen on the host without an event
        d_ev = torch.cuda.Event()
        d_ev.record()
        deadline = time.perf_counter() + self.delay_measured_ms * 0.5e-3
        while int(flag[0]) != 1 and not d_ev.query() and time.perf_counter() < deadline:
            pass
        rep["default_copy_seen"] = int(flag[0]) == 1
        rep["default_event_done"] = bool(d_ev.query())
        rep["side_pending"] = not s_ev.query()
        rep["default_done_while_side_pending"] = rep["side_pending"] and (rep["default_copy_seen"] or rep["default_event_done"])
        S.synchronize()
        torch.cuda.synchronize()

        gen = torch.Generator(device="cuda").manual_seed(5)
        real = {"x": torch.randn(4096, device="cuda", generator=gen)}
        decoy = {"x": torch.randn(4096, device="cuda", generator=gen)}

        def honest(st, b):
            return (b["x"] * 2.0 + 1.0,)

        def leaks_to_the_default_stream(st, b):
            with torch.cuda.stream(torch.cuda.default_stream()):
                return (b["x"] * 2.0 + 1.0,)

        side = torch.cuda.Stream()

        def forgets_to_wait(st, b):
            """the work goes to an internal stream that waits for S, but S is not made to wait for it"""
            out = torch.full_like(b["x"], SENT_F)
            ready = torch.cuda.Event()
            ready.record()
            with torch.cuda.stream(side):
                side.wait_event(ready)
                self.delay(0.1)                       # the internal stream is late: the consumer on S is not
                torch.add(b["x"] * 2.0, 1.0, out=out)
            return (out,)

        def waits_for_the_gpu(st, b):
            out = b["x"] * 2.0 + 1.0
            torch.cuda.current_stream().synchronize()
            return (out,)

        inputs = lambda: (real, decoy)
        rep["honest"] = self.run(Case("honest", inputs, honest, early=True))
        rep["leak"] = self.run(Case("leak", inputs, leaks_to_the_default_stream, early=True))
        rep["no_wait"] = self.run(Case("no_wait", inputs, forgets_to_wait, early=True))
        side.synchronize()
        rep["host_wait"] = self.run(Case("host_wait", inputs, waits_for_the_gpu, early=True))
        self.enqueue_ms.pop("leak", None), self.enqueue_ms.pop("no_wait", None), self.enqueue_ms.pop("host_wait", None)
        self.enqueue_ms.pop("honest", None)
        return rep
