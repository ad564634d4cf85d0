"""The float64 model of range search on the exactly summable inputs of tests/exact_inputs.py, and the
path a pass must take.  No GPU is needed here; tests/test_range_search_host.py checks the model and the path table,
tests/test_range_search_gpu.py compares the library with it bit for bit."""
import functools

import numpy as np

import exact_inputs as ex

CAND_CAP = 16384           # candidate slots per query of the filter scan (ts_index.hip kCandCap)
MIN_FILTER_ROWS = 32768    # below this every pass is dense (kMinFilterRows)


_last = []   # the scores of the last (corpus, queries) pair: a test asks for many radii on one case


def _scores(corpus, queries):
    if not (_last and _last[0] is corpus and _last[1] is queries):
        _last[:] = [corpus, queries, ex.exact_scores(corpus, queries)]
    return _last[2]


def _ok(scores, radius, live, allowed):
    B, n = scores.shape
    r = np.broadcast_to(np.asarray(radius, np.float32), (B,)).astype(np.float64)
    ok = scores >= r[:, None]                                # inclusive; a NaN score fails it
    if live is not None:
        ok &= np.asarray(live, bool)[None, :]
    if allowed is not None:
        masks = allowed if isinstance(allowed, (list, tuple)) else [allowed] * B
        assert len(masks) == B
        for b, m in enumerate(masks):
            if m is not None:
                ok[b] &= np.asarray(m, bool)
    return ok


def expected_range(corpus, queries, radius, live=None, allowed=None, id_offset=0):
    """(lims int64 [B + 1], D float32, I int64): per query every live, allowed row with score >= radius, in ascending
    id order.  ``radius``: a scalar or one float32 per query."""
    s = _scores(corpus, queries)
    ok = _ok(s, radius, live, allowed)
    lims = np.zeros(s.shape[0] + 1, dtype=np.int64)
    np.cumsum(ok.sum(axis=1), out=lims[1:])
    b, i = np.nonzero(ok)                                    # row-major: queries in order, ids ascending
    return lims, s[b, i].astype(np.float32), i.astype(np.int64) + id_offset


def sort_segments(lims, D, I):
    """Each query's segment by descending score, ties by ascending id: the order of ``range_search(sort=True)``."""
    seg = np.repeat(np.arange(len(lims) - 1), np.diff(lims))
    order = np.lexsort((I, -D.astype(np.float64), seg))
    return D[order], I[order]


def rank_radius(corpus, queries, rank, live=None, allowed=None):
    """float32 [B]: each query's score at 1-based ``rank`` among its live, allowed rows (a scalar or one per query)."""
    s = _scores(corpus, queries)
    ok = _ok(s, -np.inf, live, allowed)
    s = np.where(ok, s, -np.inf)
    ranks = np.broadcast_to(np.asarray(rank), (s.shape[0],))
    srt = -np.sort(-s, axis=1)
    return srt[np.arange(s.shape[0]), ranks - 1].astype(np.float32)


def counts(corpus, queries, radius, live=None, allowed=None):
    return np.diff(expected_range(corpus, queries, radius, live, allowed)[0])


def queries_per_pass(dtype, d):
    """64, or 32 where the query image of 64 does not fit LDS beside the staging area (ts_index.hip `qp`): fp32
    storage above a padded dimension of 512."""
    if dtype != "f32":
        return 64
    dpad = (d + 63) // 64 * 64
    return 64 if dpad <= 512 else 32


def expected_paths(n, per_query_counts, dtype="f16", d=128, masked=False, exact_dense=False):
    """One entry per pass: "filter" (the filter scan and the id sort), "redo" (the filter scan, then the whole pass
    densely: a count above the cap) or "dense" (no filter scan: a small corpus, TS_FLAG_NO_FILTER, fp32 storage with
    masks or tombstones).  A query at exactly the cap stays on the filter path."""
    qp = queries_per_pass(dtype, d)
    out = []
    c = np.asarray(per_query_counts)
    for q0 in range(0, len(c), qp):
        if exact_dense or n < MIN_FILTER_ROWS or (masked and dtype == "f32"):
            out.append("dense")
        else:
            out.append("redo" if c[q0:q0 + qp].max() > CAND_CAP else "filter")
    return out


def info_of(paths):
    """What FlatIPIndex.last_range_info() must report for these passes."""
    return {"passes": len(paths), "filter_passes": sum(p != "dense" for p in paths),
            "dense_redo": sum(p == "redo" for p in paths)}


@functools.lru_cache(maxsize=4)
def guarded_case(cls, n, d, B):
    """ex.case, guarded: nothing is compared bit for bit that is not exactly summable."""
    corpus, queries, unit = ex.case(cls, n, d, B)
    ex.assert_exactly_summable(corpus, queries, unit)
    return corpus, queries
