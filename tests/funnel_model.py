"""Models of the funnel search for tests/test_funnel_host.py and tests/test_funnel_gpu.py.

``mirror_index``: what ``search_prefix`` is specified against, an index of ``dims`` dimensions and the same storage
dtype that holds the first ``dims`` components of every stored row under the same ids, with the same rows removed.
``rescore_model``: gather from the full score matrix, then ``np.lexsort`` on (-score, id).
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def mirror_index(ix, dims):
    """A ``FlatIPIndex(dims, dtype=<ix's>)`` holding ``ix.reconstruct_n()[:, :dims]`` under the same ids, with the rows
    removed that ``ix`` has removed.  The stored values are f16 / bf16 numbers already, so adding them as float32
    stores the same bytes."""
    from tristage_rag_amd.index import FlatIPIndex
    m = FlatIPIndex(int(dims), dtype=ix.storage_dtype, device=ix.device)
    if ix.ntotal:
        m.add(np.ascontiguousarray(ix.reconstruct_n()[:, :dims]))
        if ix.nlive < ix.ntotal:
            m.remove_ids(np.flatnonzero(~ix.live_mask()))
    return m


def rescore_model(scores, ids, k=None, live=None, id_offset=0):
    """``scores`` float32 [B, n] (``ix.scores(q)``), ``ids`` int64 [B, C] -> (D float32 [B, k], I int64 [B, k]): per
    query the valid entries by score descending, then id ascending; -1, out-of-range and removed ids (``live``: bool
    [n]) become -1 / -FLT_MAX at the end; a duplicate id stays a duplicate."""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids, np.int64)
    B, C = ids.shape
    n = scores.shape[1]
    k = C if k is None else int(k)
    D = np.full((B, k), -FLT_MAX, dtype=np.float32)
    I = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        rows = ids[b] - id_offset
        ok = (ids[b] != -1) & (rows >= 0) & (rows < n)
        if live is not None:
            ok[ok] &= np.asarray(live, bool)[rows[ok]]
        cid, crow = ids[b][ok], rows[ok]
        s = scores[b, crow] + np.float32(0.0)              # (-0 -> +0: equal scores are equal keys)
        order = np.lexsort((cid, -s.astype(np.float64)))[:k]
        D[b, : order.size] = s[order]
        I[b, : order.size] = cid[order]
    return D, I
