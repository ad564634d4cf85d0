"""The model of the boosted search, built from the product's own dense scores: ``S = index.scores(q)``
is float32; a row's boosted score is the float32 sum ``S + bias``, one addition.  ``topk_model`` drops the rows a query
may not see, orders by (boosted score descending, id ascending), cuts at ``k`` and pads with -1 / -FLT_MAX, as
``search`` pads.  Comparisons against it are equalities of ids and of score values (``-0.0 == 0.0``).

``decay64`` and ``spec_bias64`` are the written-out float64 model of the boost specs (boost.py), rounded once."""
import math

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def boosted(S, bias):
    """float32 [B, n]: one float32 addition per pair."""
    S = np.asarray(S)
    bias = np.asarray(bias)
    assert S.dtype == np.float32 and bias.dtype == np.float32 and bias.shape == (S.shape[1],)
    return (S + bias[None, :]).astype(np.float32)


def topk_model(S, bias, k, live=None, allowed=None, id_offset=0):
    """``(D, I)`` float32 / int64 ``[B, k]``.  ``live``: bool [n] (rows that were not removed); ``allowed``: a bool [n]
    mask, or a list with one mask or None per query.  Returned ids carry ``id_offset``."""
    Sb = boosted(S, bias)
    B, n = Sb.shape
    ok = np.ones((B, n), dtype=bool)
    if live is not None:
        ok &= np.asarray(live, bool)[None, :]
    if allowed is not None:
        masks = allowed if isinstance(allowed, (list, tuple)) else [allowed] * B
        assert len(masks) == B
        for b, m in enumerate(masks):
            if m is not None:
                ok[b] &= np.asarray(m, bool)
    ok &= ~np.isnan(Sb)                                            # a NaN boosted score is never returned
    D = np.full((B, k), -FLT_MAX, dtype=np.float32)
    I = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        rows = np.flatnonzero(ok[b])
        sb = Sb[b, rows] + np.float32(0.0)                         # -0.0 and +0.0 are one score
        order = np.argsort(-sb.astype(np.float64), kind="stable")[:k]      # stable: equal scores keep ascending ids
        D[b, : order.size] = sb[order]
        I[b, : order.size] = rows[order] + id_offset
    return D, I


def same(got, want, what=""):
    """Equality of ids and of score VALUES (no tolerance)."""
    gd, gi = (np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in got)
    wd, wi = want
    assert gi.shape == wi.shape and gd.shape == wd.shape, f"{what}: shapes {gi.shape} / {wi.shape}"
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert bad.size == 0, f"{what}: ids differ in queries {bad[:5].tolist()}, first at column " \
                          f"{int(np.flatnonzero(gi[bad[0]] != wi[bad[0]])[0])}"
    assert np.array_equal(gd, wd), f"{what}: scores differ"


# --------------------------------------------------------------------------------------------------- boost specs
def decay64(kind, x, scale, decay_value):
    """Elasticsearch's decay functions of the distance x >= 0 in float64: 1 at x = 0, decay_value at x = scale."""
    if kind == "exp":
        lam = math.log(decay_value) / scale
        return math.exp(lam * x)
    if kind == "gauss":
        sigma2 = -scale * scale / (2.0 * math.log(decay_value))
        return math.exp(-x * x / (2.0 * sigma2))
    if kind == "linear":
        s = scale / (1.0 - decay_value)
        return max(0.0, (s - x) / s)
    raise ValueError(kind)


def spec_bias64(spec, metadata):
    """float32 bias of a dict spec over ``metadata``, every formula in float64, rounded once."""
    out = np.empty(len(metadata), dtype=np.float64)
    w = float(spec.get("weight", 1.0))
    for i, m in enumerate(metadata):
        v = m.get(spec["field"])
        if v is None:
            out[i] = float(spec.get("missing", 0.0))
        elif "decay" not in spec:
            out[i] = w * float(v)
        else:
            x = max(0.0, abs(float(v) - float(spec["origin"])) - float(spec.get("offset", 0.0)))
            out[i] = w * decay64(spec["decay"], x, float(spec["scale"]), float(spec.get("decay_value", 0.5)))
    return out.astype(np.float32)
