"""The float64 model of the BM25 kernels (ts_bm25.hip, DESIGN.md "BM25 kernels against a model"), written from the
formula: plain numpy / Python floats, one rounding per operation, no call into BM25Index.  No GPU is needed here;
tests/test_bm25_model_host.py checks the model itself, tests/test_bm25_kernels_gpu.py compares the library with it bit
for bit.

The C-level contract the model states (include/tristage.h, "BM25"):

* A query is a list of term ids in query order.  For each of them in turn, every document d in the term's postings
  (and in the query's allow mask, when it has one) receives
      acc[d] = acc[d] + idf[t] * ((tf * k1p1) / (tf + len_norm[d]))
  in float64, tf widened from float32, each operation rounded once.  A document is TOUCHED when it is in the postings
  of at least one term of the query (and allowed), whatever its contributions add up to — also 0.0, also below 0.0.
* A call returns the first min(k, n_touched) TOUCHED documents in the order (score descending, doc id ascending), with
  their scores, and n_out = min(k, n_touched).  Documents nobody touched score 0.0 and are never returned.
* With positive idf every touched document scores above 0.0, so n_out < k means "every document with a non-zero score
  is here, the rest score exactly 0.0 and follow in ascending id order".  With a non-positive idf a touched document may
  score 0.0 or less and would rank beside or below untouched ones: the C API still returns touched documents only
  (`search`), and ranking them against the untouched ones (`search_all`) is the caller's business — BM25Index takes its
  host path for such a query.
* A score of 0.0 is +0.0.
"""
import numpy as np

MAX_K = 2048        # BM_MAX_K: the largest k a call takes
PRE_MIN = 8192      # BM_PRE_MIN: the pre-filter runs when a query's postings total MORE, and its touched list is LONGER
CAND_CAP = 16384    # BM_CAND_CAP: a candidate list of at most this many documents is usable
LANES = 64          # queries per launch


class Csr:
    """An index as ts_bm25_set_index takes it."""

    def __init__(self, N, term_off, post_doc, post_tf, idf, len_norm, k1p1):
        self.N = int(N)
        self.term_off = np.ascontiguousarray(term_off, dtype=np.int64)
        self.post_doc = np.ascontiguousarray(post_doc, dtype=np.int32)
        self.post_tf = np.ascontiguousarray(post_tf, dtype=np.float32)
        self.idf = np.ascontiguousarray(idf, dtype=np.float64)
        self.len_norm = np.ascontiguousarray(len_norm, dtype=np.float64)
        self.k1p1 = float(k1p1)
        self.V = len(self.term_off) - 1
        self.nnz = int(self.term_off[-1])
        assert len(self.idf) == self.V and len(self.len_norm) == self.N
        assert len(self.post_doc) == self.nnz == len(self.post_tf)
        for t in range(self.V):       # a term's postings hit distinct documents: what makes the sums order-independent
            d = self.postings(t)[0]
            assert len(np.unique(d)) == len(d) and (len(d) == 0 or (0 <= d.min() and d.max() < self.N))

    def postings(self, t):
        lo, hi = self.term_off[t], self.term_off[t + 1]
        return self.post_doc[lo:hi], self.post_tf[lo:hi]

    def total(self, terms):
        """The sum of the posting lengths of a query: what the launcher compares with PRE_MIN."""
        return int(sum(self.term_off[t + 1] - self.term_off[t] for t in terms))


def from_postings(N, postings, idf, len_norm=None, k1p1=2.0):
    """postings: per term (docs, tfs) or docs alone (tf = 1.0)."""
    docs, tfs, off = [], [], [0]
    for p in postings:
        d, tf = p if isinstance(p, tuple) else (p, None)
        d = np.asarray(d, dtype=np.int32)
        docs.append(d)
        tfs.append(np.ones(len(d), np.float32) if tf is None else np.asarray(tf, dtype=np.float32))
        off.append(off[-1] + len(d))
    cat = (lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt))
    return Csr(N, off, cat(docs, np.int32), cat(tfs, np.float32), idf,
               np.ones(N) if len_norm is None else len_norm, k1p1)


def accumulate(ix, terms, allowed=None):
    """(acc float64 [N], touched bool [N]) of one query.  Every operation is its own ufunc call."""
    acc = np.zeros(ix.N, dtype=np.float64)
    touched = np.zeros(ix.N, dtype=bool)
    k1p1 = np.float64(ix.k1p1)
    with np.errstate(all="ignore"):
        for t in terms:
            d, tf32 = ix.postings(t)
            if allowed is not None:
                keep = np.asarray(allowed, bool)[d]
                d, tf32 = d[keep], tf32[keep]
            tf = tf32.astype(np.float64)
            num = np.multiply(tf, k1p1)
            den = np.add(tf, ix.len_norm[d])
            bracket = np.divide(num, den)
            c = np.multiply(ix.idf[t], bracket)
            acc[d] = np.add(acc[d], c)
            touched[d] = True
    return acc, touched


def accumulate_scalar(ix, terms, allowed=None):
    """`accumulate` one posting at a time in Python floats: nothing a vectorised expression could fuse."""
    acc = [0.0] * ix.N
    touched = [False] * ix.N
    for t in terms:
        d, tf32 = ix.postings(t)
        for j in range(len(d)):
            doc = int(d[j])
            if allowed is not None and not allowed[doc]:
                continue
            tf = float(tf32[j])
            num = tf * ix.k1p1
            den = tf + float(ix.len_norm[doc])
            bracket = num / den
            c = float(ix.idf[t]) * bracket
            acc[doc] = acc[doc] + c
            touched[doc] = True
    return np.array(acc, dtype=np.float64), np.array(touched, dtype=bool)


def ranked(acc, ids):
    """`ids` (ascending) by score descending, ties by ascending id: a stable descending sort."""
    ids = np.asarray(ids, dtype=np.int64)
    return ids[np.argsort(-acc[ids], kind="stable")]


def search(ix, terms, k, allowed=None):
    """What one C call returns: (ids int64 [n_out], scores float64 [n_out], n_out) — touched documents only."""
    acc, touched = accumulate(ix, terms, allowed)
    top = ranked(acc, np.flatnonzero(touched))[:k]
    return top, acc[top], len(top)


def search_all(ix, terms, k, allowed=None):
    """What BM25Index.search returns: every document (every allowed one) ranked, zero scores included."""
    acc, _ = accumulate(ix, terms, allowed)
    ids = np.arange(ix.N) if allowed is None else np.flatnonzero(np.asarray(allowed, bool))
    top = ranked(acc, ids)[:k]
    return top, acc[top]


# ---- the 96-bit key of the select (64 score bits, then the complemented id): bytes 0..7 score, 8..11 id ----------------
def score_key(v):
    u = int(np.float64(v + 0.0).view(np.uint64))
    return (~u) & (2**64 - 1) if u >> 63 else u | (1 << 63)


def key96(score, doc):
    return (score_key(score) << 32) | ((~int(doc)) & 0xFFFFFFFF)


def first_diff_byte(a, b):
    """The first byte (0 = most significant of 12) in which two 96-bit keys differ; None if they are equal."""
    for byte in range(12):
        sh = 8 * (11 - byte)
        if (a >> sh) & 0xFF != (b >> sh) & 0xFF:
            return byte
    return None


def boundary(ix, terms, k, allowed=None):
    """Of the touched list of a query: (n_touched, ties, byte) — how many touched documents score exactly what the
    k-th scores, and the key byte in which the k-th and the (k+1)-th first differ (None: fewer than k+1 touched)."""
    acc, touched = accumulate(ix, terms, allowed)
    order = ranked(acc, np.flatnonzero(touched))
    n = len(order)
    if n <= k:
        return n, (int((acc[order] == acc[order[-1]]).sum()) if n else 0), None
    a, b = order[k - 1], order[k]
    return n, int((acc[order] == acc[a]).sum()), first_diff_byte(key96(acc[a], a), key96(acc[b], b))
