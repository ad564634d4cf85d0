"""The constructed inputs of tests/test_bm25_kernels_gpu.py.  Each builder returns a `Case`: an index (bm25_model.Csr)
and searches, every search with the properties it is built for — how many documents it touches, how many tie at the
k-th place, the byte of the 96-bit key in which the k-th and (k+1)-th entries first differ, the select path it must
take.  tests/test_bm25_model_host.py checks every declared property on the model, so that a GPU test cannot pass on an
input that has lost what it was built for.

Planted scores: k1p1 = 2, tf = 1 and len_norm = 1 make the bracket exactly 1.0, so a contribution is exactly idf[t];
13 terms with idf[t] = 2^(-4t), and a document listed under term t iff bit t of its pattern is set.  A score is then a
sum of disjoint bits, exact in any order, and its bit pattern is the pattern's to choose."""
import collections
import functools

import numpy as np

import bm25_model as bm

Search = collections.namedtuple("Search", "terms k touched ties byte path")
Search.__new__.__defaults__ = (None, None, None, None)     # a property left None is not pinned
Case = collections.namedtuple("Case", "ix searches")

KS_RADIX = (1, 2, 255, 256, 257, 2047, 2048)
KS_PRE = (1, 300, 2048)
PLANTED_TERMS = 13
# key byte of the score in which term t's bit lies, for a score in [1, 2): t = 0 is the leading 1 (exponent bytes 0, 1)
BYTE_OF_TERM = (0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7)
FIRST_TERM_OF_BYTE = {b: BYTE_OF_TERM.index(b) for b in range(1, 8)}


def planted_index(patterns):
    patterns = np.asarray(patterns, dtype=np.int64)
    post = [np.flatnonzero((patterns >> t) & 1) for t in range(PLANTED_TERMS)]
    idf = [2.0 ** (-4 * t) for t in range(PLANTED_TERMS)]
    return bm.from_postings(len(patterns), post, idf, k1p1=2.0)


def planted_scores(patterns):
    """The exact scores, from integers: pattern -> v * 2^-48 with v < 2^49."""
    v = np.zeros(len(patterns), dtype=np.int64)
    for t in range(PLANTED_TERMS):
        v += ((np.asarray(patterns, np.int64) >> t) & 1) << (4 * (12 - t))
    return v.astype(np.float64) * 2.0 ** -48


def _rank_value(p):
    """Patterns order like their scores when read with term 0 as the most significant bit."""
    return sum(((p >> t) & 1) << (12 - t) for t in range(PLANTED_TERMS))


_ALL = np.arange(1, 1 << PLANTED_TERMS)
_ALL_RANK = np.array([_rank_value(int(p)) for p in _ALL])


@functools.lru_cache(maxsize=None)
def score_byte_case(byte, N=3000):
    """Radix passes 0-7: for every k of KS_RADIX its own corpus in which the k-th and (k+1)-th scores first differ in
    key byte `byte`.  The k-th document holds pattern A, k-1 documents hold larger patterns, the other N-k smaller
    ones that agree with A in every byte before `byte`.  All N documents are touched by the 13-term query.  (One Case
    per k; returned as a tuple of Cases.)"""
    rng = np.random.default_rng(100 + byte)
    cases = []
    for k in KS_RADIX:
        if byte == 0:      # A = 1.0; below: no leading term and nothing above 2^-16, whose exponent byte differs
            A = 1
            below = _ALL[((_ALL & 0b1111) == 0)]
        else:              # A = 1 + the first term of the byte; below: 1 + later terms only
            tb = FIRST_TERM_OF_BYTE[byte]
            A = 1 | (1 << tb)
            below = _ALL[((_ALL & 1) == 1) & (_ALL_RANK < _rank_value(A))]
        above = _ALL[_ALL_RANK > _rank_value(A)]
        pats = np.concatenate([rng.choice(above, size=k - 1), [A], rng.choice(below, size=N - k)])
        pats = pats[rng.permutation(N)]
        cases.append(Case(planted_index(pats), [Search(list(range(PLANTED_TERMS)), k, touched=N, byte=byte, path="short")]))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def short_list_case(N=3000, touched=100):
    """k above the number of touched documents: n_out = touched < k."""
    rng = np.random.default_rng(7)
    pats = np.zeros(N, dtype=np.int64)
    pats[rng.permutation(N)[:touched]] = rng.choice(_ALL, size=touched)
    return Case(planted_index(pats), [Search(list(range(PLANTED_TERMS)), k, touched=touched, path="short")
                                      for k in (touched, touched + 1, 255, 2048)])


@functools.lru_cache(maxsize=None)
def id_tie_case(N, X, h=3, ks=(4, 300, 2048), more=3000):
    """Id passes 8-11: `h` documents score 2.0, and a run of consecutive ids [X - (k - h), X + more) ties at 1.0, so
    that the k-th entry is id X - 1 and the (k+1)-th id X: choose X for the id byte in which those two first differ.
    One Case per k."""
    rng = np.random.default_rng(X % 1000 + 1)
    cases = []
    for k in ks:
        lo, hi = X - (k - h), min(N, X + more)
        assert 0 <= lo and X < hi
        high = set()
        while len(high) < h:
            d = int(rng.integers(0, N))
            if not lo <= d < hi:
                high.add(d)
        high = np.array(sorted(high))
        tied = np.arange(lo, hi)
        everyone = rng.permutation(np.concatenate([tied, high]))     # posting order is not id order
        ix = bm.from_postings(N, [everyone, high], [1.0, 1.0], k1p1=2.0)
        byte = bm.first_diff_byte(X - 1, X)     # ids as 12-byte numbers: their bytes are 8..11
        cases.append(Case(ix, [Search([0, 1], k, touched=len(everyone), ties=len(tied), byte=byte, path="short")]))
    return tuple(cases)


ID_TIE_SHAPES = {          # id byte -> (N, X): ids X - 1 and X first differ in that byte
    11: (3000, 0x0903),
    10: (3000, 0x0A00),
    9: (70_000, 0x10000),
}
TOP_ID_BYTE = dict(N=(1 << 24) + 64, X=1 << 24, h=3, ks=(8,), more=32)      # byte 8


def _distinct_norms(N, rng):
    """len_norm = 1 + j / N, every j once: with tf = 1 and one idf the scores 2 idf / (2 + j / N) are all different."""
    return 1.0 + rng.permutation(N) / N


@functools.lru_cache(maxsize=None)
def prefilter_case(name):
    """Pre-filter boundaries.  The path of each search is certain whatever order the atomics fill `touched` in:
      short     the touched list is <= PRE_MIN long (one of the next two): the select takes the touched list as it is;
      direct    the postings total <= PRE_MIN: the pre-filter is not launched;
      skip      the postings total more, the touched list is <= PRE_MIN long: bm25_tau leaves the lane alone;
      cand      PRE_MIN < touched <= CAND_CAP: the threshold is the m-th best of the sample with
                m = ceil(4 k 4096 / touched) >= k, so at least k and at most `touched` <= CAND_CAP documents pass;
      overflow  more than CAND_CAP documents tie at the threshold's score (everything ties, or the documents above
                the tied level are fewer than the smallest m): the list overflows, the select takes the touched list."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "twice_5000":
        N = 6000
        docs = rng.permutation(N)[:5000]
        ix = bm.from_postings(N, [docs], [1.0], _distinct_norms(N, rng))
        return Case(ix, [Search([0, 0], k, touched=5000, ties=1, path="skip") for k in KS_PRE])
    if name in ("touched_8192", "touched_8193"):
        n = int(name[-4:])
        N = 9000
        docs = rng.permutation(N)[:n]
        ix = bm.from_postings(N, [docs], [1.0], _distinct_norms(N, rng))
        s = [Search([0], k, touched=n, ties=1, path="direct" if n == 8192 else "cand") for k in KS_PRE]
        if n == 8192:
            s += [Search([0, 0], k, touched=n, ties=1, path="skip") for k in KS_PRE]
        return Case(ix, s)
    if name in ("tied_16384", "tied_16385"):
        n = int(name[-5:])
        N = 17_000
        docs = rng.permutation(N)[:n]
        ix = bm.from_postings(N, [docs], [1.0])
        return Case(ix, [Search([0], k, touched=n, ties=n, path="cand" if n == 16384 else "overflow") for k in KS_PRE])
    if name in ("two_level_12000", "two_level_17000"):
        low = int(name[-5:])
        N = 20_000
        docs = rng.permutation(N)[:low + 100]
        ix = bm.from_postings(N, [docs, rng.permutation(docs)[:100]], [1.0, 1.0])
        # k = 1 lies inside the high level; its threshold may come from either level (m = 8): any path, same result
        path = {12000: "cand", 17000: "overflow"}[low]
        return Case(ix, [Search([0, 1], k, touched=low + 100, ties=(100 if k == 1 else low),
                                path=("cand" if low == 12000 else None) if k == 1 else path) for k in KS_PRE])
    raise KeyError(name)


PREFILTER_CASES = ("twice_5000", "touched_8192", "touched_8193", "tied_16384", "tied_16385", "two_level_12000",
                   "two_level_17000")


def _random_postings(rng, N, V, df_lo, df_hi, tf_of):
    post = []
    for _ in range(V):
        df = int(rng.integers(df_lo, df_hi + 1))
        post.append((np.sort(rng.permutation(N)[:df]), tf_of(df)))
    return post


@functools.lru_cache(maxsize=None)
def arithmetic_case(N=5000, V=200):
    """Accumulation arithmetic: tf with non-integers, 1e-3 and 1e6; len_norm over 1e-3 .. 1e3; idf over 1e-300 .. 1e300
    in one index and tiny ones whose products are subnormal; queries of up to 40 tokens with repeats."""
    rng = np.random.default_rng(4)

    def tf_of(df):
        kind = rng.integers(0, 5, size=df)
        tf = rng.integers(1, 30, size=df).astype(np.float64)
        tf = np.where(kind == 1, rng.uniform(0.1, 9.0, size=df), tf)
        tf = np.where(kind == 2, 1e-3, tf)
        tf = np.where(kind == 3, 1e6, tf)
        return tf.astype(np.float32)

    post = _random_postings(rng, N, V, 1, 600, tf_of)
    idf = np.exp(rng.uniform(np.log(1e-3), np.log(20.0), size=V))
    idf[:12] = [1e-300, 1e300, 3e-305, 7e-306, 1.5e-307, 1e-150, 1e150, 2.5e-300, 4e299, 1e-303, 9e-308, 6e-310]
    idf = idf[rng.permutation(V)]
    len_norm = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size=N))
    ix = bm.from_postings(N, post, idf, len_norm, k1p1=2.2)
    extreme = np.flatnonzero((idf < 1e-100) | (idf > 1e100))
    searches = []
    for q in range(48):
        nt = int(rng.integers(1, 41))
        terms = rng.integers(0, V, size=nt)
        if q % 2:                                    # every other query carries extreme idf values, some of them twice
            terms[rng.integers(0, nt, size=min(nt, 4))] = rng.choice(extreme, size=min(nt, 4))
        if q % 3 == 0 and nt > 2:
            terms[nt // 2] = terms[0]
            terms[-1] = terms[0]
        searches.append(Search([int(t) for t in terms], (10, 300, 2048)[q % 3]))
    return Case(ix, searches)


@functools.lru_cache(maxsize=None)
def lanes_case(N=10_000, V=60):
    """Lanes and chunks: an index with three terms above PRE_MIN documents and many short ones, and batches of
    1, 63, 64, 65, 130 queries: lanes without a term between lanes with long lists, a lane above and a lane below
    PRE_MIN in one launch, the same query in several lanes."""
    rng = np.random.default_rng(5)
    tf_of = (lambda df: rng.integers(1, 9, size=df).astype(np.float32))
    post = _random_postings(rng, N, V - 3, 1, 300, tf_of)
    post += [(np.sort(rng.permutation(N)[:df]), tf_of(df)) for df in (8193, 9000, 9999)]
    idf = rng.uniform(0.05, 6.0, size=V)
    ix = bm.from_postings(N, post, idf, rng.uniform(0.3, 3.0, size=N), k1p1=2.2)
    long_terms = [V - 3, V - 2, V - 1]
    pool = [[], [long_terms[0]], [3], [long_terms[1], 5, long_terms[1]], [], [7, 7, 8], long_terms, [3]]
    for _ in range(40):
        pool.append([int(t) for t in rng.integers(0, V - 3, size=int(rng.integers(1, 9)))])
    batches = []
    for nq in (1, 63, 64, 65, 130, 1):
        # queries 0..: an empty one between two long ones, then the pool round and round (repeats in different lanes)
        qs = [[long_terms[2], 1]] if nq == 1 else [pool[(i * 7 + nq) % len(pool)] if i % 9 else pool[i % 8] for i in range(nq)]
        if nq > 3:
            qs[0], qs[1], qs[2] = [long_terms[0], 2], [], [long_terms[1]]
            qs[-1] = qs[0]
        batches.append(qs)
    return Case(ix, batches)       # (searches = batches of term lists here; k is the test's)


@functools.lru_cache(maxsize=None)
def mask_case(N=1003, V=30):
    """Masked accumulate: N is no multiple of 32; allowed sets {31}, {32}, {N-1}, none, all and a random half."""
    rng = np.random.default_rng(6)
    tf_of = (lambda df: rng.integers(1, 9, size=df).astype(np.float32))
    post = _random_postings(rng, N, V - 1, 50, 400, tf_of) + [(np.arange(N), tf_of(N))]     # the last term: everyone
    ix = bm.from_postings(N, post, rng.uniform(0.05, 6.0, size=V), rng.uniform(0.3, 3.0, size=N), k1p1=2.2)
    masks = []
    for only in ([31], [32], [N - 1], [], None):
        m = np.zeros(N, dtype=bool)
        if only is None:
            m[:] = True
        else:
            m[only] = True
        masks.append(m)
    masks.append(rng.random(N) < 0.5)
    return ix, masks


def pack_masks(masks, words):
    """bool [n_masks, N] -> uint32 [n_masks, words]: bit d % 32 of word d / 32 = document d allowed."""
    out = np.zeros((len(masks), words), dtype=np.uint32)
    for i, m in enumerate(masks):
        d = np.flatnonzero(m)
        np.bitwise_or.at(out[i], d >> 5, np.uint32(1) << (d & 31).astype(np.uint32))
    return out


@functools.lru_cache(maxsize=None)
def negative_case(N=400):
    """Negative and cancelling contributions, on exact numbers (bracket = 1.0, contribution = idf):
      term 0  idf +1.0   documents 0..99          term 1  idf -1.0   documents 50..149
      term 2  idf +0.5   documents 60..69, 200    term 3  idf -0.25  documents 300..309
    Documents 50..99 are back at exactly 0.0 after terms 0, 1; 60..69 then receive a third contribution."""
    ix = bm.from_postings(N, [np.arange(0, 100), np.arange(50, 150), np.r_[np.arange(60, 70), 200], np.arange(300, 310)],
                          [1.0, -1.0, 0.5, -0.25], k1p1=2.0)
    return Case(ix, [
        Search([3], 5, touched=10, ties=10),                    # every touched document is below 0.0; 390 are untouched
        Search([0, 1], 400, touched=150, ties=50),              # 50 at +1, 50 back at exactly 0.0, 50 at -1
        Search([0, 1, 2], 400, touched=151, ties=50),           # ... 10 of the cancelled ones at +0.5 after a third term
        Search([0, 1, 2], 70, touched=151, ties=40),
        Search([1, 0, 2, 3, 1], 2048, touched=161),
    ])
