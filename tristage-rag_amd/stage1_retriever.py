"""Stage 1: dense candidate generation on the MI355X index (+ optional BM25 fusion).

Mirror of reference src/stage1_retriever.py: same class names, config fields,
attributes callers reach into (``documents``, ``doc_metadata``, ``faiss_index``,
``bm25_index``, ``model``) and result-dict schema (:403-416).
What differs underneath:

* ``faiss_index`` is a tristage_rag_amd.index.FlatIPIndex (HIP, exact inner
  product).  The reference switches to IndexIVFFlat(nlist=100, nprobe=10) when the
  first add has >1000 rows (:262-273), an approximation of the exact result this
  index returns; exact search is kept for every size by default.
  ``Stage1Config.index_type`` = "ivf" / "auto" selects tristage_rag_amd.index.IVFFlatIndex
  (nlist / nprobe; "auto" follows the reference's 1000-row rule).
* row normalisation ``x / (|x| + 1e-8)`` (:285-288) runs on the GPU inside
  ``add`` when the embeddings are already on the device.
* ``search_many`` batches queries through one index call (the reference loops one
  query at a time, src/retrieval_pipeline.py:444-448).
* BM25 keeps an inverted index instead of per-document dict scans; scores, tie
  order and the fusion arithmetic are the reference's (:35-112, :326-366).  One
  deliberate difference: ``fit`` rebuilds its statistics from scratch, where the
  reference appends to ``doc_freqs`` on every re-fit (:73-74) and misaligns
  document ids after a second ``add_documents``.
"""
from __future__ import annotations

import json
import logging
import math
import os
import re
from collections import OrderedDict, defaultdict
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import boost as _boost


@dataclass
class Stage1Config:
    model_name: str = "google/embeddinggemma-300m"
    device: str = "auto"
    cache_dir: str = "./models"
    index_dir: str = "./faiss_index"
    top_k_candidates: int = 500
    batch_size: int = 32
    index_batch_size: int = 256     # additive: documents per encoder forward in add_documents on the device path
    fuse_on_gpu: bool = True        # additive: search_many's RRF fusion for the whole query batch on the GPU (same float64
                                    # arithmetic and tie order as the per-query host code)
    amp_dtype: str = "bf16"         # additive: what use_fp16 means on the GPU — "bf16" (BASELINE configs[2]) or "fp16"
                                    # (what torch.cuda.amp.autocast() gives the reference, :235)
    max_text_length: int = 512
    enable_bm25: bool = True
    bm25_top_k: int = 300
    fusion_method: str = "rrf"  # "rrf" (Reciprocal Rank Fusion) or "weighted"
    rrf_k: int = 60
    dense_weight: float = 0.7
    bm25_weight: float = 0.3
    use_fp16: bool = True
    nlist: int = 100  # inverted lists of the IVF index (index_type "ivf", or "auto" above 1000 documents)
    nprobe: int = 10  # lists each query of the IVF index scans
    # "flat": exact search (default); "ivf": IVFFlatIndex(nlist, nprobe) trained on the first add_documents;
    # "auto": the reference's rule (:256-283) — IVF when the first add_documents brings more than 1000 documents
    index_type: str = "flat"
    # additive knobs (not in the reference)
    index_dtype: str = "f32"   # storage dtype of the corpus matrix: f32 | f16 | bf16 | fp8 (e4m3) | fp4 (4-bit MX), the last two flat index only
    gpu_index_device: int = 0
    bm25_on_gpu: Optional[bool] = None  # BM25 postings in HBM + HIP scoring kernels; None = whenever
                                        # the HIP index is in use (a GPU is present)
    use_hip_graph: bool = False  # replay single-query encoder forwards from HIP graphs
    bm25_refit_compat: bool = False  # BM25 statistics after a SECOND add_documents exactly as the reference computes them
                                     # (its fit() appends to the previous fit's lists; see BM25Index)
    mmr_lambda: Optional[float] = None  # None: off.  0 .. 1: search / search_many diversify the dense candidates by maximal
                                        # marginal relevance (top_k picks out of min(1024, 4 top_k) fetched; dense-only route)
    group_by: Any = None   # None: off.  A metadata key, or an integer array with one entry per document: search / search_many
                           # return the top_k best GROUPS, at most group_size documents of each (dense-only)
    group_size: int = 1
    funnel_dims: Optional[int] = None     # None: off.  A multiple of 128 below the embedding dimension: the dense candidates
                                          # come from FlatIPIndex.search_funnel (ranked on that prefix of the dimensions,
                                          # rescored exactly).  For Matryoshka-trained encoders.
    funnel_fetch_k: Optional[int] = None  # the funnel's shortlist; None: min(2048, max(8 top_k, 128))
    boost: Any = None                     # None: off.  A boost spec (boost.py): an array with one bias per document, a field
                                          # or decay dict, or a callable metadata -> float; the dense candidates come from
                                          # FlatIPIndex.search_biased, ranked by score + bias


def amp_torch_dtype(name: str):
    """"bf16" / "fp16" (also "bfloat16", "f16", "float16", "half") -> the torch dtype of the AMP forwards."""
    import torch
    key = str(name).lower()
    if key in ("bf16", "bfloat16"):
        return torch.bfloat16
    if key in ("fp16", "f16", "float16", "half"):
        return torch.float16
    raise ValueError(f"amp_dtype must be 'bf16' or 'fp16', not {name!r}")


_MISSING = object()   # a metadata key a document does not have: equal to no filter value


class BM25Index:
    """BM25 (k1=1.2, b=0.75) with the reference's tokenizer and idf
    (reference src/stage1_retriever.py:35-112), over an inverted index."""

    GPU_MAX_K = 2048   # the largest k of one ts_bm25_search* call (BM_MAX_K in ts_bm25.hip)

    def __init__(self, k1: float = 1.2, b: float = 0.75, gpu_device: Optional[int] = None, refit_compat: bool = False):
        self.k1 = k1
        self.b = b
        self.gpu_device = gpu_device   # None: score on the host; int: HIP kernels on that GPU
        # refit_compat: reproduce what the reference's BM25Index does when fit() is called AGAIN (every add_documents
        # after the first, src/stage1_retriever.py:316-322): its fit() appends to doc_freqs / doc_lens instead of
        # rebuilding them (:56-80), so the statistics of earlier fits are counted again in df and the average length,
        # and document i is scored with list entry i — for documents added later that is an EARLIER document's term
        # frequencies.  Off (default): fit() rebuilds, i.e. the scores the reference gives after ONE add_documents.
        self.refit_compat = bool(refit_compat)
        self._gpu = None
        import threading
        self._gpu_lock = threading.Lock()   # the GPU handle serves one caller at a time
        self._term_id: Dict[str, int] = {}
        self.doc_freqs: List[Dict[str, int]] = []
        self.idf: Dict[str, float] = {}
        self.doc_lens: List[int] = []
        self.avg_doc_len = 0
        self.corpus_size = 0
        self.vocabulary = set()
        self.documents: List[str] = []
        self._postings: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
        self._len_norm = np.zeros(0)

    def tokenize(self, text: str) -> List[str]:
        text = text.lower()
        text = re.sub(r"[^a-z0-9\s]", " ", text)
        return text.split()

    def fit(self, documents: Sequence[str], stats_exchange=None) -> None:
        """``stats_exchange(df, total_len, n_docs) -> (df, total_len, n_docs)`` (optional): the corpus-wide document
        frequencies, token count and document count when `documents` is only one row shard of the corpus
        (parallel_pipeline.ShardedBM25 all-gathers them): idf and the average length are then the GLOBAL ones, so a
        document's score is exactly what an index over the whole corpus gives it; ids stay local."""
        self.documents = list(documents)
        self.corpus_size = len(self.documents)
        keep = self.refit_compat and bool(self.doc_freqs)
        if not keep:
            self.doc_freqs, self.doc_lens = [], []
        self.idf = {}
        for doc in self.documents:
            tf: Dict[str, int] = defaultdict(int)
            toks = self.tokenize(doc)
            for t in toks:
                tf[t] += 1
            self.doc_freqs.append(tf)         # (refit_compat: BEHIND the entries of the earlier fits, like the reference)
            self.doc_lens.append(len(toks))
        n = self.corpus_size
        # document i is scored with list entry i (reference score(), :83-101); df and the average length run over
        # ALL entries (:76-80) — the same thing unless refit_compat kept entries of earlier fits
        post_d: Dict[str, List[int]] = defaultdict(list)
        post_tf: Dict[str, List[int]] = defaultdict(list)
        df: Dict[str, int] = defaultdict(int)
        for i, tf in enumerate(self.doc_freqs):
            for t, c in tf.items():
                df[t] += 1
                if i < n:
                    post_d[t].append(i)
                    post_tf[t].append(c)
        total_len, n_idf = sum(self.doc_lens), n
        if stats_exchange is not None:
            df, total_len, n_idf = stats_exchange(dict(df), total_len, n)
        self.vocabulary = set(df)
        self.avg_doc_len = total_len / n_idf if n_idf > 0 else 0
        for t, d_ in df.items():
            self.idf[t] = math.log((n_idf - d_ + 0.5) / (d_ + 0.5) + 1.0)
        self._postings = {t: (np.asarray(post_d[t], dtype=np.int64), np.asarray(post_tf[t], dtype=np.float64))
                          for t in post_d}
        lens = np.asarray(self.doc_lens[:n], dtype=np.float64)
        self._len_norm = (self.k1 * (1 - self.b + self.b * lens / self.avg_doc_len)
                          if self.avg_doc_len else np.zeros_like(lens))
        if self.gpu_device is not None:
            self._upload()

    # -- GPU mode ------------------------------------------------------------
    def _csr(self):
        """The index as ts_bm25_set_index takes it: (terms sorted, term_off int64 [V + 1], post_doc int32, post_tf
        float32, idf float64 [V], len_norm float64 [N]); term t's id is its place in `terms`."""
        terms = sorted(self._postings)
        off = np.zeros(len(terms) + 1, dtype=np.int64)
        for i, t in enumerate(terms):
            off[i + 1] = off[i] + len(self._postings[t][0])
        nnz = int(off[-1])
        docs = (np.concatenate([self._postings[t][0] for t in terms]).astype(np.int32)
                if nnz else np.zeros(1, np.int32))
        tfs = (np.concatenate([self._postings[t][1] for t in terms]).astype(np.float32)
               if nnz else np.zeros(1, np.float32))
        idf = np.array([self.idf[t] for t in terms], dtype=np.float64) if terms else np.zeros(1)
        ln = np.ascontiguousarray(self._len_norm, dtype=np.float64) if self.corpus_size else np.zeros(1)
        return terms, off, docs, tfs, idf, ln

    def _upload(self) -> None:
        """CSR postings + statistics -> HBM (ts_bm25_set_index)."""
        import ctypes
        from . import _lib
        lib = _lib.load()
        if self._gpu is None:
            self._gpu = ctypes.c_void_p()
            _lib.check(lib.ts_bm25_create(int(self.gpu_device), ctypes.byref(self._gpu)))
        terms, off, docs, tfs, idf, ln = self._csr()
        self._term_id = {t: i for i, t in enumerate(terms)}
        self._idf_of_id = idf[:len(terms)]
        _lib.check(lib.ts_bm25_set_index(self._gpu, self.corpus_size, len(terms), int(off[-1]),
                                         off.ctypes.data, docs.ctypes.data, tfs.ctypes.data,
                                         idf.ctypes.data, ln.ctypes.data, float(self.k1 + 1)))

    def _search_gpu(self, query: str, top_k: int) -> List[Tuple[int, float]]:
        return self._search_gpu_many([query], top_k)[0]

    def _search_gpu_many(self, queries: Sequence[str], top_k: int, arrays: bool = False, allowed=None):
        """All queries through ts_bm25_search_batch (ts_bm25_search_batch_filtered with ``allowed``: one bool
        array over the documents, or None, per query): one call and one synchronisation for the batch.

        The library lists the documents a query TOUCHES (at most GPU_MAX_K of them) and the untouched ones follow at
        0.0, which is the host's ranking as long as every touched document scores above 0.0.  A query with an
        idf <= 0 (refit_compat counts earlier fits' entries in df, so df > n happens) can leave touched documents at
        0.0 or below, beside or behind the untouched ones: such a query, and every query when top_k is above
        GPU_MAX_K, is scored by the host code from the same postings — the same arithmetic, the same lists."""
        from . import _lib
        lib = _lib.load()
        all_terms = [np.array([self._term_id[t] for t in self.tokenize(q) if t in self._term_id], dtype=np.int32) for q in queries]
        k = min(int(top_k), max(self.corpus_size, 1))
        on_host = [k > self.GPU_MAX_K or bool(len(t) and (self._idf_of_id[t] <= 0).any()) for t in all_terms]
        if any(on_host):
            return self._search_mixed(queries, top_k, arrays, allowed, on_host)
        terms = all_terms
        off = np.zeros(len(queries) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(t) for t in terms])
        flat = np.concatenate(terms) if len(terms) and off[-1] else np.zeros(1, dtype=np.int32)
        nq = len(queries)
        out_s = np.zeros((nq, max(k, 1)), dtype=np.float64)
        out_i = np.zeros((nq, max(k, 1)), dtype=np.int64)
        n_out = np.zeros(max(nq, 1), dtype=np.int32)
        if k > 0 and nq and off[-1]:
            with self._gpu_lock:      # one accumulator per handle, and ctypes drops the GIL for the call
                if allowed is None:
                    _lib.check(lib.ts_bm25_search_batch(self._gpu, flat.ctypes.data, off.ctypes.data, nq, k,
                                                        out_s.ctypes.data, out_i.ctypes.data, n_out.ctypes.data, None))
                else:
                    from .index import pack_allowed
                    packed, seen = [], {}
                    moq = np.full(nq, -1, dtype=np.int32)
                    for qi, a in enumerate(allowed):
                        if a is not None:
                            if id(a) not in seen:
                                seen[id(a)] = len(packed)
                                packed.append(pack_allowed(a, self.corpus_size))
                            moq[qi] = seen[id(a)]
                    bits = np.ascontiguousarray(np.stack(packed)) if packed else np.zeros((1, 1), np.uint32)
                    _lib.check(lib.ts_bm25_search_batch_filtered(
                        self._gpu, flat.ctypes.data, off.ctypes.data, nq, k, bits.ctypes.data, bits.shape[1],
                        len(packed), moq.ctypes.data, _lib.TS_FLAG_HOST_PTR, out_s.ctypes.data, out_i.ctypes.data,
                        n_out.ctypes.data, None))
        allow_of = (lambda q: None) if allowed is None else (lambda q: allowed[q])
        if arrays:      # (ids, scores) per query, no tuples: the array path of Stage1Retriever fuses them as they are
            out = []
            for q in range(nq):
                n = int(n_out[q])
                a = allow_of(q)
                want = min(int(top_k), self.corpus_size if a is None else int(np.count_nonzero(a)))
                if n < want:    # documents without a query term score exactly 0.0 and follow in ascending id order
                    pad = self._pad_with_zero_scores(list(zip(out_i[q, :n].tolist(), out_s[q, :n].tolist())), top_k, a)
                    out.append((np.array([i for i, _ in pad], dtype=np.int64), np.array([v for _, v in pad], dtype=np.float64)))
                else:
                    out.append((out_i[q, :n], out_s[q, :n]))
            return out
        return [self._pad_with_zero_scores(list(zip(out_i[q, : n_out[q]].tolist(), out_s[q, : n_out[q]].tolist())), top_k,
                                           allow_of(q))
                for q in range(nq)]

    def _search_mixed(self, queries, top_k, arrays, allowed, on_host):
        """_search_gpu_many when some queries are the host's (`on_host`): those through _search_host, the others in
        one GPU batch, every result in its query's place."""
        gpu_q = [q for q in range(len(queries)) if not on_host[q]]
        out = [None] * len(queries)
        if gpu_q:
            got = self._search_gpu_many([queries[q] for q in gpu_q], top_k, arrays,
                                        None if allowed is None else [allowed[q] for q in gpu_q])
            for q, r in zip(gpu_q, got):
                out[q] = r
        for q in range(len(queries)):
            if on_host[q]:
                r = self._search_host(queries[q], top_k, None if allowed is None else allowed[q])
                out[q] = ((np.array([i for i, _ in r], dtype=np.int64), np.array([v for _, v in r], dtype=np.float64))
                          if arrays else r)
        return out

    def _pad_with_zero_scores(self, res: List[Tuple[int, float]], top_k: int, allowed=None) -> List[Tuple[int, float]]:
        """``allowed`` (bool array over the documents, or None): a filtered search pads with allowed documents only."""
        if allowed is None:
            if len(res) < min(top_k, self.corpus_size):
                # every document with a non-zero score is listed; the rest score exactly 0.0 and
                # follow in ascending id order (the reference's stable sort)
                seen = {i for i, _ in res}
                d = 0
                while len(res) < min(top_k, self.corpus_size):
                    if d not in seen:
                        res.append((d, 0.0))
                    d += 1
            return res
        cand = np.flatnonzero(np.asarray(allowed, dtype=bool))
        want = min(int(top_k), int(cand.size))
        if len(res) < want:
            seen = {i for i, _ in res}
            for d in cand.tolist():
                if len(res) >= want:
                    break
                if d not in seen:
                    res.append((d, 0.0))
        return res

    def close(self) -> None:
        if self._gpu is not None:
            from . import _lib
            _lib.load().ts_bm25_destroy(self._gpu)
            self._gpu = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def score(self, query: str, doc_idx: int) -> float:
        if doc_idx >= len(self.doc_freqs):
            return 0.0
        f, dl, s = self.doc_freqs[doc_idx], self.doc_lens[doc_idx], 0.0
        for tok in self.tokenize(query):
            if tok in f and tok in self.idf:
                tf = f[tok]
                s += self.idf[tok] * ((tf * (self.k1 + 1)) /
                                      (tf + self.k1 * (1 - self.b + self.b * dl / self.avg_doc_len)))
        return s

    def scores(self, query: str) -> np.ndarray:
        """Scores of every document, accumulated term by term in query order
        (the same order of float additions as the per-document loop)."""
        acc = np.zeros(self.corpus_size, dtype=np.float64)
        for tok in self.tokenize(query):
            p = self._postings.get(tok)
            if p is None:
                continue
            ds, tf = p
            acc[ds] += self.idf[tok] * ((tf * (self.k1 + 1)) / (tf + self._len_norm[ds]))
        return acc

    def search_many(self, queries: Sequence[str], top_k: int = 10, allowed=None) -> List[List[Tuple[int, float]]]:
        """search() for several queries (the GPU index takes them in one call).  ``allowed``: None, or one bool
        array over the documents (or None) per query."""
        if self._gpu is not None:
            return self._search_gpu_many(list(queries), top_k, allowed=allowed)
        return [self.search(q, top_k, allowed=None if allowed is None else allowed[i]) for i, q in enumerate(queries)]

    def search_many_arrays(self, queries: Sequence[str], top_k: int = 10, allowed=None):
        """search_many() as (ids int64 [n], scores float64 [n]) per query."""
        if self._gpu is not None:
            return self._search_gpu_many(list(queries), top_k, arrays=True, allowed=allowed)
        out = []
        for qi, q in enumerate(queries):
            r = self.search(q, top_k, allowed=None if allowed is None else allowed[qi])
            out.append((np.fromiter((i for i, _ in r), dtype=np.int64, count=len(r)),
                        np.fromiter((v for _, v in r), dtype=np.float64, count=len(r))))
        return out

    def search(self, query: str, top_k: int = 10, allowed=None) -> List[Tuple[int, float]]:
        """``allowed``: a bool array over the documents — only those are ranked (zero scores included)."""
        if self._gpu is not None:
            if allowed is None:
                return self._search_gpu(query, top_k)
            return self._search_gpu_many([query], top_k, allowed=[allowed])[0]
        return self._search_host(query, top_k, allowed)

    def _search_host(self, query: str, top_k: int, allowed=None) -> List[Tuple[int, float]]:
        s = self.scores(query)
        if allowed is not None:
            cand = np.flatnonzero(np.asarray(allowed, dtype=bool))
            order = cand[np.argsort(-s[cand], kind="stable")[:top_k]]
            return [(int(i), float(s[i])) for i in order]
        order = np.argsort(-s, kind="stable")[:top_k]  # ties keep ascending doc order
        return [(int(i), float(s[i])) for i in order]


class Stage1Retriever:
    """Stage 1: dense embeddings + exact MI355X index + optional BM25 fusion."""

    def __init__(self, config: Stage1Config, model: Any = None,
                 index_factory: Optional[Callable[[int], Any]] = None):
        self.config = config
        self.logger = logging.getLogger(__name__)
        self.model = model
        self.embedding_dim: Optional[int] = None
        self.faiss_index = None
        self.index_type_used = "flat"   # the kind of faiss_index once it exists: "flat" or "ivf"
        self.bm25_index: Optional[BM25Index] = None
        self.documents: List[str] = []
        self.doc_metadata: List[Dict[str, Any]] = []
        self._removed: Optional[np.ndarray] = None   # remove_documents: True = removed (placeholders until compact)
        # filtered search: host bitmaps of the dict filters' (key, value) pairs, extended as documents arrive, and a
        # small LRU of packed device masks of whole dict filters.  Neither is persisted, and both belong to ONE
        # metadata list (_filter_cache_meta): when doc_metadata is replaced (load_index, the sharded pipeline) they
        # are dropped and rebuilt on first use.  Metadata is append-only in between (add_documents).
        self._kv_bitmaps: Dict[Any, np.ndarray] = {}
        self._mask_lru: "OrderedDict[Any, Any]" = OrderedDict()
        self._group_tables: Dict[Any, Dict[str, Any]] = {}   # group_by keys: value codes and their device copy (same owner)
        self._boost_lru: "OrderedDict[Any, Any]" = OrderedDict()   # boost specs: their bias arrays (_boost_bias)
        self._filter_cache_meta = self.doc_metadata
        self.filter_cache_size = 8
        self._index_factory = index_factory
        os.makedirs(self.config.cache_dir, exist_ok=True)
        os.makedirs(self.config.index_dir, exist_ok=True)
        self._load_model()

    # -- model -------------------------------------------------------------
    def _load_model(self) -> None:
        if self.model is None:
            from .encoders import SentenceEncoder
            self.logger.info(f"Loading Stage 1 model: {self.config.model_name}")
            self.model = SentenceEncoder(self.config.model_name, device=self.config.device,
                                         cache_folder=self.config.cache_dir,
                                         use_hip_graph=self.config.use_hip_graph)
        if hasattr(self.model, "get_sentence_embedding_dimension"):
            self.embedding_dim = self.model.get_sentence_embedding_dimension()
        else:
            self.embedding_dim = int(np.asarray(self.model.encode("sample text", convert_to_numpy=True)).shape[0])
        self.logger.info(f"Model loaded successfully. Embedding dimension: {self.embedding_dim}")

    def _amp_dtype(self):
        import torch
        return amp_torch_dtype(getattr(self.config, "amp_dtype", "bf16"))

    def _encode_batch(self, texts: List[str]) -> np.ndarray:
        """reference :230-254 — float32 [n, d] embeddings (AMP on the GPU when use_fp16)."""
        import torch
        dev = str(getattr(self.model, "device", "cpu"))
        if self.config.use_fp16 and dev.startswith("cuda"):
            with torch.autocast("cuda", dtype=self._amp_dtype()):
                emb = self.model.encode(texts, batch_size=self.config.batch_size, convert_to_numpy=True,
                                        show_progress_bar=False)
        else:
            emb = self.model.encode(texts, batch_size=self.config.batch_size, convert_to_numpy=True,
                                    show_progress_bar=False)
        return np.asarray(emb).astype(np.float32)

    def _normalize_embeddings(self, embeddings: np.ndarray) -> np.ndarray:
        """reference :285-288"""
        norms = np.linalg.norm(embeddings, axis=1, keepdims=True)
        return embeddings / (norms + 1e-8)

    # Device-resident variants: when the encoder runs on the GPU and the index is the HIP
    # index, embeddings never visit the host — rows are normalised inside ts_index_add
    # (TS_FLAG_NORMALIZE, the same x/(|x|+1e-8) in fp32) and queries stay tensors.
    def _bm25_device(self) -> Optional[int]:
        on = self.config.bm25_on_gpu
        if on is None:
            import torch
            on = self._index_factory is None and torch.cuda.is_available()
        return self.config.gpu_index_device if on else None

    def _device_path(self) -> bool:
        dev = str(getattr(self.model, "device", "cpu"))
        return (dev.startswith("cuda") and self._index_factory is None and
                getattr(self.model, "encode", None) is not None)

    def _encode_batch_tensor(self, texts: List[str], bulk: bool = False):
        import torch
        ctx = (torch.autocast("cuda", dtype=self._amp_dtype()) if self.config.use_fp16
               else torch.autocast("cuda", enabled=False))
        bs = max(self.config.batch_size, getattr(self.config, "index_batch_size", 0) or 0) if bulk else self.config.batch_size
        with ctx:
            emb = self.model.encode(texts, batch_size=bs, convert_to_numpy=False,
                                    convert_to_tensor=True, show_progress_bar=False)
        return emb.float()

    def _normalized_query_tensor(self, texts: List[str]):
        q = self._encode_batch_tensor(texts)
        return q / (q.norm(dim=1, keepdim=True) + 1e-8)

    # -- index -------------------------------------------------------------
    def _index_kind(self, n_first: int) -> str:
        """"flat" or "ivf" for an index whose first add brings ``n_first`` rows (Stage1Config.index_type)."""
        kind = getattr(self.config, "index_type", "flat")
        if kind not in ("flat", "ivf", "auto"):
            raise ValueError(f"index_type must be 'flat', 'ivf' or 'auto', not {kind!r}")
        if kind == "auto":
            return "ivf" if n_first > 1000 else "flat"   # reference :256-283
        return kind

    def _new_device_index(self, d: int, kind: str):
        if kind == "ivf":
            from .index import IVFFlatIndex
            # (the IVF index stores f16 / bf16 rows; an f32 index_dtype stores f16)
            dt = self.config.index_dtype if self.config.index_dtype in ("f16", "bf16") else "f16"
            if dt != self.config.index_dtype and not getattr(self, "_ivf_dtype_logged", False):
                self._ivf_dtype_logged = True
                self.logger.info(f"IVF index: index_dtype={self.config.index_dtype!r} is stored as f16")
            idx = IVFFlatIndex(d, int(self.config.nlist), dtype=dt, device=self.config.gpu_index_device,
                               nprobe=int(self.config.nprobe))
        else:
            from .index import FlatIPIndex  # raises without libtristage.so / a GPU: no CPU fallback
            idx = FlatIPIndex(d, dtype=self.config.index_dtype, device=self.config.gpu_index_device)
        self.index_type_used = kind
        return idx

    def _create_faiss_index(self, embeddings: np.ndarray) -> None:
        d = int(embeddings.shape[1])
        if self._index_factory is not None:
            self.faiss_index = self._index_factory(d)
        else:
            self.faiss_index = self._new_device_index(d, self._index_kind(len(embeddings)))
            if self.index_type_used == "ivf":
                self.faiss_index.train(embeddings)
        self.faiss_index.add(embeddings)
        self.logger.info(f"Index created with {len(embeddings)} vectors (exact inner product)")

    def add_documents(self, documents: List[str], metadata: Optional[List[Dict[str, Any]]] = None):
        if not documents:
            return
        self.logger.info(f"Adding {len(documents)} documents to Stage 1 index")
        self.documents.extend(documents)
        if metadata is None:
            metadata = [{}] * len(documents)  # one shared dict, as in the reference (:302)
        self.doc_metadata.extend(metadata)
        self._drop_boost_cache()
        if self._device_path():
            emb = self._encode_batch_tensor(list(documents), bulk=True)
            if self.faiss_index is None:
                self.faiss_index = self._new_device_index(int(emb.shape[1]), self._index_kind(int(emb.shape[0])))
                if self.index_type_used == "ivf":
                    self.faiss_index.train(emb / (emb.norm(dim=1, keepdim=True) + 1e-8))
            self.faiss_index.add(emb, normalize=True)
        else:
            embeddings = self._normalize_embeddings(self._encode_batch(list(documents)))
            if self.faiss_index is None:
                self._create_faiss_index(embeddings)
            else:
                self.faiss_index.add(embeddings)
        if self.config.enable_bm25:
            if self.bm25_index is None:
                self.bm25_index = BM25Index(gpu_device=self._bm25_device(),
                                            refit_compat=getattr(self.config, "bm25_refit_compat", False))
            self.bm25_index.fit(self.documents)
        self.logger.info(f"Documents added successfully. Total documents: {len(self.documents)}")

    # -- filters -----------------------------------------------------------
    def _reset_filter_caches(self) -> None:
        self._kv_bitmaps.clear()
        self._mask_lru.clear()
        self._group_tables = {}
        self._drop_boost_cache()
        self._filter_cache_meta = self.doc_metadata

    def _check_filter_caches(self) -> None:
        """Drop the filter caches if they were built from another metadata list than the current one."""
        if self._filter_cache_meta is not self.doc_metadata:
            self._reset_filter_caches()

    def _kv_bitmap(self, key, value) -> np.ndarray:
        """Documents whose metadata has ``key`` equal to ``value`` (bool [n_docs]); built once per (key, value)
        and extended by the documents added since."""
        n = len(self.doc_metadata)
        try:
            ck = (key, value)
            hash(ck)
        except TypeError:   # an unhashable value: evaluated per call
            return np.fromiter((md.get(key, _MISSING) == value for md in self.doc_metadata), dtype=bool, count=n)
        bm = self._kv_bitmaps.get(ck)
        if bm is not None and bm.shape[0] > n:   # (a shorter corpus than the bitmap: not the corpus it was built on)
            bm = None
        have = 0 if bm is None else bm.shape[0]
        if have < n:
            ext = np.fromiter((md.get(key, _MISSING) == value for md in self.doc_metadata[have:]), dtype=bool,
                              count=n - have)
            bm = ext if bm is None else np.concatenate([bm, ext])
            self._kv_bitmaps[ck] = bm
        return bm

    def filter_mask(self, filter) -> Optional[np.ndarray]:
        """A filter spec -> bool array over the documents (None: no filter).  Specs: a dict ``{key: value}``
        (every key equal; a list / tuple / set value means membership), a callable ``metadata -> bool``, a
        sequence of document indices, or a bool array over the documents."""
        n = len(self.documents)
        if filter is None:
            return None
        self._check_filter_caches()
        if isinstance(filter, dict):
            m = np.ones(n, dtype=bool)
            for key, value in filter.items():
                if isinstance(value, (list, tuple, set, frozenset)):
                    any_ = np.zeros(n, dtype=bool)
                    for v in value:
                        any_ |= self._kv_bitmap(key, v)
                    m &= any_
                else:
                    m &= self._kv_bitmap(key, value)
            return m
        if callable(filter):
            return np.fromiter((bool(filter(md)) for md in self.doc_metadata), dtype=bool, count=n)
        if hasattr(filter, "detach"):
            filter = filter.detach().cpu().numpy()
        arr = np.asarray(filter)
        if arr.dtype == np.bool_:
            if arr.shape != (n,):
                raise ValueError(f"a bool filter needs one entry per document ({n}), got shape {arr.shape}")
            return arr
        if arr.size == 0:
            return np.zeros(n, dtype=bool)
        if arr.ndim != 1 or not np.issubdtype(arr.dtype, np.integer):
            raise TypeError("filter: expected a dict, a callable, document indices or a bool array")
        if arr.min() < 0 or arr.max() >= n:
            raise ValueError(f"filter: document index out of range [0, {n})")
        m = np.zeros(n, dtype=bool)
        m[arr] = True
        return m

    @staticmethod
    def _is_spec(f) -> bool:
        return f is None or isinstance(f, (dict, list, tuple, np.ndarray)) or callable(f) or hasattr(f, "detach")

    def _per_query_filters(self, filter, nq: int) -> Optional[list]:
        """One filter for every query, or a list with one filter per query -> one filter per query (None: no
        filter at all).  A list of integers is one filter (document indices), not one per query."""
        if filter is None:
            return None
        per_query = (isinstance(filter, (list, tuple)) and len(filter) == nq and len(filter) > 0 and
                     all(self._is_spec(f) for f in filter) and not all(isinstance(f, (int, np.integer)) for f in filter))
        return list(filter) if per_query else [filter] * nq

    def _filter_masks(self, filter, nq: int) -> Optional[List[Optional[np.ndarray]]]:
        """-> one mask (or None) per query, None when no query is filtered.  With removed documents every query is
        filtered: its mask (all documents without a filter) ANDed with the live ones."""
        if filter is not None and getattr(self, "index_type_used", "flat") == "ivf":
            raise NotImplementedError("filtered search is not supported on an IVF index (index_type='ivf')")
        live = self.live_mask()
        specs = self._per_query_filters(filter, nq)
        if specs is None:
            return None if live is None else [live] * nq
        cache: Dict[int, Optional[np.ndarray]] = {}
        masks = []
        for f in specs:   # (one filter shared by the queries: resolved once)
            if id(f) not in cache:
                m = self.filter_mask(f)
                cache[id(f)] = m if live is None else (live if m is None else m & live)
            masks.append(cache[id(f)])
        return None if all(m is None for m in masks) else masks

    # -- removal ----------------------------------------------
    def live_mask(self) -> Optional[np.ndarray]:
        """bool array over the documents, False = removed; None while nothing is removed."""
        r = getattr(self, "_removed", None)
        if r is None or not r.any():
            return None
        live = np.ones(len(self.documents), dtype=bool)
        live[: r.size] = ~r[: len(self.documents)]
        return live

    @property
    def n_removed(self) -> int:
        r = getattr(self, "_removed", None)
        return 0 if r is None else int(np.count_nonzero(r))

    def _index_removes(self) -> bool:
        """The dense index drops removed rows itself (FlatIPIndex tombstones, IVFFlatIndex list holes)."""
        return self.faiss_index is not None and hasattr(self.faiss_index, "remove_ids")

    def remove_documents(self, doc_ids) -> int:
        """Removes documents by doc_id: they are never returned again (dense search, BM25 and the fusion), but keep
        their ids, their placeholder in ``documents`` / ``doc_metadata`` and their storage until :meth:`compact`.
        BM25 statistics stay those of every document added, as in Lucene, until :meth:`compact` refits them.
        Unknown and already removed ids are skipped; returns how many documents were removed."""
        n = len(self.documents)
        ids = np.unique(np.asarray(doc_ids, dtype=np.int64).reshape(-1))
        ids = ids[(ids >= 0) & (ids < n)]
        r = getattr(self, "_removed", None)
        if r is None or r.size < n:
            grown = np.zeros(n, dtype=bool)
            if r is not None:
                grown[: r.size] = r
            r = self._removed = grown
        ids = ids[~r[ids]]
        if ids.size == 0:
            return 0
        if self._index_removes():
            got = self.faiss_index.remove_ids(ids)
            if got != ids.size:
                raise RuntimeError(f"the index removed {got} of {ids.size} rows: it is out of step with the documents")
        r[ids] = True
        self._drop_boost_cache()
        return int(ids.size)

    def compact(self) -> np.ndarray:
        """Drops the removed documents for good: the index renumbers its live rows (FlatIPIndex.compact moves them
        down; IVFFlatIndex.compact rewrites its lists without their holes and keeps the centroids), documents /
        metadata lose their placeholders, BM25 is refitted on the survivors and the filter caches start over.  Only an
        index object without ``compact`` (a custom index_factory) is rebuilt from its reconstructed rows.
        Returns the old -> new doc_id map (-1 = removed), monotone."""
        n = len(self.documents)
        live = self.live_mask()
        if live is None:
            return np.arange(n, dtype=np.int64)
        old2new = np.full(n, -1, dtype=np.int64)
        old2new[live] = np.arange(int(np.count_nonzero(live)), dtype=np.int64)
        if self._index_removes() and hasattr(self.faiss_index, "compact"):
            got = self.faiss_index.compact()
            if not np.array_equal(got, old2new):
                raise RuntimeError("the index's compaction map differs from the documents' live set")
        elif self.faiss_index is not None:   # an index without tombstones: rebuilt from its live rows
            mat = self.faiss_index.reconstruct_n(0, self.faiss_index.ntotal)[live]
            self.faiss_index = None
            if len(mat):
                self._create_faiss_index(mat.astype(np.float32))
        keep = np.flatnonzero(live).tolist()
        self.documents = [self.documents[i] for i in keep]
        self.doc_metadata = [self.doc_metadata[i] for i in keep]   # (a new list: the filter caches start over)
        self._removed = None
        self._reset_filter_caches()
        if self.bm25_index is not None:   # a fresh fit on the survivors (refit_compat would append to the old one)
            self.bm25_index.close()
            self.bm25_index = None
            if self.documents:
                self.bm25_index = BM25Index(gpu_device=self._bm25_device(),
                                            refit_compat=getattr(self.config, "bm25_refit_compat", False))
                self.bm25_index.fit(self.documents)
        return old2new

    # -- update in place --------------------------------------
    def check_update(self, doc_ids, documents, metadata=None) -> np.ndarray:
        """The ids of an update as int64, or ``ValueError``: one text (and, when given, one metadata dict) per id, every
        id in range, given once and not removed.  All or nothing: called before any stage is touched."""
        ids = np.asarray(doc_ids, dtype=np.int64).reshape(-1)
        if len(documents) != ids.size or (metadata is not None and len(metadata) != ids.size):
            raise ValueError(f"update_documents: {ids.size} ids, {len(documents)} documents"
                             + ("" if metadata is None else f", {len(metadata)} metadata entries"))
        n = len(self.documents)
        seen = set()
        r = getattr(self, "_removed", None)
        for i in ids.tolist():
            if i < 0 or i >= n:
                raise ValueError(f"update_documents: doc_id {i} is not a document of this index ({n} documents)")
            if i in seen:
                raise ValueError(f"update_documents: doc_id {i} is given twice in one call")
            if r is not None and i < r.size and r[i]:
                raise ValueError(f"update_documents: doc_id {i} was removed")
            seen.add(i)
        return ids

    def update_documents(self, doc_ids, documents: List[str], metadata: Optional[List[Dict[str, Any]]] = None) -> int:
        """Replaces the documents ``doc_ids`` by ``documents`` under the same ids: the new texts are encoded on the path
        :meth:`add_documents` uses and written over the index rows (``update_rows``; an index object without it is
        rebuilt from its reconstructed rows with these replaced, the way :meth:`compact` falls back), the texts and,
        when given, the metadata are replaced, the filter caches start over when metadata changed and BM25 is refitted
        on the document list.  All or nothing (:meth:`check_update`).  Returns how many documents were updated."""
        ids = self.check_update(doc_ids, documents, metadata)
        if ids.size == 0:
            return 0
        documents = list(documents)
        if self._device_path():
            emb = self._encode_batch_tensor(documents, bulk=True)
            self.faiss_index.update_rows(ids, emb, normalize=True)
        else:
            embeddings = self._normalize_embeddings(self._encode_batch(documents))
            if hasattr(self.faiss_index, "update_rows"):
                self.faiss_index.update_rows(ids, embeddings)
            else:   # an index without update_rows (a custom index_factory): rebuilt with the rows replaced
                mat = np.array(self.faiss_index.reconstruct_n(0, self.faiss_index.ntotal), dtype=np.float32)
                mat[ids] = embeddings
                self.faiss_index = None
                self._create_faiss_index(mat)
                if self.n_removed and self._index_removes():
                    self.faiss_index.remove_ids(np.flatnonzero(self._removed))
        for j, i in enumerate(ids.tolist()):
            self.documents[i] = documents[j]
            if metadata is not None:
                self.doc_metadata[i] = metadata[j]
        if metadata is not None:
            self._reset_filter_caches()
        self._drop_boost_cache()
        if self.config.enable_bm25 and self.bm25_index is not None:
            if self.bm25_index.refit_compat:   # (its fit() appends to the old entries: document i would keep the old
                self.bm25_index.close()        # text's term frequencies; a fresh index, as compact() builds)
                self.bm25_index = BM25Index(gpu_device=self._bm25_device(), refit_compat=True)
            self.bm25_index.fit(self.documents)
        return int(ids.size)

    def _index_mask(self, filter, mask: np.ndarray):
        """What FlatIPIndex.search(allowed=) gets for one query: for a dict filter on a device index, packed words
        on the device from the LRU (a repeated tenant filter is neither re-packed nor re-uploaded)."""
        if mask is None or not isinstance(filter, dict) or not self._device_path():
            return mask
        self._check_filter_caches()
        try:
            key = (tuple(sorted((k, tuple(sorted(map(repr, v))) if isinstance(v, (list, tuple, set, frozenset)) else v)
                                for k, v in filter.items())), len(self.documents))
            hash(key)
        except TypeError:
            return mask
        hit = self._mask_lru.get(key)
        if hit is None:
            import torch
            from .index import pack_allowed
            words = pack_allowed(mask, len(self.documents))
            hit = torch.from_numpy(words.view(np.int32)).to(torch.device("cuda", self.config.gpu_index_device))
            self._mask_lru[key] = hit
            while len(self._mask_lru) > self.filter_cache_size:
                self._mask_lru.popitem(last=False)
        else:
            self._mask_lru.move_to_end(key)
        return hit

    def _dense_search(self, q, top_k: int, masks, filters, funnel=None, boost=None):
        """faiss_index.search, with ``allowed=`` when a filter is given; ``funnel`` = (dims, fetch_k): search_funnel;
        ``boost`` = a boost spec: search_biased with the spec's bias."""
        if boost is not None:
            bias = self._boost_bias(boost, on_device=hasattr(q, "is_cuda") and q.is_cuda)
            search = lambda q_, k_, **kw: self.faiss_index.search_biased(q_, k_, bias, **kw)
        elif funnel is not None:
            search = lambda q_, k_, **kw: self.faiss_index.search_funnel(q_, k_, funnel[0], fetch_k=funnel[1], **kw)
        else:
            search = self.faiss_index.search
        if masks is None:
            return search(q, top_k)
        per_q = self._per_query_filters(filters, len(masks)) or [None] * len(masks)
        # (a query whose only mask is the live set: the index applies its own tombstones)
        drop_live = self._index_removes()
        allowed = [None if (f is None and drop_live) else self._index_mask(f, m) for f, m in zip(per_q, masks)]
        if all(a is None for a in allowed):
            return search(q, top_k)
        same = all(a is allowed[0] for a in allowed)
        return search(q, top_k, allowed=allowed[0] if same else allowed)

    # -- funnel search -----------------------------------------
    def _funnel_args(self, funnel_dims, lam=None, grp=None):
        """The funnel of a search: ``(dims, fetch_k)`` from the argument, else from the config; None: off."""
        dims = self.config.funnel_dims if funnel_dims is None else funnel_dims
        if dims is None:
            return None
        if lam is not None or grp is not None:
            raise ValueError("funnel_dims cannot be combined with mmr_lambda or group_by")
        if getattr(self, "index_type_used", "flat") == "ivf":
            raise NotImplementedError("funnel search is not supported on an IVF index (index_type='ivf')")
        if self.faiss_index is not None and not hasattr(self.faiss_index, "search_funnel"):
            raise NotImplementedError(f"{type(self.faiss_index).__name__} has no search_funnel()")
        return int(dims), self.config.funnel_fetch_k

    # -- boosted search ----------------------------------------
    BOOST_CACHE_SIZE = 4

    def _drop_boost_cache(self) -> None:
        lru = getattr(self, "_boost_lru", None)
        if lru:
            lru.clear()

    def _boost_args(self, boost, lam=None, grp=None, fun=None):
        """The boost spec of a search (the argument, else the config), checked; None: off."""
        spec = self.config.boost if boost is None else boost
        if spec is None:
            return None
        if lam is not None or grp is not None or fun is not None:
            raise ValueError("boost cannot be combined with mmr_lambda, group_by or funnel_dims")
        _boost.check_spec(spec)
        if getattr(self, "index_type_used", "flat") == "ivf":
            raise NotImplementedError("boosted search is not supported on an IVF index (index_type='ivf')")
        if self.faiss_index is not None and not hasattr(self.faiss_index, "search_biased"):
            raise NotImplementedError(f"{type(self.faiss_index).__name__} has no search_biased()")
        dt = getattr(self.faiss_index, "storage_dtype", "f16")
        if dt not in ("f16", "bf16"):
            raise NotImplementedError(f"boosted search takes an f16 or bf16 index, not {dt}")
        return spec

    def _boost_bias(self, spec, on_device: bool):
        """The bias of ``spec`` over the documents: float32, one entry per document, a tensor on the index's GPU when
        ``on_device``.  An LRU of BOOST_CACHE_SIZE specs keeps the arrays (an array or a callable is one spec by
        identity); it is dropped whenever documents are added, updated, removed or compacted or the metadata list is
        replaced, as the filter caches are."""
        self._check_filter_caches()
        lru = getattr(self, "_boost_lru", None)
        if lru is None:
            lru = self._boost_lru = OrderedDict()
        key, keep = _boost.spec_key(spec)
        hit = lru.get(key)
        if hit is None:
            hit = {"keep": keep, "host": _boost.bias_array(spec, self.doc_metadata), "dev": None}
            lru[key] = hit
            while len(lru) > self.BOOST_CACHE_SIZE:
                lru.popitem(last=False)
        else:
            lru.move_to_end(key)
        if not on_device:
            return hit["host"]
        if hit["dev"] is None:
            import torch
            hit["dev"] = torch.from_numpy(hit["host"]).to(torch.device("cuda", self.config.gpu_index_device))
        return hit["dev"]

    # -- diversified dense search (MMR) ------------------------
    def _mmr_lambda(self, mmr_lambda) -> Optional[float]:
        """The lambda of a search (the argument, else the config); None: no diversification."""
        lam = self.config.mmr_lambda if mmr_lambda is None else mmr_lambda
        if lam is None:
            return None
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"mmr_lambda must be in [0, 1], got {mmr_lambda!r}")
        if self.config.enable_bm25 and self.bm25_index is not None:
            raise ValueError("mmr_lambda applies to the dense-only route: BM25 fusion is on (enable_bm25)")
        if self.faiss_index is not None and not hasattr(self.faiss_index, "mmr"):
            raise NotImplementedError(f"{type(self.faiss_index).__name__} has no mmr()")
        return lam

    def _dense_search_mmr(self, q, top_k: int, lam: float, masks, filters):
        """top_k picks by maximal marginal relevance out of the min(1024, 4 top_k) best dense candidates, selected on
        the GPU behind the search, on its stream."""
        from .index import MMR_MAX_FETCH, mmr_check
        top_k, fetch, lam = mmr_check(top_k, min(MMR_MAX_FETCH, 4 * int(top_k)), lam)
        D, I = self._dense_search(q, fetch, masks, filters)
        return self.faiss_index.mmr(I, D, top_k, lam)

    # -- grouped dense search ----------------------------------
    def _group_args(self, group_by, group_size, lam=None):
        """The grouping of a search: ``(group_by, group_size)`` from the arguments, else from the config; None: off."""
        if group_by is None:
            group_by, group_size = self.config.group_by, self.config.group_size
        if group_by is None:
            return None
        group_size = int(group_size)
        if group_size < 1:
            raise ValueError(f"group_size must be positive, got {group_size}")
        if lam is not None:
            raise ValueError("group_by cannot be combined with mmr_lambda: pick one way to thin out near-copies")
        if self.config.enable_bm25 and self.bm25_index is not None:
            raise ValueError("group_by applies to the dense-only route: BM25 fusion is on (enable_bm25)")
        if self.faiss_index is not None and not hasattr(self.faiss_index, "search_grouped"):
            raise NotImplementedError(f"{type(self.faiss_index).__name__} has no search_grouped()")
        return group_by, group_size

    def _group_codes(self, key) -> np.ndarray:
        """int32 [n_docs]: the value of metadata ``key`` coded in first-seen order, -1 for a document without the key.
        Built once per key and extended by the documents added since; dropped with the filter caches when the
        metadata list is replaced (remove + compact, update, load_index)."""
        self._check_filter_caches()
        tabs = self.__dict__.setdefault("_group_tables", {})
        ent = tabs.get(key)
        if ent is None:
            ent = tabs[key] = {"map": {}, "codes": np.zeros(0, dtype=np.int32), "dev": None}
        n = len(self.doc_metadata)
        have = ent["codes"].shape[0]
        if have > n:   # (a shorter corpus than the table: not the corpus it was built on)
            ent["map"], ent["codes"], ent["dev"], have = {}, ent["codes"][:0], None, 0
        if have < n:
            codes, ext = ent["map"], np.empty(n - have, dtype=np.int32)
            for j, md in enumerate(self.doc_metadata[have:]):
                v = md.get(key, _MISSING) if hasattr(md, "get") else _MISSING
                if v is _MISSING:
                    ext[j] = -1
                    continue
                try:
                    ext[j] = codes.setdefault(v, len(codes))
                except TypeError:
                    raise TypeError(f"group_by={key!r}: document {have + j} has the unhashable value {v!r}") from None
            ent["codes"] = np.concatenate([ent["codes"][:have], ext])
            ent["dev"] = None
        return ent["codes"]

    def _group_table(self, group_by, on_device: bool):
        """The group table of a search: a metadata key's codes (with their cached device copy) or the caller's array."""
        n = len(self.documents)
        if isinstance(group_by, (np.ndarray, list, tuple)) or hasattr(group_by, "detach"):
            arr = np.asarray(group_by.detach().cpu().numpy() if hasattr(group_by, "detach") else group_by)
            if arr.shape != (n,) or not np.issubdtype(arr.dtype, np.integer):
                raise ValueError(f"group_by: expected a metadata key or an integer array with one entry per document ({n}), "
                                 f"got shape {arr.shape}, dtype {arr.dtype}")
            if arr.size and (arr.max() > np.iinfo(np.int32).max or arr.min() < np.iinfo(np.int32).min):
                raise ValueError("group_by: the group ids must fit 32 bits")
            return arr.astype(np.int32)
        codes = self._group_codes(group_by)
        if not on_device:
            return codes
        ent = self._group_tables[group_by]
        if ent["dev"] is None:
            import torch
            ent["dev"] = torch.from_numpy(codes).to(torch.device("cuda", self.config.gpu_index_device))
        return ent["dev"]

    def _dense_search_grouped(self, q, top_k: int, grp, masks, filters):
        """The top_k best groups, at most group_size documents of each: _dense_search (filters and removed documents
        as ever) collapsed on the GPU behind it, refetched while a query's list was full and held too few groups.
        -> (D, I) [B, top_k * group_size], padded."""
        from .index import grouped_search
        group_by, group_size = grp
        tab = self._group_table(group_by, on_device=hasattr(q, "is_cuda") and q.is_cuda)
        D, I, _ = grouped_search(self.faiss_index, lambda x, f: self._dense_search(x, f, masks, filters), q, top_k, tab,
                                 group_size)
        return D, I

    def _pick_dense_search(self, lam, grp, fun=None, bst=None):
        if bst is not None:
            return lambda q_, k_, m_, f_: self._dense_search(q_, k_, m_, f_, boost=bst)
        if fun is not None:
            return lambda q_, k_, m_, f_: self._dense_search(q_, k_, m_, f_, funnel=fun)
        if grp is not None:
            return lambda q_, k_, m_, f_: self._dense_search_grouped(q_, k_, grp, m_, f_)
        if lam is not None:
            return lambda q_, k_, m_, f_: self._dense_search_mmr(q_, k_, lam, m_, f_)
        return self._dense_search

    # -- fusion ------------------------------------------------------------
    def _reciprocal_rank_fusion(self, dense_results, bm25_results):
        """reference :326-343"""
        scores: Dict[int, float] = defaultdict(float)
        for rank, (doc_idx, _) in enumerate(dense_results):
            scores[doc_idx] += 1.0 / (self.config.rrf_k + rank + 1)
        for rank, (doc_idx, _) in enumerate(bm25_results):
            scores[doc_idx] += 1.0 / (self.config.rrf_k + rank + 1)
        fused = [(i, s) for i, s in scores.items()]
        fused.sort(key=lambda x: x[1], reverse=True)
        return fused

    def _weighted_fusion(self, dense_results, bm25_results):
        """reference :345-366"""
        scores: Dict[int, float] = defaultdict(float)
        if dense_results:
            mx = max(s for _, s in dense_results)
            for i, s in dense_results:
                scores[i] += self.config.dense_weight * (s / mx)
        if bm25_results:
            mx = max(s for _, s in bm25_results)
            for i, s in bm25_results:
                scores[i] += self.config.bm25_weight * (s / mx)
        fused = [(i, s) for i, s in scores.items()]
        fused.sort(key=lambda x: x[1], reverse=True)
        return fused

    # -- search ------------------------------------------------------------
    def _finish(self, query: str, dense_results: List[Tuple[int, float]], top_k: int,
                allowed: Optional[np.ndarray] = None) -> List[Dict[str, Any]]:
        bm25_results: List[Tuple[int, float]] = []
        if self.config.enable_bm25 and self.bm25_index is not None:
            if allowed is None:
                bm25_results = self.bm25_index.search(query, self.config.bm25_top_k)
            else:   # the lexical half is filtered too: no disallowed document may come back through it
                bm25_results = self.bm25_index.search(query, self.config.bm25_top_k, allowed=allowed)
        if self.config.enable_bm25 and bm25_results:
            if self.config.fusion_method == "rrf":
                fused = self._reciprocal_rank_fusion(dense_results, bm25_results)
            else:
                fused = self._weighted_fusion(dense_results, bm25_results)
            final = fused[:top_k]
        else:
            final = dense_results[:top_k]
        results = []
        for doc_idx, score in final:
            if doc_idx < len(self.documents):
                results.append({"doc_id": doc_idx, "document": self.documents[doc_idx], "score": score,
                                "stage1_score": score, "metadata": self.doc_metadata[doc_idx],
                                "stage": "stage1"})
        return results

    def range_search(self, queries, min_score: float, filter=None, max_results: Optional[int] = None):
        """Every document whose dense score is at least ``min_score`` (inclusive), per query: a similarity cut-off
        instead of a top-k (FAISS ``range_search``, FlatIPIndex.range_search).  ``queries``: one string
        (-> the records :meth:`search` returns, sorted by descending score, ties by ascending doc_id) or a list of
        strings (-> one such list per query).  The dense index only: no BM25, no fusion.  ``filter`` as for
        :meth:`search`; removed documents are never returned.  ``max_results``: the most records the call may return
        in all (FlatIPIndex.range_search raises RangeSearchLimitError beyond it).  Not supported on an IVF index."""
        if self.faiss_index is None:
            raise ValueError("No documents indexed. Call add_documents() first.")
        if getattr(self, "index_type_used", "flat") == "ivf":
            raise NotImplementedError("range search is not supported on an IVF index (index_type='ivf')")
        single = isinstance(queries, str)
        texts = [queries] if single else list(queries)
        if not texts:
            return []
        nq = len(texts)
        masks = self._filter_masks(filter, nq)
        if self._device_path() and hasattr(self.faiss_index, "range_search"):
            allowed = None
            if masks is not None:
                per_q = self._per_query_filters(filter, nq) or [None] * nq
                drop_live = self._index_removes()   # (the index applies its own tombstones)
                allowed = [None if (f is None and drop_live) else self._index_mask(f, m) for f, m in zip(per_q, masks)]
                if all(a is None for a in allowed):
                    allowed = None
                elif all(a is allowed[0] for a in allowed):
                    allowed = allowed[0]
            lims, D, I = self.faiss_index.range_search(self._normalized_query_tensor(texts), float(min_score),
                                                       allowed=allowed, max_results=max_results, sort=True)
            lims, D, I = lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()
            per_query = [(I[lims[b]: lims[b + 1]], D[lims[b]: lims[b + 1]]) for b in range(nq)]
        else:
            # every score through the index's scores() route, cut on the host
            if not hasattr(self.faiss_index, "scores"):
                raise NotImplementedError("range search needs an index with range_search() or scores()")
            q = self._normalize_embeddings(self._encode_batch(texts))
            S = np.asarray(self.faiss_index.scores(np.ascontiguousarray(q, dtype=np.float32)))
            thr = np.float32(min_score)
            per_query, total = [], 0
            for b in range(nq):
                ok = S[b] >= thr
                if masks is not None and masks[b] is not None:
                    ok &= masks[b][: ok.shape[0]]
                ids = np.nonzero(ok)[0]
                order = np.lexsort((ids, -(S[b][ids] + np.float32(0.0))))
                per_query.append((ids[order], S[b][ids][order]))
                total += ids.size
            if max_results is not None and total > int(max_results):
                raise RuntimeError(f"range search: {total} results exceed the limit of {int(max_results)}")
        out = []
        for ids, scores in per_query:
            out.append([{"doc_id": int(i), "document": self.documents[int(i)], "score": float(s), "stage1_score": float(s),
                         "metadata": self.doc_metadata[int(i)], "stage": "stage1"}
                        for i, s in zip(ids, scores) if 0 <= int(i) < len(self.documents)])
        return out[0] if single else out

    def search(self, query: str, top_k: Optional[int] = None, filter=None,
               mmr_lambda: Optional[float] = None, group_by=None, group_size: int = 1,
               funnel_dims: Optional[int] = None, boost=None) -> List[Dict[str, Any]]:
        """``filter``: restrict the candidates to some documents (see :meth:`filter_mask`); fewer than
        ``top_k`` results when fewer documents are allowed, none when none are.
        ``mmr_lambda`` (default: the config's, None = off): the ``top_k`` records are picked by maximal marginal
        relevance out of the ``min(1024, 4 top_k)`` best dense candidates and come back in selection order, with their
        dense scores; 1.0 is the plain result.  Dense-only: ``ValueError`` while BM25 fusion is on.
        ``group_by`` (default: the config's, None = off): a metadata key, or an integer array with one entry per
        document (a document without the key, or with a negative entry, is a group of its own).  ``top_k`` then counts
        GROUPS: the records of the ``top_k`` groups with the best best-document come back in dense order, at most
        ``group_size`` of each (its best within the places fetched, FlatIPIndex.search_grouped).  Dense-only, and not
        together with ``mmr_lambda``: ``ValueError``.
        ``funnel_dims`` (default: the config's, None = off): the dense candidates are ranked on that prefix of the
        dimensions and a shortlist of ``funnel_fetch_k`` is rescored exactly (FlatIPIndex.search_funnel); filters and
        BM25 fusion work on its output as on the plain search's.  Not together with ``mmr_lambda`` or ``group_by``
        (``ValueError``); a flat f16 / bf16 index only (``NotImplementedError``).
        ``boost`` (default: the config's, None = off): a boost spec (boost.py): the dense candidates are the ``top_k``
        documents with the largest ``score + bias`` and carry that sum as their score (FlatIPIndex.search_biased, exact);
        filters and BM25 fusion work on its output as on the plain search's.  The bias arrays of the last 4 specs are kept:
        a dict is one spec by value, an array or a callable by IDENTITY, so an array changed in place (or a callable whose
        closure changed) has to be passed as a new object, or it gets the bias computed from it before.  Not together
        with ``mmr_lambda``, ``group_by`` or ``funnel_dims`` (``ValueError``); a flat f16 / bf16 index only
        (``NotImplementedError``)."""
        if self.faiss_index is None:
            raise ValueError("No documents indexed. Call add_documents() first.")
        top_k = top_k or self.config.top_k_candidates
        lam = self._mmr_lambda(mmr_lambda)
        grp = self._group_args(group_by, group_size, lam)
        fun = self._funnel_args(funnel_dims, lam, grp)
        bst = self._boost_args(boost, lam, grp, fun)
        masks = self._filter_masks(filter, 1)
        if masks is not None and not masks[0].any():
            return []
        dense_search = self._pick_dense_search(lam, grp, fun, bst)
        if self._device_path():
            D, I = dense_search(self._normalized_query_tensor([query]), top_k, masks, filter)
            scores, ids = D.cpu().numpy(), I.cpu().numpy()
        else:
            q = self._normalize_embeddings(self._encode_batch([query]))
            scores, ids = dense_search(q, top_k, masks, filter)
        dense = [(int(i), float(s)) for i, s in zip(ids[0], scores[0]) if i >= 0]
        results = self._finish(query, dense, top_k if grp is None else top_k * grp[1], None if masks is None else masks[0])
        self.logger.info(f"Stage 1 search completed. Found {len(results)} candidates")
        return results

    def search_many(self, queries: Sequence[str], top_k: Optional[int] = None, filter=None,
                    mmr_lambda: Optional[float] = None, group_by=None, group_size: int = 1,
                    funnel_dims: Optional[int] = None, boost=None) -> List[List[Dict[str, Any]]]:
        """All queries through ONE encoder pass and ONE index call (64 queries share a
        single sweep over the corpus on the GPU).  ``filter``: one filter for every query, or a list with one
        per query (None: unfiltered).  ``mmr_lambda``: as for :meth:`search`, one selection call for the batch.
        ``group_by`` / ``group_size``: as for :meth:`search`, one collapse for the batch.  ``funnel_dims``: as for
        :meth:`search`, one funnel for the batch.  ``boost``: as for :meth:`search`, one bias for the batch."""
        if self.faiss_index is None:
            raise ValueError("No documents indexed. Call add_documents() first.")
        top_k = top_k or self.config.top_k_candidates
        lam = self._mmr_lambda(mmr_lambda)
        grp = self._group_args(group_by, group_size, lam)
        fun = self._funnel_args(funnel_dims, lam, grp)
        bst = self._boost_args(boost, lam, grp, fun)
        if not queries:
            return []
        masks = self._filter_masks(filter, len(queries))
        dense_search = self._pick_dense_search(lam, grp, fun, bst)
        if self._device_path():
            D, I = dense_search(self._normalized_query_tensor(list(queries)), top_k, masks, filter)
            scores, ids = D.cpu().numpy(), I.cpu().numpy()
        else:
            q = self._normalize_embeddings(self._encode_batch(list(queries)))
            scores, ids = dense_search(q, top_k, masks, filter)
        out = []
        for qi, query in enumerate(queries):
            m = None if masks is None else masks[qi]
            if m is not None and not m.any():
                out.append([])
                continue
            dense = [(int(i), float(s)) for i, s in zip(ids[qi], scores[qi]) if i >= 0]
            out.append(self._finish(query, dense, top_k if grp is None else top_k * grp[1], m))
        return out

    def search_many_arrays(self, queries: Sequence[str], top_k: Optional[int] = None, filter=None,
                           group_by=None, group_size: int = 1, funnel_dims: Optional[int] = None, boost=None):
        """Stage 1 for a query batch WITHOUT building result records: (ids int64 [B, k'], scores [B, k'])
        as torch tensors on the index's device for the pure dense search, numpy arrays (float64 fused
        scores) when BM25 fusion is on.  Row q, in order, is exactly what ``search_many`` would list for
        query q.  None when the corpus holds fewer than top_k rows (the caller then uses ``search_many``,
        which deals with padded results).  ``filter`` as for :meth:`search_many`: None also when some query has
        fewer than top_k allowed documents.  ``group_by`` / ``group_size`` as for :meth:`search_many` (device path):
        rows of top_k * group_size entries; None also when some query's row would be padded.  ``funnel_dims`` as for
        :meth:`search_many`; None also when the funnel left some query's row padded.  ``boost`` as for
        :meth:`search_many`; None also when some query's boosted row would be padded."""
        import torch
        if self.faiss_index is None:
            raise ValueError("No documents indexed. Call add_documents() first.")
        top_k = top_k or self.config.top_k_candidates
        n = int(self.faiss_index.ntotal)
        if top_k > n or n != len(self.documents):
            return None
        grp = self._group_args(group_by, group_size, self.config.mmr_lambda)
        fun = self._funnel_args(funnel_dims, self.config.mmr_lambda, grp)
        bst = self._boost_args(boost, self.config.mmr_lambda, grp, fun)
        if self.config.mmr_lambda is not None:   # a diversified stage 1 goes through search_many
            return None
        if grp is not None:
            if not self._device_path():
                return None
            masks = self._filter_masks(filter, len(queries))
            if masks is not None and any(m is not None and not m.any() for m in masks):
                return None
            D, I = self._dense_search_grouped(self._normalized_query_tensor(list(queries)), top_k, grp, masks, filter)
            if bool((I[:, -1] < 0).any()):   # (kept entries come first: a padded row ends in -1)
                return None
            return I, D
        masks = self._filter_masks(filter, len(queries))
        if masks is not None:
            if any(m is not None and int(np.count_nonzero(m)) < top_k for m in masks):
                return None
            return self._search_many_arrays_filtered(list(queries), top_k, masks, filter, fun, bst)
        fuse = self.config.enable_bm25 and self.bm25_index is not None
        if fun is not None or bst is not None:
            if self._device_path():
                D, I = self._dense_search(self._normalized_query_tensor(list(queries)), top_k, None, None, funnel=fun,
                                          boost=bst)
            else:
                D, I = self._dense_search(self._normalize_embeddings(self._encode_batch(list(queries))), top_k, None, None,
                                          funnel=fun, boost=bst)
                D, I = torch.as_tensor(D), torch.as_tensor(I)
            if bool((I[:, -1] < 0).any()):   # (a shortlist, or a boosted list, that held fewer than top_k live rows)
                return None
        elif self._device_path():
            qt = self._normalized_query_tensor(list(queries))
            if not fuse and hasattr(self.faiss_index, "search_in_stream_order"):
                D, I = self.faiss_index.search_in_stream_order(qt, top_k)   # (ids stay on the GPU for stage 2: no wait here)
            else:
                D, I = self.faiss_index.search(qt, top_k)
        else:
            D, I = self.faiss_index.search(self._normalize_embeddings(self._encode_batch(list(queries))), top_k)
            D, I = torch.as_tensor(D), torch.as_tensor(I)
        if not fuse:
            return I, D
        bm25 = self.bm25_index
        if (self.config.fusion_method == "rrf" and I.is_cuda and getattr(self.config, "fuse_on_gpu", True)
                and hasattr(bm25, "search_many_arrays")):
            bms = bm25.search_many_arrays(list(queries), self.config.bm25_top_k)
            k2 = len(bms[0][0]) if bms else 0
            if k2 > 0 and all(len(b[0]) == k2 for b in bms):      # (ragged BM25 lists: the per-query host code below)
                return self._fuse_rrf_device(I, np.stack([b[0] for b in bms]), top_k)
        ids, scores = I.cpu().numpy(), D.cpu().numpy()
        out_i = np.empty((len(queries), top_k), dtype=np.int64)
        out_s = np.empty((len(queries), top_k), dtype=np.float64)
        bms = (bm25.search_many_arrays(list(queries), self.config.bm25_top_k) if hasattr(bm25, "search_many_arrays")
               else [bm25.search(q, self.config.bm25_top_k) for q in queries])
        for qi, bm in enumerate(bms):
            fi, fs = self._fuse_arrays(ids[qi], scores[qi], bm)
            if len(fi) < top_k:
                return None
            out_i[qi], out_s[qi] = fi[:top_k], fs[:top_k]
        return out_i, out_s

    def _search_many_arrays_filtered(self, queries: List[str], top_k: int, masks, filter, funnel=None, boost=None):
        """search_many_arrays with a filter (every query has >= top_k allowed documents), same return types as without
        one: torch tensors (ids, scores) for the pure dense search — on the index's device on the device path —,
        numpy arrays with float64 fused scores when BM25 fusion is on (through the host arrays code, _fuse_arrays,
        with the BM25 lists filtered alike)."""
        import torch
        if self._device_path():
            D, I = self._dense_search(self._normalized_query_tensor(queries), top_k, masks, filter, funnel=funnel,
                                      boost=boost)
        else:
            D, I = self._dense_search(self._normalize_embeddings(self._encode_batch(queries)), top_k, masks, filter,
                                      funnel=funnel, boost=boost)
            D, I = torch.as_tensor(D), torch.as_tensor(I)
        if (funnel is not None or boost is not None) and bool((I[:, -1] < 0).any()):   # (a shortlist that held fewer than top_k allowed rows)
            return None
        if not (self.config.enable_bm25 and self.bm25_index is not None):
            return I, D
        ids, scores = I.cpu().numpy(), D.cpu().numpy()
        bms = self.bm25_index.search_many_arrays(queries, self.config.bm25_top_k, allowed=masks)
        out_i = np.empty((len(queries), top_k), dtype=np.int64)
        out_s = np.empty((len(queries), top_k), dtype=np.float64)
        for qi, bm in enumerate(bms):
            fi, fs = self._fuse_arrays(ids[qi], scores[qi], bm)
            if len(fi) < top_k:
                return None
            out_i[qi], out_s[qi] = fi[:top_k], fs[:top_k]
        return out_i, out_s

    def _fuse_rrf_device(self, dense_ids, bm25_ids: np.ndarray, top_k: int):
        """Reciprocal rank fusion of a whole query batch on the GPU: dense_ids int64 [B, k1] (device, rank order), bm25_ids
        int64 [B, k2] (host, rank order) -> (ids int64 [B, top_k], fused scores float64 [B, top_k]) on the device.  The
        arithmetic of _fuse_arrays / _reciprocal_rank_fusion (reference :326-340) in float64 — 1 / (k + rank + 1), the
        dense term first, then the BM25 term — and its order: descending fused score, ties in first-seen order (dense
        list, then the BM25-only documents in BM25 order), by ONE stable sort per batch; bit-identical to the host code
        (tested)."""
        import torch
        dev = dense_ids.device
        B, k1 = dense_ids.shape
        b_ids = torch.from_numpy(np.ascontiguousarray(bm25_ids)).to(dev)
        k2 = int(b_ids.shape[1])
        rk = float(self.config.rrf_k)
        d_part = 1.0 / (rk + torch.arange(k1, dtype=torch.float64, device=dev) + 1)
        b_part = 1.0 / (rk + torch.arange(k2, dtype=torch.float64, device=dev) + 1)
        sorted_ids, order = torch.sort(dense_ids, dim=1, stable=True)
        pos = torch.searchsorted(sorted_ids, b_ids).clamp(max=k1 - 1)
        hit = torch.gather(sorted_ids, 1, pos) == b_ids                       # the BM25 document is in the dense list
        where = torch.gather(order, 1, pos)                                   # ... at this rank
        fused = d_part.expand(B, k1).clone()
        fused.scatter_add_(1, where, torch.where(hit, b_part.expand(B, k2), torch.zeros((), dtype=torch.float64, device=dev)))
        all_ids = torch.cat([dense_ids, b_ids], dim=1)
        minus_inf = torch.full((), float("-inf"), dtype=torch.float64, device=dev)
        all_sc = torch.cat([fused, torch.where(hit, minus_inf, 0.0 + b_part.expand(B, k2))], dim=1)
        srt, rank = torch.sort(all_sc, dim=1, descending=True, stable=True)
        return torch.gather(all_ids, 1, rank[:, :top_k]).contiguous(), srt[:, :top_k].contiguous()

    def _fuse_arrays(self, dense_ids: np.ndarray, dense_scores: np.ndarray, bm25_results):
        """The fusion of _finish() on arrays: same float64 arithmetic, same order (descending fused score,
        ties in first-seen order: dense list first, then the BM25-only documents) as the dictionary code of
        _reciprocal_rank_fusion / _weighted_fusion (reference :326-366)."""
        if isinstance(bm25_results, tuple):          # (ids, scores) arrays
            b_ids, b_sc = bm25_results
            if not len(b_ids):
                return dense_ids, dense_scores.astype(np.float64)
        else:                                         # [(id, score), ...]
            if not bm25_results:
                return dense_ids, dense_scores.astype(np.float64)
            b_ids = np.fromiter((i for i, _ in bm25_results), dtype=np.int64, count=len(bm25_results))
            b_sc = np.fromiter((s for _, s in bm25_results), dtype=np.float64, count=len(bm25_results))
        if self.config.fusion_method == "rrf":
            d_part = 1.0 / (self.config.rrf_k + np.arange(len(dense_ids), dtype=np.float64) + 1)
            b_part = 1.0 / (self.config.rrf_k + np.arange(len(b_ids), dtype=np.float64) + 1)
        else:
            d_sc = dense_scores.astype(np.float64)
            if (len(d_sc) and d_sc.max() == 0.0) or b_sc.max() == 0.0:
                raise ZeroDivisionError("float division by zero")   # what _weighted_fusion (and the reference) does
            d_part = self.config.dense_weight * (d_sc / d_sc.max()) if len(d_sc) else d_sc
            b_part = self.config.bm25_weight * (b_sc / b_sc.max())
        # position of every BM25 document in the dense list (or -1)
        order = np.argsort(dense_ids, kind="stable")
        pos = np.searchsorted(dense_ids[order], b_ids)
        pos = np.where(pos < len(order), pos, 0)
        hit = dense_ids[order][pos] == b_ids if len(order) else np.zeros(len(b_ids), dtype=bool)
        fused = d_part.copy()
        fused[order[pos[hit]]] = fused[order[pos[hit]]] + b_part[hit]          # dense term first, then the BM25 term
        all_ids = np.concatenate([dense_ids, b_ids[~hit]])
        all_sc = np.concatenate([fused, (0.0 + b_part[~hit])])
        rank = np.argsort(-all_sc, kind="stable")
        return all_ids[rank], all_sc[rank]

    # -- persistence (reference :421-465; raw matrix + JSON instead of pickle + faiss file)
    def save_index(self, index_path: Optional[str] = None):
        if index_path is None:
            index_path = os.path.join(self.config.index_dir, "stage1_index.pkl")
        base = os.path.splitext(index_path)[0]
        os.makedirs(os.path.dirname(os.path.abspath(index_path)), exist_ok=True)
        manifest = {"format": "tristage-rag_amd/1", "documents": self.documents,
                    "doc_metadata": self.doc_metadata,
                    # (a boost spec may be an array or a callable and belongs to the searches, not to the stored index)
                    "config": {k: v for k, v in self.config.__dict__.items() if k != "boost"},
                    "ntotal": 0, "dim": self.embedding_dim, "matrix": None,
                    "index_type": getattr(self, "index_type_used", "flat"), "centroids": None}
        if self.faiss_index is not None:
            # the stored rows, decoded to float32.  An fp8 index needs no format of its own: its decoded rows are e4m3
            # values times 2^-s, and quantising those again at load gives back the same bytes.  Nor does an fp4 index:
            # quantising its decoded rows gives back the same decoded values.
            mat = self.faiss_index.reconstruct_n(0, self.faiss_index.ntotal)
            np.save(base + ".matrix.npy", mat)
            manifest.update(ntotal=int(mat.shape[0]), dim=int(mat.shape[1]),
                            matrix=os.path.basename(base + ".matrix.npy"))
            if manifest["index_type"] == "ivf":   # the trained centroids: a reload neither retrains nor reassigns
                np.save(base + ".centroids.npy", self.faiss_index.centroids)
                manifest.update(centroids=os.path.basename(base + ".centroids.npy"),
                                nlist=int(self.faiss_index.nlist), ivf_dtype=self.faiss_index.storage_dtype)
        if self.live_mask() is not None:   # the tombstones: bool per document, True = removed
            np.save(base + ".removed.npy", ~self.live_mask())
            manifest.update(removed=os.path.basename(base + ".removed.npy"))
        with open(index_path, "w") as f:  # JSON under the reference's file name
            json.dump(manifest, f)
        self.logger.info(f"Stage 1 index saved to {index_path}")

    def load_index(self, index_path: Optional[str] = None):
        if index_path is None:
            index_path = os.path.join(self.config.index_dir, "stage1_index.pkl")
        if not os.path.exists(index_path):
            self.logger.warning(f"Index file not found: {index_path}")
            return
        with open(index_path, "rb") as f:
            head = f.read(1)
        if head != b"{":
            raise ValueError(f"{index_path} is not a tristage-rag_amd index manifest (a pickle written by the "
                             "reference is not loaded: unpickling executes code)")
        manifest = json.load(open(index_path))
        self.documents = manifest["documents"]
        self.doc_metadata = manifest["doc_metadata"]
        self._reset_filter_caches()   # the cached filter bitmaps describe the corpus that was here before
        self.faiss_index = None
        self.index_type_used = "flat"
        if manifest.get("matrix"):
            here = os.path.dirname(os.path.abspath(index_path))
            mat = np.load(os.path.join(here, manifest["matrix"]), allow_pickle=False)
            if manifest.get("index_type", "flat") == "ivf" and self._index_factory is None:
                from .index import IVFFlatIndex
                cent = np.load(os.path.join(here, manifest["centroids"]), allow_pickle=False)
                self.faiss_index = IVFFlatIndex(int(mat.shape[1]), int(manifest["nlist"]), dtype=manifest["ivf_dtype"],
                                                device=self.config.gpu_index_device, nprobe=int(self.config.nprobe))
                self.faiss_index.set_centroids(cent.astype(np.float32))
                self.faiss_index.add(mat.astype(np.float32))
                self.index_type_used = "ivf"
            elif self._index_factory is not None:
                self._create_faiss_index(mat.astype(np.float32))
            else:
                self.faiss_index = self._new_device_index(int(mat.shape[1]), "flat")
                self.faiss_index.add(mat.astype(np.float32))
        if self.config.enable_bm25 and self.documents:
            self.bm25_index = BM25Index(gpu_device=self._bm25_device())
            self.bm25_index.fit(self.documents)
        self._removed = None
        if manifest.get("removed"):   # (a manifest without the entry: every document live)
            removed = np.load(os.path.join(os.path.dirname(os.path.abspath(index_path)), manifest["removed"]),
                              allow_pickle=False)
            self.remove_documents(np.flatnonzero(removed))
        self.logger.info(f"Stage 1 index loaded from {index_path}")

    def get_stats(self) -> Dict[str, Any]:
        return {"total_documents": len(self.documents), "removed_documents": self.n_removed,
                "live_documents": len(self.documents) - self.n_removed, "embedding_dimension": self.embedding_dim,
                "faiss_index_type": type(self.faiss_index).__name__ if self.faiss_index else None,
                "index_type": getattr(self, "index_type_used", None) if self.faiss_index else None,
                "bm25_enabled": self.config.enable_bm25,
                "bm25_vocabulary_size": len(self.bm25_index.vocabulary) if self.bm25_index else 0,
                "config": self.config.__dict__}
