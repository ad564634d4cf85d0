"""RetrievalPipeline — the three-stage orchestrator, API-compatible with the
reference's src/retrieval_pipeline.py.

Kept verbatim: ``PipelineConfig`` field names and defaults
(reference :52-87), ``RetrievalPipeline(config_path=None, config=None)``, lazy
``initialize_stages`` (:238-290), ``add_documents`` (:292-321), ``search`` with its
result keys ``query / results / stage1_results / stage2_results / timing /
performance_stats`` and the early returns when a stage yields nothing (:323-424),
``batch_search``, ``save_index`` / ``load_index``, ``get_pipeline_info``,
``export_config``, the running-mean ``performance_stats`` (:567-606).

MI355X-side differences: stage 1 is the exact HIP index, stage 2 one MaxSim
kernel launch per query, no ``torch.cuda.empty_cache()`` per query, and
``search_many`` pushes a whole query batch through one stage-1 sweep.
Additive config fields carry a default so reference YAML files still load.
"""
from __future__ import annotations

import logging
import os
import time
from dataclasses import asdict, dataclass, fields
from typing import Any, Dict, List, Optional

import numpy as np
import yaml

from .stage1_retriever import Stage1Config, Stage1Retriever
from .stage2_rescorer import ColBERTScorer, Stage2Config
from .stage3_reranker import AdaptiveCrossEncoderReranker, Stage3Config


@dataclass
class PipelineConfig:
    """All knobs of the three-stage pipeline (reference src/retrieval_pipeline.py:15-87)."""
    # Stage 1
    stage1_model: str = "google/embeddinggemma-300m"
    stage1_top_k: int = 500
    stage1_batch_size: int = 32
    stage1_enable_bm25: bool = True
    stage1_bm25_top_k: int = 300
    stage1_fusion_method: str = "rrf"
    stage1_use_fp16: bool = True
    # Stage 2
    stage2_model: str = "lightonai/GTE-ModernColBERT-v1"
    stage2_top_k: int = 100
    stage2_batch_size: int = 16
    stage2_max_seq_length: int = 192
    stage2_use_fp16: bool = True
    stage2_scoring_method: str = "maxsim"
    # Stage 3
    stage3_model: str = "cross-encoder/ms-marco-MiniLM-L6-v2"
    stage3_top_k: int = 20
    stage3_batch_size: int = 32
    stage3_max_length: int = 256
    stage3_use_fp16: bool = True
    # General
    device: str = "auto"
    cache_dir: str = "./models"
    index_dir: str = "./faiss_index"
    log_level: str = "INFO"
    log_file: str = "retrieval_pipeline.log"
    enable_timing: bool = True
    save_intermediate_results: bool = False
    auto_cleanup: bool = True
    max_memory_usage_gb: float = 4.0
    # ---- additive (MI355X) ----
    stage1_index_dtype: str = "f32"          # corpus storage on the GPU: f32 | f16 | bf16 | fp8 (e4m3) | fp4 (4-bit MX), the last two flat index only
    stage1_bm25_on_gpu: Optional[bool] = None  # BM25 postings in HBM, HIP scoring; None = when a GPU is used
    stage1_bm25_refit_compat: bool = False     # BM25 after a second add_documents as the reference computes it (appended statistics)
    stage2_cache_document_embeddings: bool = False
    stage2_precompute_document_embeddings: bool = False  # token store filled by add_documents
    use_hip_graphs: bool = False             # query forwards of stages 1/2 and a query's stage-3 pairs replayed from HIP graphs
    stage2_token_store_dtype: str = "auto"   # "auto": bf16 under AMP, else the encoder's output type; or bf16 | f16 | f32 | fp8
    amp_dtype: str = "bf16"                     # what stage*_use_fp16 means on the GPU: "bf16" (BASELINE configs[2]) or "fp16"
                                                # (what torch.cuda.amp.autocast() gives the reference on a GPU)
    stage1_index_batch_size: int = 256          # documents per encoder forward at add_documents time (stage 1, device path)
    stage2_index_batch_size: int = 256          # ... and for the stage-2 token store
    tune_gemms: bool = False                    # PyTorch TunableOp: the fastest hipBLASLt / rocBLAS solution per GEMM shape,
                                                # found by timing at the shape's first occurrence (~1 s each, kept in the
                                                # process and in tune_gemms_file): the 1024-pair stage-3 forward 9.6 -> 8.7 ms
    tune_gemms_file: str = ""                   # results file (read at start, written at exit); "" = TunableOp's default name
    stage3_width_multiple: int = 1              # pad the token width of search_many's stage-3 batches to a multiple of this
                                                # (16 with tune_gemms: bounds the number of GEMM shapes to tune)
    search_on_arrays: bool = True               # search() takes the array path of search_many when its preconditions hold
    stage3_cache_document_tokens: bool = False  # tokenise every document once at add time; search_many then assembles
                                                # the cross-encoder inputs from token ids on the GPU
    stage3_many_batch_size: int = 1024       # pairs per cross-encoder forward in search_many
    stage3_many_packed_batch_size: int = 4096  # ... when the batch is packed (written-out forward on the GPU): no padding to pay
    mmr_lambda: Optional[float] = None       # None: off.  0 .. 1: the list stage 3 returns is diversified by maximal marginal
                                             # relevance (relevance = stage3_score, similarity from the stage-1 index)
    group_by: Any = None                     # None: off.  A metadata key or an integer array over the documents: stage 1
                                             # returns the stage1_top_k best GROUPS, at most group_size documents of each, so
    group_size: int = 1                      # stages 2 and 3 and the final list see no more of any group
    stage1_funnel_dims: Optional[int] = None     # None: off.  A multiple of 128 below stage 1's embedding dimension: its dense
                                                 # candidates are ranked on that prefix of the dimensions and a shortlist is
    stage1_funnel_fetch_k: Optional[int] = None  # rescored exactly; the shortlist, None: min(2048, max(8 k, 128))
    passage_window: Optional[int] = None     # None: off.  Tokens of the best passage every final record then carries
                                             # under "passage" (windowed MaxSim over the stage-2 tokens)
    stage1_boost: Any = None                 # None: off.  A boost spec (boost.py): stage 1's dense candidates are ranked by
                                             # score + a per-document bias, exactly


# (section, key) in the reference's YAML layout -> PipelineConfig field (reference :182-217)
_YAML_MAP = {
    ("stage1", "model"): "stage1_model", ("stage1", "top_k"): "stage1_top_k",
    ("stage1", "batch_size"): "stage1_batch_size", ("stage1", "enable_bm25"): "stage1_enable_bm25",
    ("stage1", "bm25_top_k"): "stage1_bm25_top_k", ("stage1", "fusion_method"): "stage1_fusion_method",
    ("stage1", "use_fp16"): "stage1_use_fp16", ("stage1", "index_dtype"): "stage1_index_dtype",
    ("stage2", "model"): "stage2_model", ("stage2", "top_k"): "stage2_top_k",
    ("stage2", "batch_size"): "stage2_batch_size", ("stage2", "max_seq_length"): "stage2_max_seq_length",
    ("stage2", "use_fp16"): "stage2_use_fp16", ("stage2", "scoring_method"): "stage2_scoring_method",
    ("stage3", "model"): "stage3_model", ("stage3", "top_k"): "stage3_top_k",
    ("stage3", "batch_size"): "stage3_batch_size", ("stage3", "max_length"): "stage3_max_length",
    ("stage3", "use_fp16"): "stage3_use_fp16",
}
_GENERAL_KEYS = ("device", "cache_dir", "index_dir", "log_level", "log_file", "enable_timing",
                 "save_intermediate_results", "auto_cleanup", "max_memory_usage_gb")


_NO_MMR = object()      # search(..., mmr_lambda=_NO_MMR): the plain search inside a diversified one
_ALL_RESULTS = 1 << 30  # top_k of that plain search: the whole list stage 3 returns
_NO_PASSAGES = object()  # search(..., passages=_NO_PASSAGES): the search inside one that adds passages


class RetrievalPipeline:
    """Stage 1 candidate generation -> stage 2 MaxSim rescoring -> stage 3 cross-encoder."""

    def __init__(self, config_path: Optional[str] = None, config: Optional[PipelineConfig] = None):
        self.logger = logging.getLogger(__name__)
        if config_path:
            self.config = self._load_config(config_path)
        elif config:
            self.config = config
        else:
            self.config = PipelineConfig()
        self._setup_logging()
        self.stage1: Optional[Stage1Retriever] = None
        self.stage2: Optional[ColBERTScorer] = None
        self.stage3: Optional[AdaptiveCrossEncoderReranker] = None
        self.performance_stats: Dict[str, Any] = {
            "total_queries": 0, "avg_stage1_time": 0.0, "avg_stage2_time": 0.0,
            "avg_stage3_time": 0.0, "avg_total_time": 0.0, "stage_time_history": []}
        self.logger.info("RetrievalPipeline initialized")

    # -- configuration -------------------------------------------------------
    def _load_config(self, config_path: str) -> PipelineConfig:
        """YAML with a top-level ``pipeline:`` mapping; nested stage sections as in the
        reference, or the flat field names that ``export_config`` writes."""
        try:
            with open(config_path, "r") as f:
                data = yaml.safe_load(f) or {}
            pd = data.get("pipeline", {}) or {}
            kw: Dict[str, Any] = {}
            names = {f.name for f in fields(PipelineConfig)}
            for k, v in pd.items():
                if k in names and not isinstance(v, dict):
                    kw[k] = v
            for (section, key), field_name in _YAML_MAP.items():
                sec = pd.get(section)
                if isinstance(sec, dict) and key in sec:
                    kw[field_name] = sec[key]
            for k in _GENERAL_KEYS:
                if k in pd:
                    kw[k] = pd[k]
            return PipelineConfig(**kw)
        except Exception as e:  # reference :219-221: fall back to defaults
            self.logger.error(f"Error loading config: {e}")
            return PipelineConfig()

    def _setup_logging(self) -> None:
        level = getattr(logging, str(self.config.log_level).upper(), logging.INFO)
        handlers: List[logging.Handler] = [logging.StreamHandler()]
        try:
            handlers.insert(0, logging.FileHandler(self.config.log_file))
        except OSError:
            pass
        logging.basicConfig(level=level, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s",
                            handlers=handlers)

    def initialize_stages(self) -> None:
        self.logger.info("Initializing pipeline stages...")
        c = self.config
        if c.tune_gemms:
            import torch
            if torch.cuda.is_available():
                if c.tune_gemms_file:
                    torch.cuda.tunable.set_filename(c.tune_gemms_file)
                torch.cuda.tunable.enable(True)
                torch.cuda.tunable.tuning_enable(True)
        try:
            self.stage1 = Stage1Retriever(Stage1Config(
                model_name=c.stage1_model, device=c.device, cache_dir=c.cache_dir, index_dir=c.index_dir,
                top_k_candidates=c.stage1_top_k, batch_size=c.stage1_batch_size,
                enable_bm25=c.stage1_enable_bm25, bm25_top_k=c.stage1_bm25_top_k,
                fusion_method=c.stage1_fusion_method, use_fp16=c.stage1_use_fp16,
                index_dtype=c.stage1_index_dtype, bm25_on_gpu=c.stage1_bm25_on_gpu,
                bm25_refit_compat=c.stage1_bm25_refit_compat, funnel_fetch_k=c.stage1_funnel_fetch_k,
                use_hip_graph=c.use_hip_graphs, index_batch_size=c.stage1_index_batch_size, amp_dtype=c.amp_dtype))
            self.logger.info("Stage 1 initialized")
            self.stage2 = ColBERTScorer(Stage2Config(
                model_name=c.stage2_model, device=c.device, cache_dir=c.cache_dir,
                max_seq_length=c.stage2_max_seq_length, batch_size=c.stage2_batch_size,
                top_k_candidates=c.stage2_top_k, use_fp16=c.stage2_use_fp16,
                scoring_method=c.stage2_scoring_method,
                cache_document_embeddings=c.stage2_cache_document_embeddings,
                precompute_document_embeddings=c.stage2_precompute_document_embeddings,
                token_store_dtype=c.stage2_token_store_dtype, passage_window=c.passage_window,
                use_hip_graph=c.use_hip_graphs, index_batch_size=c.stage2_index_batch_size, amp_dtype=c.amp_dtype))
            self.logger.info("Stage 2 initialized")
            self.stage3 = AdaptiveCrossEncoderReranker(Stage3Config(
                model_name=c.stage3_model, device=c.device, cache_dir=c.cache_dir,
                max_length=c.stage3_max_length, batch_size=c.stage3_batch_size,
                top_k_final=c.stage3_top_k, use_fp16=c.stage3_use_fp16, use_hip_graph=c.use_hip_graphs,
                many_batch_size=c.stage3_many_batch_size, amp_dtype=c.amp_dtype,
                many_width_multiple=c.stage3_width_multiple,
                many_packed_batch_size=max(c.stage3_many_batch_size, c.stage3_many_packed_batch_size)))
            self.logger.info("Stage 3 initialized")
        except Exception as e:
            self.logger.error(f"Error initializing pipeline stages: {e}")
            raise

    # -- indexing --------------------------------------------------------------
    def add_documents(self, documents: List[str], metadata: Optional[List[Dict[str, Any]]] = None):
        if not self.stage1:
            self.initialize_stages()
        self.logger.info(f"Adding {len(documents)} documents to pipeline")
        try:
            first_id = len(self.stage1.documents)
            self.stage1.add_documents(documents, metadata)
            if self.stage2 is not None and self.stage2.config.precompute_document_embeddings:
                self.stage2.index_documents(list(documents), first_id)
            if self.stage3 is not None and self.config.stage3_cache_document_tokens:
                self.stage3.index_documents(list(documents), first_id)
        except Exception as e:
            self.logger.error(f"Error adding documents: {e}")
            raise

    # -- removal -------------------------------------------------
    def remove_documents(self, doc_ids) -> int:
        """Removes documents by doc_id: no stage returns them again (stage 1 drops them from the dense search, BM25 and
        the fusion; stages 2 and 3 only see stage 1's candidates).  Their ids stay valid and their placeholders stay in
        the documents / metadata lists until :meth:`compact`.  Returns how many documents were removed."""
        if not self.stage1:
            self.initialize_stages()
        return self.stage1.remove_documents(doc_ids)

    def compact(self):
        """Drops the removed documents everywhere: the stage-1 index moves its live rows down on the GPU, BM25 is
        refitted on the survivors, the stage-2 token store and the stage-3 token-id cache move their live entries
        down in place.  Returns the old -> new doc_id map (numpy int64, -1 = removed; monotone)."""
        if not self.stage1:
            self.initialize_stages()
        old2new = self.stage1.compact()
        if self.stage2 is not None and hasattr(self.stage2, "compact_documents"):
            self.stage2.compact_documents(old2new)
        if self.stage3 is not None and hasattr(self.stage3, "compact_documents"):
            self.stage3.compact_documents(old2new)
        return old2new

    # -- update in place -------------------------------------------
    def update_documents(self, doc_ids, documents: List[str], metadata: Optional[List[Dict[str, Any]]] = None) -> int:
        """Replaces the documents ``doc_ids`` by ``documents`` (and, when given, their metadata) under the same
        doc_ids, in every stage: the stage-1 index rows are rewritten in place, BM25 is refitted, the stage-2 token
        rows are overwritten (or appended and repointed when the new text has more tokens) and the stage-3 token ids
        replaced.  All or nothing: an id out of range, given twice or removed raises ``ValueError`` before any stage
        is touched.  Returns how many documents were updated."""
        if not self.stage1:
            self.initialize_stages()
        ids = self.stage1.check_update(doc_ids, documents, metadata)
        if ids.size == 0:
            return 0
        documents = list(documents)
        n = self.stage1.update_documents(ids, documents, metadata)
        if self.stage2 is not None and self.stage2.config.precompute_document_embeddings:
            self.stage2.update_documents(ids.tolist(), documents)
        if self.stage3 is not None and self.config.stage3_cache_document_tokens:
            self.stage3.update_documents(ids.tolist(), documents)
        return n

    # -- search ----------------------------------------------------------------
    def _now(self) -> Optional[float]:
        return time.time() if self.config.enable_timing else None

    def _get_timing(self, enable_timing: bool) -> Optional[float]:
        return time.time() if enable_timing else None

    def _calculate_timing(self, total_start, stage1_time, stage2_time, stage3_time) -> Dict[str, float]:
        if not self.config.enable_timing:
            return {}
        total = time.time() - total_start if total_start else None
        return {"stage1_time": stage1_time or 0.0, "stage2_time": stage2_time or 0.0,
                "stage3_time": stage3_time or 0.0, "total_time": total or 0.0}

    def _run_later_stages(self, query: str, top_k: int, stage1_results, total_start, stage1_time):
        if not stage1_results:
            return {"query": query, "results": [], "stage1_results": [], "stage2_results": [],
                    "timing": self._calculate_timing(total_start, stage1_time, None, None),
                    "performance_stats": self.performance_stats}
        t = self._now()
        stage2_results = self.stage2.rescore_candidates(query, stage1_results)
        stage2_time = time.time() - t if t else None
        if not stage2_results:
            return {"query": query, "results": [], "stage1_results": stage1_results, "stage2_results": [],
                    "timing": self._calculate_timing(total_start, stage1_time, stage2_time, None),
                    "performance_stats": self.performance_stats}
        t = self._now()
        final = self.stage3.rerank(query, stage2_results)
        stage3_time = time.time() - t if t else None
        final = final[:top_k]
        total_time = time.time() - total_start if total_start else None
        if self.config.enable_timing:
            self._update_performance_stats(stage1_time, stage2_time, stage3_time, total_time)
        keep = self.config.save_intermediate_results
        result = {"query": query, "results": final,
                  "stage1_results": stage1_results if keep else [],
                  "stage2_results": stage2_results if keep else [],
                  "timing": self._calculate_timing(total_start, stage1_time, stage2_time, stage3_time),
                  "performance_stats": self.performance_stats.copy()}
        if self.config.auto_cleanup:
            self._cleanup_memory()
        return result

    # -- diversified results (MMR) -------------------------------
    def _mmr_lambda(self, mmr_lambda) -> Optional[float]:
        """The lambda of a search (the argument, else the config); None: no diversification."""
        if mmr_lambda is _NO_MMR:
            return None
        lam = self.config.mmr_lambda if mmr_lambda is None else mmr_lambda
        if lam is None:
            return None
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"mmr_lambda must be in [0, 1], got {mmr_lambda!r}")
        return lam

    def _group_kwargs(self, group_by, group_size, lam) -> Dict[str, Any]:
        """The grouping of a search as keyword arguments for stage 1 (the arguments, else the config); {}: off."""
        if group_by is None:
            group_by, group_size = self.config.group_by, self.config.group_size
        if group_by is None:
            return {}
        if lam is not None:
            raise ValueError("group_by cannot be combined with mmr_lambda: pick one way to thin out near-copies")
        if int(group_size) < 1:
            raise ValueError(f"group_size must be positive, got {group_size}")
        return {"group_by": group_by, "group_size": int(group_size)}

    def _funnel_kwargs(self, funnel_dims, lam, gkw) -> Dict[str, Any]:
        """The funnel of a search as a keyword argument for stage 1 (the argument, else the config); {}: off."""
        dims = self.config.stage1_funnel_dims if funnel_dims is None else funnel_dims
        if dims is None:
            return {}
        if lam is not None or gkw:
            raise ValueError("funnel_dims cannot be combined with mmr_lambda or group_by")
        return {"funnel_dims": int(dims)}

    def _boost_kwargs(self, boost, lam, gkw) -> Dict[str, Any]:
        """The boost of a search as a keyword argument for stage 1 (the argument, else the config); {}: off."""
        spec = self.config.stage1_boost if boost is None else boost
        if spec is None:
            return {}
        if lam is not None or gkw:
            raise ValueError("boost cannot be combined with mmr_lambda, group_by or funnel_dims")
        return {"boost": spec}

    def _diversify(self, outs: List[Dict[str, Any]], top_k: int, lam: float) -> List[Dict[str, Any]]:
        """``results`` of each output (the whole list stage 3 returned) -> its ``top_k`` picks by maximal marginal
        relevance, in selection order: relevance = stage3_score as f32, similarity = the inner product of the rows the
        stage-1 index stores (one ts_index_mmr call for the batch).  The records themselves are not changed."""
        index = self.stage1.faiss_index
        if not hasattr(index, "mmr"):
            raise NotImplementedError(f"{type(index).__name__} has no mmr()")
        lists = [o["results"] for o in outs]
        C = max((len(r) for r in lists), default=0)
        if C == 0:
            return outs
        from .index import mmr_check
        k, C, lam = mmr_check(min(int(top_k), C), C, lam)
        ids = np.full((len(lists), C), -1, dtype=np.int64)
        rel = np.zeros((len(lists), C), dtype=np.float32)
        for q, recs in enumerate(lists):
            ids[q, : len(recs)] = [int(r["doc_id"]) for r in recs]
            rel[q, : len(recs)] = [r["stage3_score"] for r in recs]
        _, picked = index.mmr(ids, rel, k, lam)
        picked = picked.cpu().numpy() if hasattr(picked, "cpu") else np.asarray(picked)
        for o, recs, row in zip(outs, lists, picked):
            by_id = {int(r["doc_id"]): r for r in recs}
            o["results"] = [by_id[int(i)] for i in row if int(i) >= 0]
        return outs

    # -- best passage per hit -------------------------------------
    def _passage_window(self, passages) -> Optional[int]:
        """The window of a search (the argument, else the config); None: no passages."""
        if passages is _NO_PASSAGES:
            return None
        w = self.config.passage_window if passages is None else passages
        if w is None:
            return None
        if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or w < 1:
            raise ValueError(f"passages must be a window of at least 1 token, got {passages!r}")
        return int(w)

    def _add_passages(self, outs: List[Dict[str, Any]], window: int) -> List[Dict[str, Any]]:
        """Every record of each output's ``results`` gains ``"passage"``: the window of ``window`` stage-2 token rows
        of the document that matches the query best (ColBERTScorer.best_passages: one kernel call for the batch,
        from the token store where every document has a slot, else from the re-encoded texts) and the text it covers.
        Nothing else of a record changes."""
        from .encoders import token_offsets
        lists = [o["results"] for o in outs]
        if not any(lists):
            return outs
        st2 = self.stage2
        ids = [[r.get("doc_id") for r in recs] for recs in lists]
        in_store = len(st2.token_store) and all(i in st2._store_slot for lst in ids for i in lst)
        docs = ids if in_store else [[r["document"] for r in recs] for recs in lists]
        found = st2.best_passages([o["query"] for o in outs], docs, window)
        L = st2.config.max_seq_length
        for recs, spans in zip(lists, found):
            for r, sp in zip(recs, spans):
                a, b = sp["token_start"], sp["token_end"]
                psg = {"token_start": a, "token_end": b, "score": sp["score"],
                       "char_start": None, "char_end": None, "text": None}
                doc = r["document"]
                blank = not doc or not doc.strip()       # stage 2 encodes such a document as "empty"
                off = token_offsets(st2.tokenizer, "empty" if blank else doc, L)
                if off is not None:
                    pieces = [x for x in off[0][a:b] if x != (0, 0)]      # (special tokens have no characters)
                    if blank or not pieces:
                        psg.update(char_start=0, char_end=0, text="")
                    else:
                        psg.update(char_start=pieces[0][0], char_end=pieces[-1][1],
                                   text=off[1][pieces[0][0]: pieces[-1][1]])
                r["passage"] = psg
        return outs

    def search(self, query: str, top_k: Optional[int] = None, filter=None, mmr_lambda=None,
               group_by=None, group_size: int = 1, passages=None, funnel_dims: Optional[int] = None,
               boost=None) -> Dict[str, Any]:
        """``filter``: search only the documents it allows (Stage1Retriever.filter_mask: a metadata dict, a
        callable, document indices or a bool array).  Stages 2 and 3 rescore stage 1's candidates, so fewer
        than ``top_k`` results come back when fewer documents are allowed, and none when none are.
        ``mmr_lambda`` (default: the config's, None = off): stages 1 to 3 run as without it, then ``top_k`` of the
        records stage 3 returned are picked by maximal marginal relevance (see :meth:`_diversify`) and come back in
        selection order with the keys and scores they have anyway.
        ``group_by`` / ``group_size`` (default: the config's, None = off): the collapse is applied at stage 1
        (Stage1Retriever.search), where ``stage1_top_k`` then counts groups: stages 2 and 3 see at most ``group_size``
        documents of any group, and so does the final list.  Dense-only and not together with ``mmr_lambda``:
        ``ValueError``.
        ``passages`` (an int window in tokens; default: the config's ``passage_window``, None = off): stages 1 to 3
        run as without it, then every record of the final list — after MMR or grouping if those are on — gains
        ``"passage": {"token_start", "token_end" (exclusive), "score", "char_start", "char_end", "text"}`` (see
        :meth:`_add_passages`; the character fields are None for a tokenizer without offsets).
        ``funnel_dims`` (default: the config's ``stage1_funnel_dims``, None = off): stage 1's dense candidates come from
        the funnel (Stage1Retriever.search); it replaces only that search, so ``filter`` and BM25 fusion work unchanged.
        Not together with ``mmr_lambda`` or ``group_by``: ``ValueError``.
        ``boost`` (default: the config's ``stage1_boost``, None = off): a boost spec (boost.py); stage 1's dense candidates
        are the documents with the largest score + bias (Stage1Retriever.search).  It replaces only that search, so
        ``filter`` and BM25 fusion work unchanged; stages 2 and 3 score as ever.  Stage 1 keeps the bias arrays of the
        last 4 specs; an array or a callable is one spec by IDENTITY: one changed in place has to be passed as a new
        object.  Not together with ``mmr_lambda``, ``group_by`` or ``funnel_dims``: ``ValueError``."""
        if not self.stage1 or not self.stage2 or not self.stage3:
            self.initialize_stages()
        pw = self._passage_window(passages)
        if pw is not None:
            return self._add_passages([self.search(query, top_k, filter=filter, mmr_lambda=mmr_lambda, group_by=group_by,
                                                   group_size=group_size, passages=_NO_PASSAGES,
                                                   funnel_dims=funnel_dims, boost=boost)], pw)[0]
        top_k = top_k or self.config.stage3_top_k
        lam = self._mmr_lambda(mmr_lambda)
        gkw = self._group_kwargs(group_by, group_size, lam)
        gkw.update(self._funnel_kwargs(funnel_dims, lam, gkw))
        gkw.update(self._boost_kwargs(boost, lam, gkw))
        if lam is not None:
            return self._diversify([self.search(query, _ALL_RESULTS, filter=filter, mmr_lambda=_NO_MMR,
                                                passages=_NO_PASSAGES)], top_k, lam)[0]
        if self.config.search_on_arrays and filter is None:
            # one query through the array path of search_many (resident token store + stage-3 id cache): no candidate
            # text is tokenised or re-encoded, one cross-encoder forward for the query's pairs; same records (tests)
            fast = self._search_many_arrays([query], top_k, **gkw)
            if fast is not None:
                return fast[0]
        total_start = self._now()
        try:
            t = self._now()
            if filter is None:
                stage1_results = self.stage1.search(query, self.config.stage1_top_k, **gkw)
            else:
                stage1_results = self.stage1.search(query, self.config.stage1_top_k, filter=filter, **gkw)
            stage1_time = time.time() - t if t else None
            return self._run_later_stages(query, top_k, stage1_results, total_start, stage1_time)
        except Exception as e:
            self.logger.error(f"Error during search: {e}")
            raise

    def batch_search(self, queries: List[str], top_k: Optional[int] = None, filter=None,
                     mmr_lambda=None, group_by=None, group_size: int = 1, passages=None,
                     funnel_dims: Optional[int] = None, boost=None) -> List[Dict[str, Any]]:
        """Sequential, like the reference (:444-448); see search_many for the batched form.  ``filter``: one
        filter for every query or a list with one per query.  ``mmr_lambda``, ``group_by`` / ``group_size``: as for
        :meth:`search`.  ``passages``: as for :meth:`search`, one kernel call for the batch.  ``funnel_dims``, ``boost``:
        as for :meth:`search`."""
        if passages is not _NO_PASSAGES:
            if not self.stage2:
                self.initialize_stages()
            pw = self._passage_window(passages)
            if pw is not None:
                return self._add_passages(self.batch_search(queries, top_k, filter=filter, mmr_lambda=mmr_lambda,
                                                            group_by=group_by, group_size=group_size,
                                                            passages=_NO_PASSAGES, funnel_dims=funnel_dims,
                                                            boost=boost), pw)
        gkw = {} if group_by is None else {"group_by": group_by, "group_size": group_size}
        gkw["passages"] = _NO_PASSAGES
        if funnel_dims is not None:
            gkw["funnel_dims"] = funnel_dims
        if boost is not None:
            gkw["boost"] = boost
        if filter is None:
            if mmr_lambda is None:
                return [self.search(q, top_k, **gkw) for q in queries]
            return [self.search(q, top_k, mmr_lambda=mmr_lambda, **gkw) for q in queries]
        if not self.stage1:
            self.initialize_stages()
        specs = self.stage1._per_query_filters(filter, len(queries))
        return [self.search(q, top_k, filter=f, mmr_lambda=mmr_lambda, **gkw) for q, f in zip(queries, specs)]

    def search_many(self, queries: List[str], top_k: Optional[int] = None, filter=None,
                    mmr_lambda=None, group_by=None, group_size: int = 1, passages=None,
                    funnel_dims: Optional[int] = None, boost=None) -> List[Dict[str, Any]]:
        """Same result records as batch_search, every stage batched over the queries: one
        bi-encoder pass and one sweep of the corpus per 64 queries (stage 1), one query forward
        and one MaxSim launch (stage 2, with the resident token store), one length-sorted pass
        of the cross-encoder over all (query, candidate) pairs (stage 3).  Stage times are
        reported as equal shares of the batch's stage times.  ``filter``: one filter for every query or a list
        with one per query (see :meth:`search`); a filtered batch takes the record path.  ``group_by`` /
        ``group_size``: as for :meth:`search`, one collapse for the batch.  ``passages``: as for :meth:`search`, one
        kernel call for the batch.  ``funnel_dims``: as for :meth:`search`, one funnel for the batch.
        ``boost``: as for :meth:`search`, one bias for the batch."""
        if not self.stage1 or not self.stage2 or not self.stage3:
            self.initialize_stages()
        pw = self._passage_window(passages)
        if pw is not None:
            return self._add_passages(self.search_many(queries, top_k, filter=filter, mmr_lambda=mmr_lambda,
                                                       group_by=group_by, group_size=group_size,
                                                       passages=_NO_PASSAGES, funnel_dims=funnel_dims, boost=boost), pw)
        top_k = top_k or self.config.stage3_top_k
        if not queries:
            return []
        lam = self._mmr_lambda(mmr_lambda)
        gkw = self._group_kwargs(group_by, group_size, lam)
        gkw.update(self._funnel_kwargs(funnel_dims, lam, gkw))
        gkw.update(self._boost_kwargs(boost, lam, gkw))
        if lam is not None:   # (mmr_lambda: as for search(); one selection call for the batch)
            return self._diversify(self.search_many(queries, _ALL_RESULTS, filter=filter, mmr_lambda=_NO_MMR,
                                                    passages=_NO_PASSAGES), top_k, lam)
        queries = list(queries)
        n = len(queries)
        # a batch builds ~n x stage1_top_k candidate records; the cyclic collector would rescan
        # them on every allocation burst (measured: a list comprehension over 6400 pairs took 69 ms)
        import gc
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            if filter is None:
                fast = self._search_many_arrays(queries, top_k, **gkw)
                if fast is not None:
                    return fast
            total_start = self._now()
            t = self._now()
            if filter is None:
                s1 = self.stage1.search_many(queries, self.config.stage1_top_k, **gkw)
            else:
                s1 = self.stage1.search_many(queries, self.config.stage1_top_k, filter=filter, **gkw)
            t1 = (time.time() - t) / n if t else None
            s2, s3, t2, t3 = self._later_stages_many(queries, s1)
            total = (time.time() - total_start) / n if total_start else None
            return self._assemble_many(queries, top_k, s1, s2, s3, t1, t2, t3, total)
        finally:
            if gc_was_on:
                gc.enable()

    def _search_many_arrays(self, queries: List[str], top_k: int, **group) -> Optional[List[Dict[str, Any]]]:
        """search_many with every stage on ARRAYS (the candidate sets never become Python records): stage 1
        returns id / score matrices, stage 2 looks the candidates up in the resident token store and keeps the
        best by one stable device sort, stage 3 assembles its (query, document) inputs from cached token ids on
        the GPU; dictionaries are built only for what is returned (all three lists with
        ``save_intermediate_results``, else the final top_k per query).  Same records as the per-record path
        (tests).  None when a precondition is missing (HIP index on the device path, complete token store,
        complete stage-3 id cache, at least stage1_top_k documents) — the caller then takes the record path."""
        if not self._arrays_ready():
            return None
        n = len(queries)
        m0 = self._tick()
        # what the later stages need from the QUERIES alone is started first: the stage-2 query forward runs beside
        # stage 1's sweep of the corpus, stage 3's query tokens are ready when its pairs are assembled
        for st in (self.stage2, self.stage3):
            if hasattr(st, "prefetch_queries"):
                st.prefetch_queries(queries)
        mp = self._tick()
        got = self._arrays_stage1(queries, **group)
        if got is None:
            return None
        ids1_dev, sc1 = got
        m1 = self._tick()
        later = self._arrays_stage23(queries, ids1_dev)
        if later is None:
            return None
        pos2_h, sc2_h, pos3_h, sc3_h, t2s, t3s = later       # (the host has waited for the GPU in there: marks are complete)
        t1 = self._span(mp, m1)
        t1 = t1 / n if t1 is not None else None
        pre = self._span(m0, mp)                              # the prefetched query work belongs to stages 2 / 3
        t2 = (t2s + (pre or 0.0)) / n if t2s is not None else None
        t3 = t3s / n if t3s is not None else None
        ids1_h = ids1_dev.cpu().numpy()
        sc1_h = sc1.cpu().numpy() if hasattr(sc1, "cpu") else sc1
        total = (time.time() - m0[0]) / n if m0 is not None else None
        return self._records_from_arrays(queries, top_k, ids1_h, sc1_h, pos2_h, sc2_h, pos3_h, sc3_h, t1, t2, t3, total)

    def _tick(self):
        """A stage boundary of the array path: (host time, HIP event recorded on the current stream) — NOT a
        synchronisation.  Round 2 synchronised the device at every boundary (six times per search): correct stage
        times, but the GPU drained six times per query and `search()` paid 1.5 ms of its 5.5 ms for it.  The stage
        times are now the GPU-side intervals between the events, read after the call's results have been copied
        out (`_span`); the total stays wall-clock."""
        if not self.config.enable_timing:
            return None
        import torch
        ev = None
        if torch.cuda.is_available():
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
        return (time.time(), ev)

    @staticmethod
    def _span(a, b) -> Optional[float]:
        """Seconds between two _tick() marks (device time when both carry an event, else host time)."""
        if a is None or b is None:
            return None
        if a[1] is not None and b[1] is not None:
            b[1].synchronize()
            return a[1].elapsed_time(b[1]) / 1e3
        return b[0] - a[0]

    def _arrays_ready(self) -> bool:
        s1, s2, s3 = self.stage1, self.stage2, self.stage3
        return bool(getattr(s2, "token_store", None) is not None and len(s2.token_store)
                    and getattr(s3, "_pairs_usable", False) and hasattr(s1, "search_many_arrays"))

    def _arrays_stage1(self, queries: List[str], **group):
        """-> (ids int64 [B, k] on the token store's device, scores [B, k] tensor or numpy) or None.  ``group``:
        group_by / group_size of a grouped search (k is then stage1_top_k * group_size)."""
        import torch
        got = self.stage1.search_many_arrays(queries, self.config.stage1_top_k, **group)
        if got is None:
            return None
        ids1, sc1 = got
        dev = self.stage2.token_store.data.device
        ids1_dev = ids1.to(dev) if torch.is_tensor(ids1) else torch.from_numpy(ids1).to(dev)
        return ids1_dev, sc1

    def _arrays_stage23(self, queries: List[str], ids1_dev):
        """Stages 2 and 3 of `queries` (row i of ids1_dev = the stage-1 ids of queries[i]) ->
        (pos2, sc2, pos3, sc3 as host arrays, stage-2 seconds, stage-3 seconds) or None."""
        import torch
        ma = self._tick()
        r2 = self.stage2.rescore_arrays(queries, ids1_dev, lazy=True)
        if r2 is None:
            return None
        pos2, sc2, bad2 = r2
        ids2_dev = torch.gather(ids1_dev.to(pos2.device), 1, pos2)
        mb = self._tick()
        r3 = self.stage3.rerank_arrays(queries, ids2_dev, lazy=True)
        if r3 is None:
            return None
        pos3, sc3, bad3 = r3
        mc = self._tick()
        out = (pos2.cpu().numpy(), sc2.cpu().numpy(), pos3.cpu().numpy(), sc3.cpu().numpy())
        if bool(bad2) or bool(bad3):     # a candidate outside the token store / id cache (looked at only now: the copies
            return None                  # above were the first time the host waited for the GPU since stage 3's batch plan)
        return out + (self._span(ma, mb), self._span(mb, mc))

    def _records_from_arrays(self, queries, top_k, ids1_h, sc1_h, pos2_h, sc2_h, pos3_h, sc3_h, t1, t2, t3, total):
        s1 = self.stage1
        n = len(queries)
        docs, meta = s1.documents, s1.doc_metadata
        keep = self.config.save_intermediate_results

        def rec1(q, j):
            i = int(ids1_h[q, j])
            s = float(sc1_h[q, j])
            return {"doc_id": i, "document": docs[i], "score": s, "stage1_score": s, "metadata": meta[i],
                    "stage": "stage1"}

        def rec2(q, j):
            r = rec1(q, int(pos2_h[q, j]))
            r["stage2_score"] = float(sc2_h[q, j])
            r["stage"] = "stage2"
            return r

        def rec3(q, j):
            r = rec2(q, int(pos3_h[q, j]))
            r["stage3_score"] = float(sc3_h[q, j])
            r["stage"] = "stage3"
            return r
        out1 = [[rec1(q, j) for j in range(ids1_h.shape[1])] if keep else None for q in range(n)]
        out2 = [[rec2(q, j) for j in range(pos2_h.shape[1])] if keep else None for q in range(n)]
        out3 = [[rec3(q, j) for j in range(pos3_h.shape[1])] for q in range(n)]
        if not keep:   # _assemble_many only tests the lists of a non-empty stage for truth
            out1 = [[True]] * n
            out2 = [[True]] * n
        return self._assemble_many(queries, top_k, out1, out2, out3, t1, t2, t3, total)

    def _later_stages_many(self, queries, s1):
        """Stages 2 and 3 for several queries -> (stage-2 lists, stage-3 lists, per-query time shares)."""
        n = max(len(queries), 1)
        t = self._now()
        s2 = self.stage2.rescore_many(queries, s1)
        t2 = (time.time() - t) / n if t else None
        t = self._now()
        s3 = self.stage3.rerank_many(queries, s2)
        t3 = (time.time() - t) / n if t else None
        return s2, s3, t2, t3

    def _assemble_many(self, queries, top_k, s1, s2, s3, t1, t2, t3, total):
        keep = self.config.save_intermediate_results
        out = []
        for q, r1, r2, r3 in zip(queries, s1, s2, s3):
            if not r1 or not r2:   # the reference's early returns (:363-371, :380-388)
                out.append({"query": q, "results": [], "stage1_results": r1 if r1 else [], "stage2_results": [],
                            "timing": ({"stage1_time": t1 or 0.0, "stage2_time": (t2 or 0.0) if r1 else 0.0,
                                        "stage3_time": 0.0, "total_time": total or 0.0}
                                       if self.config.enable_timing else {}),
                            "performance_stats": self.performance_stats})
                continue
            if self.config.enable_timing:
                self._update_performance_stats(t1, t2, t3, total)
            out.append({"query": q, "results": r3[:top_k],
                        "stage1_results": r1 if keep else [], "stage2_results": r2 if keep else [],
                        "timing": ({"stage1_time": t1 or 0.0, "stage2_time": t2 or 0.0, "stage3_time": t3 or 0.0,
                                    "total_time": total or 0.0} if self.config.enable_timing else {}),
                        "performance_stats": self.performance_stats.copy()})
        if self.config.auto_cleanup:
            self._cleanup_memory()
        return out

    # -- persistence -------------------------------------------------------------
    def save_index(self, index_path: Optional[str] = None):
        if not self.stage1:
            raise ValueError("Pipeline not initialized")
        if index_path is None:
            index_path = os.path.join(self.config.index_dir, "pipeline_index.pkl")
        self.stage1.save_index(index_path)
        if self.stage2 is not None and self.stage2.config.precompute_document_embeddings:
            self.stage2.save_token_store(self._token_store_path(index_path))
        self.logger.info(f"Pipeline index saved to {index_path}")

    @staticmethod
    def _token_store_path(index_path: str) -> str:
        return os.path.splitext(index_path)[0] + ".stage2_tokens.safetensors"

    def load_index(self, index_path: Optional[str] = None):
        if not self.stage1:
            self.initialize_stages()
        if index_path is None:
            index_path = os.path.join(self.config.index_dir, "pipeline_index.pkl")
        self.stage1.load_index(index_path)
        if self.stage2 is not None and self.stage2.config.precompute_document_embeddings and self.stage1.documents:
            # the resident stage-2 token store comes back from its file, or is re-encoded
            if not self.stage2.load_token_store(self._token_store_path(index_path), len(self.stage1.documents)):
                self.stage2.reset_token_store()
                self.stage2.index_documents(list(self.stage1.documents), 0)
        if self.stage3 is not None and self.config.stage3_cache_document_tokens and self.stage1.documents:
            self.stage3._pairs = None     # token ids are cheap to recompute: no file of their own
            self.stage3.index_documents(list(self.stage1.documents), 0)
        self.logger.info(f"Pipeline index loaded from {index_path}")

    # -- introspection -----------------------------------------------------------
    def _config_dict(self) -> Dict[str, Any]:
        """The configuration as plain data: a boost spec that is an array or a callable is named, not dumped."""
        d = asdict(self.config)
        b = self.config.stage1_boost
        if b is not None and not isinstance(b, dict):
            d["stage1_boost"] = (f"<callable {getattr(b, '__name__', type(b).__name__)}>" if callable(b)
                                 else f"<array of {len(b)} biases>")
        return d

    def get_pipeline_info(self) -> Dict[str, Any]:
        info = {"config": self._config_dict(),
                "stages_initialized": {"stage1": self.stage1 is not None, "stage2": self.stage2 is not None,
                                       "stage3": self.stage3 is not None},
                "performance_stats": self.performance_stats}
        if self.stage1:
            info["stage1_stats"] = self.stage1.get_stats()
            info["documents"] = {"total": len(self.stage1.documents), "removed": self.stage1.n_removed,
                                 "live": len(self.stage1.documents) - self.stage1.n_removed}
        if self.stage2:
            info["stage2_info"] = self.stage2.get_model_info()
            info["stage2_token_store_dtype"] = info["stage2_info"].get("token_store_dtype")
        if self.stage3:
            info["stage3_info"] = self.stage3.get_model_info()
        return info

    def _update_performance_stats(self, stage1_time, stage2_time, stage3_time, total_time):
        """Cumulative mean with alpha = 1/n and a 100-entry history (reference :567-606)."""
        ps = self.performance_stats
        ps["total_queries"] += 1
        alpha = 1.0 / ps["total_queries"]
        for key, val in (("avg_stage1_time", stage1_time), ("avg_stage2_time", stage2_time),
                         ("avg_stage3_time", stage3_time), ("avg_total_time", total_time)):
            ps[key] = (1 - alpha) * ps[key] + alpha * val
        ps["stage_time_history"].append({"stage1": stage1_time, "stage2": stage2_time,
                                         "stage3": stage3_time, "total": total_time})
        if len(ps["stage_time_history"]) > 100:
            ps["stage_time_history"] = ps["stage_time_history"][-100:]

    def _cleanup_memory(self):
        try:
            if self.stage2:
                self.stage2.clear_gpu_memory()
            if self.stage3:
                self.stage3.clear_gpu_memory()
        except Exception as e:
            self.logger.warning(f"Error during memory cleanup: {e}")

    def export_config(self, config_path: str):
        with open(config_path, "w") as f:
            yaml.dump({"pipeline": self._config_dict()}, f, default_flow_style=False)
        self.logger.info(f"Configuration exported to {config_path}")
