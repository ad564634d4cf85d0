"""Row-sharded stage-1 index: one process per GPU, RCCL all-gather of partial top-k.

The reference has no multi-device path at all (no
torch.distributed, batch_search is a sequential loop at
src/retrieval_pipeline.py:444-448); this is the scale-out BASELINE.json's
north_star specifies for the same `faiss_index.search` call
(src/stage1_retriever.py:380):

  * the corpus matrix is split row-wise and contiguously: rank r of R holds rows
    [r*ceil(N/R), min(N, (r+1)*ceil(N/R)))  and reports global ids (local row +
    offset) straight from the kernel;
  * every rank scans its shard for the full query batch (queries are replicated,
    64 x 768 fp16 = 96 KiB);
  * ONE collective per batch: an all-gather of each rank's packed partial result
    (B*k*(4+8) bytes, 768 KB at B=64, k=1000).  xGMI is point-to-point, so this is
    a direct peer exchange, latency-bound and far below the shard scan time; no
    ring all-reduce anywhere;
  * each rank merges the R sorted lists with the HIP select kernel
    (ts_merge_topk), so every rank ends with the identical global top-k, in the
    canonical (score desc, id asc) order — the result does not depend on R.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np


def shard_bounds(n_total: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Rows [lo, hi) held by `rank`; contiguous, ceil-divided."""
    per = -(-int(n_total) // int(world_size)) if n_total > 0 else 0
    lo = min(n_total, rank * per)
    hi = min(n_total, lo + per)
    return lo, hi


class ShardedFlatIPIndex:
    """FAISS-shaped index over R row shards (this process owns one of them).

    ``local_index`` is a tristage_rag_amd.index.FlatIPIndex on this rank's GPU;
    ``merge_fn(scores[R,B,k], ids[R,B,k]) -> (D[B,k], I[B,k])`` defaults to the
    HIP merge kernel.  Both are attributes so the process-group plumbing can be
    exercised on CPU (gloo) with stand-ins in tests.
    """

    def __init__(self, d: int, n_total: int, dtype: str = "f16", device: Optional[int] = None,
                 group=None, local_index=None, merge_fn: Optional[Callable] = None):
        import torch.distributed as dist
        self._dist = dist
        self.group = group
        self.world_size = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.d = int(d)
        self.n_total = int(n_total)
        self.lo, self.hi = shard_bounds(self.n_total, self.world_size, self.rank)
        if str(dtype) in ("fp8", "e4m3", "float8_e4m3fn") or getattr(local_index, "storage_dtype", None) == "fp8":
            raise NotImplementedError("ShardedFlatIPIndex does not take an fp8 index (fp8 storage is single-GPU, flat only)")
        if str(dtype) in ("fp4", "mxfp4", "e2m1") or getattr(local_index, "storage_dtype", None) == "fp4":
            raise NotImplementedError("ShardedFlatIPIndex does not take an fp4 index (fp4 storage is single-GPU, flat only)")
        if local_index is None:
            from .index import FlatIPIndex
            local_index = FlatIPIndex(d, dtype=dtype, device=0 if device is None else device)
            local_index.reserve(max(self.hi - self.lo, 1))
        self.local_index = local_index
        self.local_index.set_id_offset(self.lo)
        if hasattr(self.local_index, "auto_finish"):
            # this wrapper owns the finish() cadence: a finish that repairs a batch must be followed
            # by a repeat of that batch's exchange on EVERY rank, so it has to be the collective one
            self.local_index.auto_finish = False
        if hasattr(self.local_index, "coalesce"):
            # the local result is all-gathered in stream order before finish(): a held scan would feed the exchange
            # buffers that are not written yet (TS_FLAG_COALESCE is never set here)
            self.local_index.coalesce = False
        self.merge_packed_fn = None
        if merge_fn is None:
            from .index import merge_topk, merge_topk_packed
            merge_fn = merge_topk
            self.merge_packed_fn = merge_topk_packed   # reads the all-gather buffer in place
        self.merge_fn = merge_fn
        self._pending = []
        self._pending_passes = 0      # scan passes of the pending batches, counted HERE so every rank counts alike
        self.always_exchange = False  # tests: run the collective + merge even for one rank

    # -- FAISS duck type ----------------------------------------------------
    @property
    def ntotal(self) -> int:
        return self.n_total

    def add_local(self, rows) -> None:
        """Append rows of THIS rank's shard (in shard order)."""
        self.local_index.add(rows)
        if self.local_index.ntotal > self.hi - self.lo:
            raise ValueError("more rows added than this rank's shard holds")

    def add_global(self, rows) -> None:
        """Every rank passes the same full matrix; each keeps its own slice."""
        if rows.shape[0] != self.n_total:
            raise ValueError(f"expected {self.n_total} rows, got {rows.shape[0]}")
        self.local_index.add(rows[self.lo:self.hi])

    def remove_ids(self, ids) -> int:
        raise NotImplementedError("removal is not supported on a row-sharded index")

    def compact(self):
        raise NotImplementedError("removal is not supported on a row-sharded index")

    def range_search(self, q, radius, allowed=None, max_results=None, sort: bool = False):
        raise NotImplementedError("range search is not supported on a row-sharded index")

    def mmr(self, ids, relevance, k: int, lambda_mult: float = 0.5):
        raise NotImplementedError("MMR is not supported on a row-sharded index (the candidates' rows live on several ranks)")

    def search_mmr(self, q, k: int, fetch_k=None, lambda_mult: float = 0.5, allowed=None):
        raise NotImplementedError("MMR is not supported on a row-sharded index (the candidates' rows live on several ranks)")

    def search_grouped(self, q, k: int, groups, group_size: int = 1, fetch_k=None, allowed=None):
        raise NotImplementedError("grouped search is not supported on a row-sharded index (the collapse needs the merged list)")

    def search_prefix(self, q, k: int, dims: int, allowed=None):
        raise NotImplementedError("funnel search is not supported on a row-sharded index")

    def rescore(self, q, ids, k=None):
        raise NotImplementedError("funnel search is not supported on a row-sharded index (the candidates' rows live on several ranks)")

    def search_funnel(self, q, k: int, dims: int, fetch_k=None, allowed=None):
        raise NotImplementedError("funnel search is not supported on a row-sharded index")

    def search_biased(self, q, k: int, bias, allowed=None, exact_dense: bool = False, check_finite: bool = True):
        raise NotImplementedError("boosted search (search_biased) is not supported on a row-sharded index")

    def search(self, q, k: int, async_: bool = False, inputs_ready: bool = False, allowed=None):
        """Global top-k for the replicated query batch `q` (tensor).  Returns
        tensors (D float32 [B,k], I int64 [B,k]) identical on every rank.

        ``async_=True``: local search, all-gather and merge are only enqueued (all
        three are stream-ordered); call :meth:`finish` before reading the result.
        ``allowed`` (filtered search) is not supported on the sharded index."""
        if allowed is not None:
            raise NotImplementedError("filtered search (allowed=) is not supported by ShardedFlatIPIndex; "
                                      "use a single FlatIPIndex")
        import torch
        if not torch.is_tensor(q):  # FAISS-style numpy call: same path, numpy back
            D, I = self.search(torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)), k)
            return D.cpu().numpy(), I.cpu().numpy()
        dev = self._index_device()
        if dev is not None and not q.is_cuda:
            # host queries with the HIP index underneath: the exchange buffer the local search
            # writes into lives on the index's GPU, so the queries go there first
            q = q.to(dev)
        B = q.shape[0]
        # finish() is COLLECTIVE, so its cadence must follow state that is identical on every rank: the batches seen
        # by this wrapper.  (Round 2 asked the local index for room — but a rank with an empty shard, e.g. 17 rows
        # on 8 ranks, never searches locally, never ran out of room, and met the others' all_reduce with its next
        # all_gather: a hang after ~30 batches.)  PENDING_PASSES passes of <= 32 queries is the local index's own limit,
        # which it can only reach later than this count does.  A finish() drains the pipeline (0.7 ms at 2.5 M rows per
        # rank, tools/sessions/r03_outlier.sh): every 120 batches, not every 30 as in round 2.
        passes = (B + 31) // 32
        limit = int(getattr(self.local_index, "PENDING_PASSES", 60))
        if async_ and self._pending_passes and (len(self._pending) >= 120 or self._pending_passes + passes > limit):
            self.finish()
        # the local result is produced directly inside the buffer that is exchanged:
        # [float32 scores | pad to 8 | int64 ids], no packing kernels
        from .index import packed_layout
        ids_at, _ = packed_layout(B, k)
        packed = self._packed_buffer(B, k, q.device)
        D = packed[: 4 * B * k].view(torch.float32).view(B, k)
        I = packed[ids_at:].view(torch.int64).view(B, k)
        if self.hi > self.lo:
            if getattr(self.local_index, "supports_out", False):
                self.local_index.search(q, k, async_=async_, out=(D, I), inputs_ready=inputs_ready and async_)
            else:
                d, i = self.local_index.search(q, k)
                D.copy_(torch.as_tensor(d))
                I.copy_(torch.as_tensor(i))
        else:  # an empty shard contributes only padding
            D.fill_(-3.4028234663852886e38)
            I.fill_(-1)
        if async_:
            self._pending_passes += passes
        if self.world_size == 1 and not self.always_exchange:
            return D, I
        out = self._exchange_and_merge(packed, B, k)
        if async_:
            self._pending.append((q, k, packed, out))
        return out

    def _host_staged(self) -> bool:
        return self._dist.is_initialized() and self._dist.get_backend(self.group) == "gloo"

    def _index_device(self):
        """torch device of the local HIP index (None for a stand-in index without one)."""
        if getattr(self.local_index, "supports_out", False) and hasattr(self.local_index, "device"):
            import torch
            return torch.device("cuda", int(self.local_index.device))
        return None

    def _packed_buffer(self, B: int, k: int, device):
        import torch
        from .index import packed_layout
        ids_at, nbytes = packed_layout(B, k)
        buf = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        if ids_at != 4 * B * k:
            buf[4 * B * k: ids_at] = 0     # the padding travels through the all-gather: keep it defined
        return buf

    def _exchange_and_merge(self, packed, B: int, k: int):
        """ONE collective (all-gather of the packed partial results) + the merge kernel,
        which reads the gathered buffer in place."""
        import torch
        if packed.is_cuda and self._host_staged():
            # a gloo group (tests: several ranks sharing one GPU) cannot move device memory:
            # the same exchange through host copies
            host = torch.empty((self.world_size * packed.numel(),), dtype=torch.uint8)
            self._dist.all_gather_into_tensor(host, packed.cpu(), group=self.group)
            flat = host.to(packed.device)
        else:
            flat = torch.empty((self.world_size * packed.numel(),), dtype=torch.uint8, device=packed.device)
            self._dist.all_gather_into_tensor(flat, packed, group=self.group)  # 1-D: gloo and RCCL both take it
        if self.merge_packed_fn is not None:
            return self.merge_packed_fn(flat, self.world_size, B, k)
        from .index import packed_layout
        ns, ids_at = 4 * B * k, packed_layout(B, k)[0]
        blocks = flat.view(self.world_size, packed.numel())
        Dg = blocks[:, :ns].contiguous().view(torch.float32).reshape(self.world_size, B, k)
        Ig = blocks[:, ids_at:].contiguous().view(torch.int64).reshape(self.world_size, B, k)
        return self.merge_fn(Dg, Ig)

    def finish(self):
        """Complete asynchronous searches on every rank.  If ANY rank had to repeat a
        local search, all ranks repeat the exchange for that batch (collectively)."""
        import torch
        redone_local = set(self.local_index.finish()) if hasattr(self.local_index, "finish") else set()
        if (self.world_size == 1 and not self.always_exchange) or not self._pending:
            self._pending.clear()
            self._pending_passes = 0
            return
        # the i-th pending entry of every rank is the same batch; local tickets are
        # consecutive, so "repeated" maps to positions from the end
        last = self._last_ticket()
        flags = torch.zeros(len(self._pending), dtype=torch.int32, device=self._pending[0][2].device)
        for t in redone_local:
            pos = len(self._pending) - 1 - (last - t)
            if 0 <= pos < len(self._pending):
                flags[pos] = 1
        if flags.is_cuda and self._host_staged():
            hf = flags.cpu()
            self._dist.all_reduce(hf, op=self._dist.ReduceOp.MAX, group=self.group)
            flags = hf
        else:
            self._dist.all_reduce(flags, op=self._dist.ReduceOp.MAX, group=self.group)
        for pos in torch.nonzero(flags).flatten().tolist():
            q, k, packed, out = self._pending[pos]   # packed was corrected in place by local finish()
            Dn, In = self._exchange_and_merge(packed, q.shape[0], k)
            out[0].copy_(Dn)
            out[1].copy_(In)
        torch.cuda.current_stream().synchronize() if flags.is_cuda else None
        self._pending.clear()
        self._pending_passes = 0

    def _last_ticket(self) -> int:
        li = self.local_index
        return int(li._lib.ts_index_last_ticket(li._h)) if hasattr(li, "_lib") else -1
