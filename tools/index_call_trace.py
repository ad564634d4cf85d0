"""The library calls behind every public method of FlatIPIndex / IVFFlatIndex, recorded: each index's ``_lib`` is
wrapped in a proxy that logs the entry name of every call and, by ``_lib.SIGNATURES``, each argument — the value of an
integer / float parameter, "null" / "ptr" for a ``c_void_p`` one, nothing for a by-reference output.  The walk calls
every method with numpy, CPU-tensor and CUDA-tensor inputs where it takes them, and also records the container types of
what comes back and the type and text of what is raised.  Only public methods, ``ix._lib`` and ``_lib.SIGNATURES`` are
used, so one file runs on any two trees whose binding should make the same calls.  The comparison holds the two traces
equal entry for entry, except that calls of the read-only getters (GETTERS: how often a method reads ``ntotal`` is not
part of its contract) are counted, not compared; every array that came back must be ``array_equal`` too (the arrays go
to an .npz beside the trace, which is not kept).  d = 256, f16 storage, 16416 rows, k = 10, dims = 128; a few seconds.

  python tools/index_call_trace.py --out a.json --npz a.npz                (in each tree)
  python tools/index_call_trace.py --compare a.json b.json --npz-compare a.npz b.npz --verdict verdict.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, D, K, DIMS, BIG_K, NB = 16416, 256, 10, 128, 16385, 130


class Recorder:
    """Stands where an index keeps the loaded library; every call goes through and is logged first."""

    def __init__(self, lib, signatures, log):
        self._lib, self._sig, self._log = lib, signatures, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._sig:
            return fn
        argtypes = self._sig[name][1]

        def call(*args):
            rec = [name]
            for a, t in zip(args, argtypes):
                if t is ctypes.c_void_p:
                    v = a.value if hasattr(a, "value") else a
                    rec.append("ptr" if v else "null")
                elif t is ctypes.c_float or t is ctypes.c_double:
                    rec.append(float(a))
                elif t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32):
                    rec.append(int(a))
                # anything else is POINTER(...): a by-reference output
            self._log.append(rec)
            return fn(*args)
        return call


class Walk:
    def __init__(self):
        self.log, self.arrays, self.sections = [], {}, 0

    def wrap(self, ix):
        from tristage_rag_amd import _lib
        ix._lib = Recorder(ix._lib, _lib.SIGNATURES, self.log)
        return ix

    def _flat(self, label, r):
        """The container types of a result; its arrays go to ``self.arrays``."""
        if isinstance(r, (tuple, list)):
            return [self._flat(f"{label}.{i}", x) for i, x in enumerate(r)]
        if isinstance(r, dict):
            return {k: self._flat(f"{label}.{k}", v) for k, v in sorted(r.items())}
        if hasattr(r, "data_ptr"):
            self.arrays[label] = r.detach().cpu().numpy()
            return f"tensor:{r.device.type}:{str(r.dtype)}"
        if isinstance(r, np.ndarray):
            self.arrays[label] = r.copy()
            return f"ndarray:{r.dtype}"
        return r if r is None or isinstance(r, (bool, int, float, str)) else repr(r)

    def __call__(self, label, fn):
        self.sections += 1
        self.log.append(["#", label])
        label = f"{self.sections:04d}_{label}"   # (array names: unique whatever the labels are)
        try:
            r = fn()
        except Exception as e:   # the type and the text are part of the contract
            self.log.append(["!raise", type(e).__name__, str(e)])
            return None
        self.log.append(["=", self._flat(label, r)])
        return r


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def forms(torch, x):
    """One [B, d] float32 array in every documented input form."""
    return {"np32": x, "np16": x.astype(np.float16), "np64": x.astype(np.float64), "npF": np.asfortranarray(x),
            "cpu32": torch.from_numpy(x), "cpu16": torch.from_numpy(x).half(), "cpubf16": torch.from_numpy(x).bfloat16(),
            "cuda32": torch.from_numpy(x).cuda(), "cuda16": torch.from_numpy(x).cuda().half(),
            "cudaT": torch.from_numpy(np.ascontiguousarray(x.T)).cuda().half().t()}


def walk_flat(w, torch):
    from tristage_rag_amd.index import FlatIPIndex
    rng = np.random.default_rng(7)
    rows = unit(rng, N, D)
    q5 = forms(torch, unit(rng, 5, D))
    qbig = torch.from_numpy(unit(rng, NB, D)).cuda().half()
    bad = {"np": np.zeros((3, D + 1), np.float32), "np1d": np.zeros(D, np.float32),
           "cuda": torch.zeros((3, D + 1), device="cuda"), "cpu": torch.zeros((3, D + 1))}

    empty = w.wrap(FlatIPIndex(D, dtype="f16"))
    for f in ("np32", "cuda16"):
        w(f"empty.search.{f}", lambda: empty.search(q5[f], K))
        w(f"empty.filtered.{f}", lambda: empty.search(q5[f], K, allowed=np.ones(0, bool)))
        w(f"empty.range.{f}", lambda: empty.range_search(q5[f], 0.1))
        w(f"empty.scores.{f}", lambda: empty.scores(q5[f]))
        w(f"empty.prefix.{f}", lambda: empty.search_prefix(q5[f], K, DIMS))
        w(f"empty.rescore.{f}", lambda: empty.rescore(q5[f], np.zeros((5, 4), np.int64)))
        w(f"empty.funnel.{f}", lambda: empty.search_funnel(q5[f], K, DIMS))
    empty.close()

    ix = w.wrap(FlatIPIndex(D, dtype="f16"))
    third = N // 3
    w("add.np32", lambda: ix.add(rows[:third]))
    w("add.cpu", lambda: ix.add(torch.from_numpy(rows[third: 2 * third])))
    w("add.cuda16", lambda: ix.add(torch.from_numpy(rows[2 * third:]).cuda().half(), normalize=True))
    for f, x in bad.items():
        w(f"add.bad.{f}", lambda: ix.add(x))
    w("ntotal", lambda: ix.ntotal)

    for f, q in q5.items():
        w(f"search.{f}", lambda: ix.search(q, K))
    for f in ("np32", "cuda16"):
        w(f"search.exact_dense.{f}", lambda: ix.search(q5[f], K, exact_dense=True))
        w(f"search.classic.{f}", lambda: ix.search(q5[f], K, classic=True))
        w(f"search.one_launch.{f}", lambda: ix.search(q5[f], K, one_launch=True))
    for f, x in bad.items():
        w(f"search.bad.{f}", lambda: ix.search(x, K))
    w("search.bad.k", lambda: ix.search(q5["np32"], 0))
    w("search.async.np", lambda: ix.search(q5["np32"], K, async_=True))

    def out_pair(B, k=K, dt=torch.float32, it=torch.int64):
        return (torch.empty((B, k), dtype=dt, device="cuda"), torch.empty((B, k), dtype=it, device="cuda"))
    w("search.out", lambda: ix.search(q5["cuda16"], K, out=out_pair(5)))
    w("search.out.bad_shape", lambda: ix.search(q5["cuda16"], K, out=out_pair(4)))
    w("search.out.bad_dtype", lambda: ix.search(q5["cuda16"], K, out=out_pair(5, it=torch.int32)))
    w("search.out.bad_stride", lambda: ix.search(q5["cuda16"], K, out=tuple(t[:, ::2] for t in out_pair(5, 2 * K))))

    def after(r, fin=True):   # asynchronous results are complete after finish()
        if fin:
            red = ix.finish()
        torch.cuda.synchronize()
        return (r, red) if fin else r
    w("search.async", lambda: after(ix.search(q5["cuda16"], K, async_=True)))
    w("search.async.ready", lambda: after(ix.search(q5["cuda16"], K, async_=True, inputs_ready=True)))
    w("search.async.out", lambda: after(ix.search(q5["cuda16"], K, async_=True, out=out_pair(5))))
    w("search.async.130", lambda: after(ix.search(qbig, K, async_=True)))
    w("search.async.130.flush", lambda: (ix.search(qbig, K, async_=True), ix.flush(), ix.finish())[::2])
    w("search.async.130.out", lambda: after(ix.search(qbig, K, async_=True, out=out_pair(NB), classic=True)))
    ix.coalesce = False
    w("search.async.no_coalesce", lambda: after(ix.search(q5["cuda16"], K, async_=True)))
    ix.coalesce, ix.wide_passes = True, False
    w("search.async.no_wide", lambda: after(ix.search(q5["cuda16"], K, async_=True)))
    ix.wide_passes = "auto"
    w("search_in_stream_order", lambda: after(ix.search_in_stream_order(q5["cuda16"], K)))
    w("last_search_info", ix.last_search_info)

    # -- allowed, in every form ----------------------------------------------------------------------------------
    m = rng.random(N) < 0.3
    m2 = rng.random(N) < 0.05
    m2d = rng.random((5, N)) < 0.2
    words = (N + 31) // 32
    packed = np.zeros(words * 4, np.uint8)
    pb = np.packbits(m, bitorder="little")
    packed[: pb.shape[0]] = pb
    packed = packed.view(np.uint32)
    pk_cuda = torch.from_numpy(packed.view(np.int32)).cuda()
    pk2_cuda = torch.from_numpy(np.ascontiguousarray(packed[::-1]).view(np.int32)).cuda()
    allowed = {"bool": m, "list": [m, None, m, m2, None], "2d": m2d, "2d_tensor": torch.from_numpy(m2d),
               "bool_tensor": torch.from_numpy(m).cuda(), "packed_np": packed, "packed_cuda": pk_cuda,
               "packed_cuda_list": [pk_cuda, None, pk2_cuda, pk_cuda, None], "all_none": [None] * 5,
               "mixed_list": [pk_cuda, m, None, m, pk_cuda]}
    for a, al in allowed.items():
        for f in ("np32", "cpu16", "cuda16"):
            w(f"filtered.{a}.{f}", lambda: ix.search(q5[f], K, allowed=al))
        w(f"filtered.{a}.info", ix.last_filter_info)
    w("filtered.exact_dense", lambda: ix.search(q5["cuda16"], K, allowed=m, exact_dense=True))
    w("filtered.out", lambda: ix.search(q5["cuda16"], K, allowed=m, out=out_pair(5)))
    w("filtered.out.bad", lambda: ix.search(q5["cuda16"], K, allowed=m, out=out_pair(4)))
    w("filtered.bad.count", lambda: ix.search(q5["np32"], K, allowed=[m, m2, m, m2]))
    w("filtered.bad.len", lambda: ix.search(q5["np32"], K, allowed=m[:-1]))
    w("filtered.bad.dtype", lambda: ix.search(q5["np32"], K, allowed=m.astype(np.float32)))
    for f, x in bad.items():
        if f != "np1d":
            w(f"filtered.bad.{f}", lambda: ix.search(x, K, allowed=m))
    w("filtered.async.np", lambda: ix.search(q5["np32"], K, allowed=m, async_=True))
    w("filtered.async", lambda: after(ix.search(q5["cuda16"], K, allowed=m, async_=True)))
    w("filtered.async.packed", lambda: after(ix.search(q5["cuda16"], K, allowed=pk_cuda, async_=True)))
    w("filtered.async.130", lambda: after(ix.search(qbig, K, allowed=m, async_=True)))
    per_query = [(m, None, m2)[i % 3] for i in range(NB)]
    w("filtered.async.130.list", lambda: after(ix.search(qbig, K, allowed=per_query, async_=True)))
    w("filtered.async.130.packed", lambda: after(ix.search(qbig, K, allowed=pk_cuda, async_=True, out=out_pair(NB))))
    w("filtered.async.130.2d", lambda: after(ix.search(qbig, K, allowed=rng.random((NB, N)) < 0.5, async_=True)))
    w("filtered.async.info", ix.last_filter_info)

    # -- k beyond the select limit -------------------------------------------------------------------------------
    for f in ("np32", "cpu16", "cuda16"):
        w(f"large_k.{f}", lambda: ix.search(q5[f], BIG_K))
        w(f"large_k.masked.{f}", lambda: ix.search(q5[f], BIG_K, allowed=m))
    w("large_k.list", lambda: ix.search(q5["cuda16"], BIG_K, allowed=allowed["list"]))
    w("large_k.packed_cuda", lambda: ix.search(q5["cuda16"], BIG_K, allowed=pk_cuda))
    w("large_k.out", lambda: ix.search(q5["cuda16"], BIG_K, out=out_pair(5, BIG_K)))
    w("large_k.bad", lambda: ix.search(bad["cuda"], BIG_K))

    # -- range search, scores ------------------------------------------------------------------------------------
    for f in ("np32", "np16", "cpu16", "cuda16", "cuda32"):
        w(f"range.{f}", lambda: ix.range_search(q5[f], 0.15))
        w(f"range.allowed.{f}", lambda: ix.range_search(q5[f], 0.1, allowed=m, sort=True))
        w(f"scores.{f}", lambda: ix.scores(q5[f]))
    for a in ("list", "2d", "packed_cuda", "packed_cuda_list", "all_none"):
        w(f"range.{a}.np", lambda: ix.range_search(q5["np32"], 0.1, allowed=allowed[a]))
        w(f"range.{a}.cuda", lambda: ix.range_search(q5["cuda16"], 0.1, allowed=allowed[a]))
    w("range.radii", lambda: ix.range_search(q5["cuda16"], np.linspace(0.1, 0.2, 5), exact_dense=True))
    w("range.limit", lambda: ix.range_search(q5["np32"], -1.0, max_results=100))
    w("range.info", ix.last_range_info)
    for f, x in bad.items():
        w(f"range.bad.{f}", lambda: ix.range_search(x, 0.1))
        w(f"scores.bad.{f}", lambda: ix.scores(x))
    w("scores.np64", lambda: ix.scores(q5["np64"]))

    # -- funnel --------------------------------------------------------------------------------------------------
    cand_np = rng.integers(0, N, size=(5, 64)).astype(np.int64)
    cand_np[:, -3:] = -1
    for f in ("np32", "np16", "np64", "cpu32", "cpu16", "cuda16", "cuda32"):
        w(f"prefix.{f}", lambda: ix.search_prefix(q5[f], K, DIMS))
        w(f"prefix.allowed.{f}", lambda: ix.search_prefix(q5[f], K, DIMS, allowed=m))
        w(f"rescore.{f}", lambda: ix.rescore(q5[f], cand_np))
        w(f"rescore.cuda_ids.{f}", lambda: ix.rescore(q5[f], torch.from_numpy(cand_np).cuda(), K))
        w(f"funnel.{f}", lambda: ix.search_funnel(q5[f], K, DIMS))
        w(f"funnel.allowed.{f}", lambda: ix.search_funnel(q5[f], K, DIMS, allowed=m))
    for a in ("list", "2d", "packed_cuda", "packed_cuda_list", "all_none"):
        w(f"prefix.{a}.np", lambda: ix.search_prefix(q5["np32"], K, DIMS, allowed=allowed[a]))
        w(f"prefix.{a}.cuda", lambda: ix.search_prefix(q5["cuda16"], K, DIMS, allowed=allowed[a], exact_dense=True))
    w("funnel.info", ix.last_funnel_info)
    for f in ("np", "cuda"):
        w(f"prefix.bad.{f}", lambda: ix.search_prefix(bad[f], K, DIMS))
        w(f"rescore.bad.{f}", lambda: ix.rescore(bad[f], cand_np[:3]))
        w(f"funnel.bad.{f}", lambda: ix.search_funnel(bad[f], K, DIMS))
    w("prefix.bad.dims", lambda: ix.search_prefix(q5["np32"], K, 100))

    # -- MMR, groups ---------------------------------------------------------------------------------------------
    groups = (np.arange(N) % 97).astype(np.int32)
    for f in ("np32", "cpu16", "cuda16"):
        Dq, Iq = ix.search(q5[f], 40)
        w(f"mmr.{f}", lambda: ix.mmr(Iq, Dq, K, 0.3))
        w(f"search_mmr.{f}", lambda: ix.search_mmr(q5[f], K))
        w(f"search_mmr.allowed.{f}", lambda: ix.search_mmr(q5[f], K, fetch_k=32, lambda_mult=0.7, allowed=m))
        w(f"search_grouped.{f}", lambda: ix.search_grouped(q5[f], K, groups))
        w(f"search_grouped.info.{f}", ix.last_group_info)
        w(f"search_grouped.size2.{f}", lambda: ix.search_grouped(q5[f], 4, groups, group_size=2, fetch_k=16, allowed=m))
    w("mmr.cpu_tensors", lambda: ix.mmr(torch.from_numpy(Iq.cpu().numpy()), torch.from_numpy(Dq.cpu().numpy()), K))
    w("mmr.bad.shape", lambda: ix.mmr(Iq, Dq[:, :-1], K))
    w("mmr.bad.k", lambda: ix.mmr(Iq, Dq, 41))
    w("mmr.bad.id", lambda: ix.mmr(np.full((2, 4), N + 5, np.int64), np.zeros((2, 4), np.float32), 2))
    w("search_grouped.bad", lambda: ix.search_grouped(q5["np32"], K, groups[:-1]))

    # -- mutation ------------------------------------------------------------------------------------------------
    new = unit(rng, 4, D)
    w("update.np", lambda: ix.update_rows([1, 5, 9, 13], new))
    w("update.np16", lambda: ix.update_rows(np.array([2, 6, 10, 14]), new.astype(np.float16), normalize=True))
    w("update.cpu", lambda: ix.update_rows(torch.tensor([3, 7, 11, 15]), torch.from_numpy(new)))
    w("update.cuda", lambda: ix.update_rows(torch.tensor([4, 8, 12, 16]).cuda(), torch.from_numpy(new).cuda().half()))
    w("update.pending", lambda: (ix.search(q5["cuda16"], K, async_=True), ix.update_rows([20, 21, 22, 23], new))[0])
    w("update.bad.id", lambda: ix.update_rows([1, 1, 2, N], new))
    w("update.bad.shape", lambda: ix.update_rows([1, 2, 3], new))
    w("update.bad.width", lambda: ix.update_rows([1, 2, 3], torch.zeros((3, D + 1), device="cuda")))
    w("remove.np", lambda: ix.remove_ids(np.arange(0, 200, 2)))
    w("remove.list", lambda: ix.remove_ids([1, 3, 3, N + 7]))
    w("remove.cuda", lambda: ix.remove_ids(torch.arange(300, 340).cuda()))
    w("remove.pending", lambda: (ix.search(q5["cuda16"], K, async_=True), ix.remove_ids([500]))[::-1])
    w("nlive", lambda: ix.nlive)
    w("live_mask", ix.live_mask)
    w("removed.search", lambda: ix.search(q5["cuda16"], K))
    w("removed.filtered", lambda: ix.search(q5["np32"], K, allowed=m))
    w("removed.large_k", lambda: ix.search(q5["cuda16"], BIG_K))
    w("removed.large_k.masked", lambda: ix.search(q5["np32"], BIG_K, allowed=[m, None, m, m2, None]))
    w("removed.range", lambda: ix.range_search(q5["cuda16"], 0.15, allowed=pk_cuda))
    w("compact.pending", lambda: (ix.search(q5["cuda16"], K, async_=True), ix.compact())[::-1])
    w("compact.search", lambda: ix.search(q5["np32"], K))
    w("reconstruct_n", lambda: ix.reconstruct_n(3, 4))
    w("set_id_offset", lambda: ix.set_id_offset(1000))
    w("offset.search", lambda: ix.search(q5["cuda16"], K))
    w("read_probe.keys", lambda: sorted(ix.read_probe(1)))
    w("reset", ix.reset)
    ix.close()


def walk_ivf(w, torch):
    from tristage_rag_amd.index import IVFFlatIndex
    rng = np.random.default_rng(11)
    rows = unit(rng, 4096, D)
    q5 = forms(torch, unit(rng, 5, D))
    bad = {"np": np.zeros((3, D + 1), np.float32), "cuda": torch.zeros((3, D + 1), device="cuda")}
    iv = w.wrap(IVFFlatIndex(D, 16, dtype="f16", nprobe=4))
    w("ivf.add.untrained", lambda: iv.add(rows[:8]))
    w("ivf.train.bad", lambda: iv.train(bad["np"]))
    w("ivf.train.few", lambda: iv.train(rows[:8]))
    w("ivf.train", lambda: iv.train(rows[:2048], seed=3, niter=5))
    w("ivf.search.empty", lambda: iv.search(q5["np32"], K))
    w("ivf.add.np32", lambda: iv.add(rows[:1500]))
    w("ivf.add.np64", lambda: iv.add(rows[1500:2000].astype(np.float64)))
    w("ivf.add.cpu16", lambda: iv.add(torch.from_numpy(rows[2000:3000]).half()))
    w("ivf.add.cuda", lambda: iv.add(torch.from_numpy(rows[3000:]).cuda(), normalize=True))
    w("ivf.add.bad", lambda: iv.add(bad["cuda"]))
    w("ivf.list_sizes", iv.list_sizes)
    w("ivf.centroids", lambda: iv.centroids)
    for f, q in q5.items():
        w(f"ivf.probe.{f}", lambda: iv.probe(q))
        w(f"ivf.search.{f}", lambda: iv.search(q, K))
    w("ivf.search.nprobe", lambda: iv.search(q5["cuda16"], K, nprobe=16, async_=True))
    w("ivf.search.out", lambda: iv.search(q5["cuda16"], K, out=(torch.empty((5, K), device="cuda"),
                                                               torch.empty((5, K), dtype=torch.int64, device="cuda"))))
    w("ivf.search.out.bad", lambda: iv.search(q5["cuda16"], K, out=(torch.empty((4, K), device="cuda"),
                                                                   torch.empty((4, K), dtype=torch.int64, device="cuda"))))
    for f, x in bad.items():
        w(f"ivf.search.bad.{f}", lambda: iv.search(x, K))
        w(f"ivf.probe.bad.{f}", lambda: iv.probe(x))
    groups = (np.arange(4096) % 31).astype(np.int32)
    for f in ("np32", "cpu16", "cuda16"):
        Dq, Iq = iv.search(q5[f], 24)
        w(f"ivf.mmr.{f}", lambda: iv.mmr(Iq, Dq, K, 0.4))
        w(f"ivf.search_mmr.{f}", lambda: iv.search_mmr(q5[f], K, nprobe=8))
        w(f"ivf.search_grouped.{f}", lambda: iv.search_grouped(q5[f], 5, groups, nprobe=8))
        w(f"ivf.search_grouped.info.{f}", iv.last_group_info)
    new = unit(rng, 3, D)
    w("ivf.update.np", lambda: iv.update_rows([1, 5, 9], new))
    w("ivf.update.cuda", lambda: iv.update_rows(torch.tensor([2, 6, 10]).cuda(), torch.from_numpy(new).cuda().half(), normalize=True))
    w("ivf.update.bad.id", lambda: iv.update_rows([1, 1, 4096], new))
    w("ivf.update.bad.shape", lambda: iv.update_rows([1, 2], new))
    w("ivf.remove.np", lambda: iv.remove_ids(np.arange(0, 100, 2)))
    w("ivf.remove.cuda", lambda: iv.remove_ids(torch.arange(200, 210).cuda()))
    w("ivf.nlive", lambda: iv.nlive)
    w("ivf.removed.search", lambda: iv.search(q5["np32"], K))
    w("ivf.compact", iv.compact)
    w("ivf.reconstruct_n", lambda: iv.reconstruct_n(2, 4))
    w("ivf.compact.search", lambda: iv.search(q5["cuda16"], K))
    w("ivf.last_search_info", iv.last_search_info)
    w("ivf.finish", lambda: (iv.finish(), iv.flush()))
    w("ivf.reset", iv.reset)
    iv.close()


def record(out, npz):
    import torch
    w = Walk()
    walk_flat(w, torch)
    walk_ivf(w, torch)
    torch.cuda.synchronize()
    for path in (out, npz):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(w.log, f)
    np.savez(npz, **w.arrays)
    calls = sum(1 for r in w.log if r[0][0] not in "#!=")
    print(json.dumps({"sections": sum(1 for r in w.log if r[0] == "#"), "library_calls": calls,
                      "raised": sum(1 for r in w.log if r[0] == "!raise"), "arrays": len(w.arrays)}))


# read-only getters: they launch nothing and change nothing, so how often a method reads one is not part of its contract
GETTERS = ("ts_index_ntotal", "ts_index_live_count", "ts_ivf_ntotal", "ts_ivf_is_trained")


def compare(a_path, b_path, npz_pair, verdict_path):
    full_a, full_b = json.load(open(a_path)), json.load(open(b_path))
    a, b = ([r for r in t if r[0] not in GETTERS] for t in (full_a, full_b))
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
    verdict = {"what": "tools/index_call_trace.py on the parent tree (before) and on this tree (after): every library call "
                       "with its scalar arguments and null / non-null pointers, result container types and raised "
                       "errors, section by section ('#')",
               "getters_not_compared": list(GETTERS),
               "getter_calls_before": len(full_a) - len(a), "getter_calls_after": len(full_b) - len(b),
               "entries_before": len(a), "entries_after": len(b), "traces_equal": a == b, "first_difference": first}
    if first is not None:
        verdict["difference"] = {"before": a[first: first + 3], "after": b[first: first + 3],
                                 "section": next((r[1] for r in reversed(a[: first + 1]) if r[0] == "#"), None)}
    if npz_pair:
        x, y = np.load(npz_pair[0]), np.load(npz_pair[1])
        differ = sorted(k for k in set(x.files) | set(y.files)
                        if k not in x.files or k not in y.files or x[k].dtype != y[k].dtype
                        or not np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == "f"))
        verdict.update(arrays_compared=len(set(x.files) | set(y.files)), arrays_differing=differ,
                       arrays_equal=not differ)
    verdict["before"], verdict["after"] = full_a, full_b
    with open(verdict_path, "w") as f:
        json.dump(verdict, f, indent=None, separators=(",", ":"))
    print(json.dumps({k: v for k, v in verdict.items() if k not in ("before", "after")}))
    return 0 if verdict["traces_equal"] and verdict.get("arrays_equal", True) else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="gpu_jobs/index_call_trace.json")
    ap.add_argument("--npz", default="gpu_jobs/index_call_trace.npz")
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"))
    ap.add_argument("--npz-compare", nargs=2, metavar=("BEFORE", "AFTER"))
    ap.add_argument("--verdict", default="profiles/index_call_trace_before_after.json")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.npz_compare, args.verdict))
    record(args.out, args.npz)
