"""Shared by the tests of the query-stationary coalesced passes (test_qstat_gpu.py, test_stream_order_of_qstat_gpu.py):
read-only corpora, an index with the pass policies set, held batches run to finish(), and the number of filter scans a
run launched."""
import functools

from helpers import make_corpus

N_SHORT = 33_001    # just above the filter path's floor: 1 032 row blocks, 4 or 5 steps per workgroup on 256 CUs (the
                    # ring holds 2.5 to 3 row blocks), and the last block holds 9 rows
N_LONG = 100_003    # walks several rings long


def tq(torch, a, dtype):
    t = torch.tensor(a).cuda()   # (a copy: the shared corpora are read-only arrays)
    return t.half() if dtype == "f16" else t.bfloat16()


@functools.lru_cache(maxsize=2)
def corpus_of(n, d, dtype, seed=7):
    c = make_corpus(n, d, seed=seed, dtype=dtype)
    c.setflags(write=False)
    return c


def index_of(torch, d, dtype, n=N_LONG, stat=True, wide="auto", corpus=None):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=dtype)
    idx.add(tq(torch, corpus_of(n, d, dtype) if corpus is None else corpus, dtype))
    idx.classic_filter = True
    idx.stationary_passes = stat
    idx.wide_passes = wide
    return idx


def batches_of(torch, d, dtype, sizes, ks, seed):
    if isinstance(ks, int):
        ks = (ks,) * len(sizes)
    return [(tq(torch, make_corpus(b, d, seed=seed + i, dtype=dtype), dtype), k) for i, (b, k) in enumerate(zip(sizes, ks))]


def run(torch, idx, batches, coalesce):
    idx.coalesce = coalesce
    outs = [idx.search(q, k, async_=True) for q, k in batches]
    redone = idx.finish()
    torch.cuda.synchronize()
    return outs, redone


def same(torch, a, b):
    assert len(a) == len(b)
    for (D, I), (D0, I0) in zip(a, b):
        assert torch.equal(I, I0) and torch.equal(D, D0)


def sync_search(idx, batches):
    return [idx.search(q, k) for q, k in batches]


def scan_launches(torch, idx, batches, coalesce=True):
    """The results of the held batches and the number of filter scans they took."""
    idx.set_profiling(True, every=1)
    idx.timings(reset=True)
    outs, redone = run(torch, idx, batches, coalesce)
    n = idx.timings(reset=True)["filter_scan"][1]
    idx.set_profiling(False)
    assert redone == []
    return outs, n
