"""remove_ids / update_rows / add / compact of FlatIPIndex and IVFFlatIndex on the GPU, held to the exact host model
of tests/mutation_model.py.  After every mutating op the index is compared with the model on ntotal,
nlive, the live mask, the value the op returned, the whole of reconstruct_n bit for bit, and a search (ids and score
bits).  Inputs are integers in [-63, 63], so there is no tolerance anywhere: every comparison is np.array_equal.

The kernels under test: live_set / live_clear, word_count / tile_scan / word_scan / compact_map / compact_gather
(ts_remove.hip), upd_block / upd_rows / upd_live_check and the IVF placement (ts_update.hip), ivfc_classify / tables /
move (ts_ivf_compact.hip), the add / remove kernels of ts_ivf.hip and the host drivers of ts_index.hip.

Measured on the MI355X: see DESIGN.md 4.14 (the whole file, and test_flat_large on its own)."""
import functools

import numpy as np
import pytest

import exact_inputs as xi
import mutation_model as mm
from mutation_model import HOLE_PATTERNS, SIZES, UPDATE_SETS, IndexModel

pytestmark = pytest.mark.gpu

FLAT = [("f16", 40), ("bf16", 128), ("f32", 96)]
B = 5
KS = (1, 50)


@functools.lru_cache(maxsize=8)
def rows(n, d, seed=0):
    x = mm.rows_for(n, d, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=8)
def queries(d):
    return mm.queries_for(B, d, seed=4242)


def dev(x, storage):
    """Rows on the device in the storage type (exact: the values are small integers)."""
    import torch
    t = torch.from_numpy(np.array(x)).cuda()          # (a copy: the cached inputs are read-only)
    return t.to({"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[storage])


def flat_index(d, storage, offset=0):
    from tristage_rag_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, dtype=storage)
    if offset:
        idx.set_id_offset(offset)
    return idx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_state(idx, m, what):
    assert idx.ntotal == m.ntotal, what
    assert idx.nlive == m.nlive, what
    if hasattr(idx, "live_mask"):
        assert np.array_equal(idx.live_mask(), m.live), what
    else:
        assert int(idx.list_sizes().sum()) == m.nlive, what
    assert same_bits(idx.reconstruct_n(), m.rows), what      # removed rows keep their content until compact


def check_search(idx, m, what, allowed=None, **kw):
    """k = 50 and k = 1 against the model (whose top 1 is the first column of its top 50)."""
    q = queries(m.d)
    if m.ntotal == 0:
        with pytest.raises(ValueError):
            idx.search(q, 1, **kw)
        return
    Dm, Im = m.expected_topk(q, max(KS), allowed=allowed)
    for k in KS:
        D, I = idx.search(q, k, **kw)
        D, I = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in (D, I))
        assert np.array_equal(I, Im[:, :k]), (what, k, kw)
        assert same_bits(D, Dm[:, :k]), (what, k, kw)


def check(idx, m, what, modes=False):
    check_state(idx, m, what)
    check_search(idx, m, what)
    if modes and m.ntotal > mm.FILTER_FLOOR:
        check_search(idx, m, what, classic=True)
        check_search(idx, m, what, one_launch=True)


# ------------------------------------------------------------------------------------------ flat: pattern x size
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(HOLE_PATTERNS))
@pytest.mark.parametrize("storage,d", FLAT)
def test_flat_pattern(storage, d, name, n):
    """remove, compact, add 50 rows: the last checks the cleared padding of the last new block."""
    x = rows(n, d)
    idx, m = flat_index(d, storage), IndexModel(d)
    idx.add(x)
    m.add(x)
    ids = HOLE_PATTERNS[name](n)
    assert idx.remove_ids(ids) == m.remove(ids) == ids.size
    check(idx, m, "remove", modes=True)
    assert np.array_equal(idx.compact(), m.compact())
    check(idx, m, "compact", modes=True)
    extra = rows(50, d, seed=9)
    idx.add(extra)
    m.add(extra)
    check(idx, m, "add")
    idx.close()


@pytest.mark.parametrize("storage,d", FLAT)
def test_flat_add_at_a_partial_word_and_bitmap_growth_under_tombstones(storage, d):
    """live_set_kernel's live[w] | bits (an add at a row that is no multiple of 32 while tombstones exist), live_reserve
    growing the bitmap with its content kept, and the bitmap's re-initialisation at the first removal after a compact,
    which leaves the old holes in it."""
    x = rows(3000, d)
    idx, m = flat_index(d, storage), IndexModel(d)
    idx.add(x[:77])
    m.add(x[:77])
    gone = np.array([0, 31, 64, 70, 76])
    assert idx.remove_ids(gone) == m.remove(gone) == 5
    at = 77
    for count in (1, 18, 32, 1000, 1872):        # 77 -> 78 -> 96 (a word border) -> 128 -> 1128 -> 3000: the bitmap grows
        idx.add(dev(x[at:at + count], storage))
        m.add(x[at:at + count])
        at += count
        check(idx, m, f"add {count}")
        last = np.array([at - 1, 5])             # the row just added and an old one
        assert idx.remove_ids(last) == m.remove(last)
        check_state(idx, m, f"remove after add {count}")
    assert np.array_equal(idx.compact(), m.compact())
    check(idx, m, "compact")
    # the first removal after a compact: the stale holes of the bitmap must not come back
    idx.add(x[:100])
    m.add(x[:100])
    one = np.array([m.ntotal - 1])
    assert idx.remove_ids(one) == m.remove(one) == 1
    check(idx, m, "first removal after compact")
    assert np.array_equal(idx.compact(), m.compact())
    assert np.array_equal(idx.compact(), m.compact())          # twice: the identity
    check(idx, m, "compact twice")
    idx.close()


# -------------------------------------------------------------------------------------------- flat: update sets
UPD = FLAT + [("f16", 1024)]      # the last: float32 host rows, whose staging chunk is the smaller one


def _update_chunk(storage, d):
    return mm.update_chunk_rows(d, storage, host_elem_bytes=4 if d == 1024 else None)


UPD_CASES = [(st, d, name) for st, d in UPD for name in sorted(UPDATE_SETS)] + [("f16", 1024, "20000_ids")]


@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("storage,d,name", UPD_CASES)
def test_flat_update_set(storage, d, name, tombstones):
    host = d == 1024
    chunk = _update_chunk(storage, d)
    rng = np.random.default_rng(len(name) + d)
    if name == "20000_ids":     # host rows only: 20 000 ids cross the 16 384-row host chunk
        assert chunk < 20_000 < 2 * chunk
        n = 20_011
        ids = rng.permutation(n)[:20_000].astype(np.int64)
    else:
        n = mm.update_rows_needed(name, chunk) + 3
        ids = UPDATE_SETS[name](n, chunk, rng)
    x = rows(n + 40, d)
    idx, m = flat_index(d, storage), IndexModel(d)
    idx.add(x)
    m.add(x)
    if tombstones:    # rows the call does not name: the last 40 and every seventh of the others
        dead = np.union1d(np.arange(n, n + 40), np.setdiff1d(np.arange(0, n, 7), ids))
        assert idx.remove_ids(dead) == m.remove(dead)
    y = rows(ids.size, d, seed=17)
    idx.update_rows(ids, y if host else dev(y, storage))
    m.update(ids, y)
    check(idx, m, name)
    idx.close()


@pytest.mark.parametrize("storage,d", FLAT)
def test_flat_update_refused_calls_write_nothing(storage, d):
    n = 1061
    x = rows(n, d)
    idx, m = flat_index(d, storage, offset=500), IndexModel(d, offset=500)
    idx.add(x)
    m.add(x)
    dead = np.array([40, 41, 900]) + 500
    assert idx.remove_ids(dead) == m.remove(dead) == 3
    good = np.random.default_rng(1).permutation(np.setdiff1d(np.arange(n), [40, 41, 900]))[:300] + 500
    y = rows(301, d, seed=3)
    for bad in (n + 500, 499, int(good[7]), 900 + 500):     # beyond the end, below the offset, given twice, removed
        ids = np.concatenate([good, [bad]])
        with pytest.raises(ValueError):
            m.update(ids, y)
        with pytest.raises(ValueError):
            idx.update_rows(ids, dev(y, storage))
        with pytest.raises(ValueError):
            idx.update_rows(ids, y)
        check_state(idx, m, f"refused {bad}")
    idx.update_rows(good, dev(y[:300], storage))
    m.update(good, y[:300])
    check(idx, m, "accepted")
    idx.close()


# ------------------------------------------------------------------------- flat: several compaction chunks, small
def test_flat_compaction_moves_rows_across_a_staging_chunk_border():
    """f32 storage at d = 1024 has 128 KiB row blocks, so 65 536 rows fill the staging buffer of ts_compact_corpus; of
    100 000 rows more than that survive, and rows move across the chunk border."""
    d, n = 1024, 100_000
    chunk = mm.compact_chunk_rows(d, "f32")
    idx, m = flat_index(d, "f32"), IndexModel(d)
    for i in range(10):
        part = mm.rows_for(n // 10, d, seed=100 + i)
        idx.add(part)
        m.add(part)
    ids = np.union1d(np.arange(1003), np.arange(0, n, 10))      # a prefix run (first hole 0) and every tenth row
    assert idx.remove_ids(ids) == m.remove(ids) == ids.size
    assert m.nlive > chunk + 32
    o2n = m.compact()
    assert np.flatnonzero((o2n >= chunk) & (o2n < chunk + 32)).min() > chunk + 32    # the border's rows come from beyond it
    assert np.array_equal(idx.compact(), o2n)
    check(idx, m, "compact")
    idx.close()


# ------------------------------------------------------------------------------------------------- flat: large
LARGE_N = 8_388_608 + 8192 + 5      # more than 1024 tiles of 256 words: tile_scan_kernel takes two tiles per thread
LARGE_D = 40


def _hashed_rows(ids, d=LARGE_D):
    """[len(ids), d] integers in [-63, 63], a function of (row, column) alone; the device version is _hashed_rows_dev."""
    i = np.asarray(ids).astype(np.uint32)[:, None]
    j = np.arange(d, dtype=np.uint32)[None, :]
    h = i * np.uint32(2654435761) + j * np.uint32(40503)        # (wraps at 2^32)
    h ^= h >> np.uint32(13)
    return ((h >> np.uint32(7)) % np.uint32(127)).astype(np.float32) - np.float32(63)


def _hashed_rows_dev(r0, r1, d=LARGE_D):
    import torch
    i = torch.arange(r0, r1, dtype=torch.int64, device="cuda")[:, None]
    j = torch.arange(d, dtype=torch.int64, device="cuda")[None, :]
    h = (i * 2654435761 + j * 40503) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    return (((h >> 7) % 127) - 63).to(torch.float16)


def test_flat_large():
    """The only way to per > 1 in tile_scan_kernel and to the second upload of ts_index_remove: 8 396 805 rows of f16
    d = 40 (256 B per stored row, 2.2 GB), generated on the device; more than 2^22 ids removed in one call."""
    N, d = LARGE_N, LARGE_D
    words = (N + 31) // 32
    tiles = (words + mm.TILE_WORDS - 1) // mm.TILE_WORDS
    per = (tiles + mm.SCAN_THREADS - 1) // mm.SCAN_THREADS
    assert per == 2
    idx = flat_index(d, "f16")
    idx.reserve(N)
    for r0 in range(0, N, 1 << 21):
        idx.add(_hashed_rows_dev(r0, min(N, r0 + (1 << 21))))
    assert idx.ntotal == idx.nlive == N
    assert same_bits(idx.reconstruct_n(N - 4096, 4096), _hashed_rows(np.arange(N - 4096, N)))
    # alternate words, the whole of tile 0 (half of it named twice), the last row
    ids = np.concatenate([HOLE_PATTERNS["alternate_words"](N), HOLE_PATTERNS["whole_tile_0"](N), [N - 1]])
    assert ids.size > mm.REMOVE_CHUNK_IDS
    live = np.ones(N, bool)
    live[ids] = False
    nlive = int(live.sum())
    assert idx.remove_ids(ids) == N - nlive
    assert idx.nlive == nlive and idx.ntotal == N
    from tristage_rag_amd.index import pack_allowed
    assert np.array_equal(idx.live_words(), pack_allowed(live, N))
    old2new = idx.compact()
    before = np.cumsum(live) - live                      # live rows below each row
    assert np.array_equal(old2new, np.where(live, before, -1))
    assert idx.ntotal == idx.nlive == nlive
    new2old = np.flatnonzero(live)
    # 4096-row slices: the start, each staging-chunk border of the new corpus (the first hole is row 0, so the chunks
    # begin at block 0), each border between two threads' tiles of the tile scan, the end
    chunk = mm.compact_chunk_rows(d, "f16")
    assert nlive > 3 * chunk
    centres = [2048, nlive - 2048] + list(range(chunk, nlive, chunk))
    centres += [int(before[t * mm.TILE_ROWS]) for t in range(per, tiles, per)]
    for c in sorted(set(centres)):
        i0 = min(max(c - 2048, 0), nlive - 4096)
        assert same_bits(idx.reconstruct_n(i0, 4096), _hashed_rows(new2old[i0:i0 + 4096])), i0
    # one search against the float64 scores of the survivors, in slices
    q = queries(d)
    k = 50
    cand_s, cand_i = [], []
    for s0 in range(0, nlive, 1 << 19):
        part = _hashed_rows(new2old[s0:s0 + (1 << 19)])
        sc = xi.exact_scores(part, q)
        top = np.argsort(-sc, axis=1, kind="stable")[:, :k]
        cand_s.append(np.take_along_axis(sc, top, axis=1))
        cand_i.append(top + s0)
    cand_s, cand_i = np.concatenate(cand_s, axis=1), np.concatenate(cand_i, axis=1)
    order = np.lexsort((cand_i, -cand_s), axis=1)[:, :k]        # score descending, ties by ascending id
    want_s = np.take_along_axis(cand_s, order, axis=1).astype(np.float32)
    want_i = np.take_along_axis(cand_i, order, axis=1)
    D, I = idx.search(q, k)
    assert np.array_equal(I, want_i)
    assert same_bits(D, want_s)
    idx.close()


# --------------------------------------------------------------------------------------------------------- IVF
NLIST = 8
IVF = [("f16", 96), ("bf16", 768)]
IVF_N = (5000, mm.FILTER_FLOOR + 37)     # the dense path, and the filter path with a partial block


def ivf_index(d, storage, offset=0):
    from tristage_rag_amd.index import IVFFlatIndex
    ivf = IVFFlatIndex(d, NLIST, dtype=storage, nprobe=NLIST)
    c = mm.rows_for(NLIST, d, seed=777).astype(np.float64)
    ivf.set_centroids((c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32))
    if offset:
        ivf.set_id_offset(offset)
    return ivf


def row_lists(ivf):
    """The list of every stored row: the quantizer's top 1 of the stored row, which is what add assigned."""
    import torch
    return ivf.probe(torch.from_numpy(ivf.reconstruct_n()).cuda(), 1)[1][:, 0].cpu().numpy()


def check_ivf(ivf, m, what, probes=(1, 3)):
    check_state(ivf, m, what)
    check_search(ivf, m, what, nprobe=NLIST)      # every list probed: the model's top k, whatever the assignment
    if m.ntotal == 0 or not probes:
        return
    lists = row_lists(ivf)
    assert np.array_equal(np.bincount(lists[m.live], minlength=NLIST), ivf.list_sizes()), what
    q = queries(m.d)
    for p in probes:
        P = ivf.probe(q, p)[1]
        check_search(ivf, m, (what, p), allowed=[np.isin(lists, P[i]) for i in range(B)], nprobe=p)
    return lists


def _ivf_pair(storage, d, n, offset=0):
    x = rows(n, d)
    ivf, m = ivf_index(d, storage, offset), IndexModel(d, offset)
    for part in np.array_split(x, 3):
        ivf.add(dev(part, storage))
    m.add(x)
    return ivf, m, x


@pytest.mark.parametrize("n", IVF_N)
@pytest.mark.parametrize("storage,d", IVF)
def test_ivf_planted_lists(storage, d, n):
    """a list that loses every row, a list whose live rows end exactly at a 32-slot block, compact, compact again"""
    ivf, m, x = _ivf_pair(storage, d, n)
    lists = check_ivf(ivf, m, "add")
    sizes = ivf.list_sizes()
    assert (sizes > 80).all()
    a, b = int(np.argmax(sizes)), int(np.argmin(sizes))
    ids = np.flatnonzero(lists == a)
    assert ivf.remove_ids(ids) == m.remove(ids) == sizes[a]
    assert ivf.list_sizes()[a] == 0
    check_ivf(ivf, m, "a list emptied")
    ids = np.flatnonzero(lists == b)[1::2][:sizes[b] % 32 or 32]
    assert ivf.remove_ids(ids) == m.remove(ids) == ids.size
    assert ivf.list_sizes()[b] % 32 == 0 and ivf.list_sizes()[b] > 0
    check_ivf(ivf, m, "a list of whole blocks")
    assert np.array_equal(ivf.compact(), m.compact())
    check_ivf(ivf, m, "compact")
    assert ivf.list_sizes()[a] == 0 and ivf.list_sizes()[b] % 32 == 0
    assert np.array_equal(ivf.compact(), m.compact())
    check_ivf(ivf, m, "compact twice", probes=(3,))
    extra = rows(50, d, seed=9)
    ivf.add(dev(extra, storage))
    m.add(extra)
    check_ivf(ivf, m, "add after compact", probes=(1,))
    ivf.close()


@pytest.mark.parametrize("n", IVF_N)
@pytest.mark.parametrize("storage,d", IVF)
def test_ivf_updates_move_rows_between_lists_and_back(storage, d, n):
    ivf, m, x = _ivf_pair(storage, d, n, offset=70)
    lists = row_lists(ivf)
    sizes = ivf.list_sizes()
    a, b = int(np.argmax(sizes)), int(np.argmin(sizes))
    mine = np.flatnonzero(lists == a)[3:43][::-1].copy()          # 40 rows of list a, descending
    theirs = np.flatnonzero(lists == b)[:40]
    ivf.update_rows(mine + 70, dev(x[theirs], storage))           # the content of rows of list b: they move there
    m.update(mine + 70, x[theirs])
    now = ivf.list_sizes()
    assert now[a] == sizes[a] - 40 and now[b] == sizes[b] + 40
    check_ivf(ivf, m, "moved")
    ivf.update_rows(mine + 70, dev(x[mine], storage))             # and back
    m.update(mine + 70, x[mine])
    assert np.array_equal(ivf.list_sizes(), sizes)
    check_ivf(ivf, m, "moved back", probes=(1,))
    # compact after updates only: the holes of the updates are closed, the map is the identity
    o2n = ivf.compact()
    assert np.array_equal(o2n, np.arange(n)) and np.array_equal(o2n, m.compact())
    check_ivf(ivf, m, "compact after updates only", probes=(3,))
    with pytest.raises(ValueError):
        ivf.update_rows(np.array([n + 70]), dev(x[:1], storage))
    assert ivf.remove_ids([70 + 11]) == m.remove([70 + 11]) == 1
    with pytest.raises(ValueError):
        ivf.update_rows(np.array([70 + 10, 70 + 11]), dev(x[:2], storage))
    with pytest.raises(ValueError):
        ivf.update_rows(np.array([70 + 10, 70 + 10]), dev(x[:2], storage))
    check_ivf(ivf, m, "refused updates", probes=())
    ivf.close()


@pytest.mark.parametrize("n", IVF_N)
@pytest.mark.parametrize("storage,d", IVF)
def test_ivf_life_cycle_and_every_list_emptied(storage, d, n):
    """remove -> update -> compact -> add -> remove; then every row of all lists removed, add, compact; compact to an
    empty index, add again"""
    ivf, m, x = _ivf_pair(storage, d, n)
    rng = np.random.default_rng(n + d)
    ids = HOLE_PATTERNS["alternate_words"](n)
    assert ivf.remove_ids(ids) == m.remove(ids)
    check_ivf(ivf, m, "remove", probes=(3,))
    ids = rng.permutation(np.flatnonzero(m.live))[:500]
    y = rows(500, d, seed=21)
    ivf.update_rows(ids, dev(y, storage))
    m.update(ids, y)
    check_ivf(ivf, m, "update", probes=(1,))
    assert np.array_equal(ivf.compact(), m.compact())
    check_ivf(ivf, m, "compact", probes=(3,))
    extra = rows(777, d, seed=22)
    ivf.add(dev(extra, storage))
    m.add(extra)
    ids = np.concatenate([np.arange(m.ntotal - 400, m.ntotal), [3, 3, -1, 10 ** 12]])
    assert ivf.remove_ids(ids) == m.remove(ids) == 401
    check_ivf(ivf, m, "add, remove", probes=(1,))
    # every row of all lists
    ids = np.arange(m.ntotal)
    assert ivf.remove_ids(ids) == m.remove(ids)
    assert (ivf.list_sizes() == 0).all()
    check_ivf(ivf, m, "everything removed", probes=(3,))
    ivf.add(dev(extra, storage))
    m.add(extra)
    check_ivf(ivf, m, "add to tombstones only", probes=(3,))
    assert np.array_equal(ivf.compact(), m.compact())
    assert m.ntotal == 777
    check_ivf(ivf, m, "compact", probes=(1,))
    ids = np.arange(777)
    assert ivf.remove_ids(ids) == m.remove(ids) == 777
    assert np.array_equal(ivf.compact(), m.compact())
    check_ivf(ivf, m, "compact to nothing")
    ivf.add(dev(extra[:40], storage))
    m.add(extra[:40])
    check_ivf(ivf, m, "add to the empty index", probes=(1,))
    ivf.close()


# -------------------------------------------------------------------------------------------- random sequences
SEQ = [("flat", "f16", 128), ("flat", "f32", 96), ("ivf", "f16", 96)]


@pytest.mark.parametrize("n0", [3000, 40_000])       # the dense path; across the 32768-row floor in both directions
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind,storage,d", SEQ)
def test_random_sequence(kind, storage, d, seed, n0):
    offset = 1000 if seed == 1 else 0
    ivf = kind == "ivf"
    idx = ivf_index(d, storage, offset) if ivf else flat_index(d, storage, offset)
    m = IndexModel(d, offset)
    x = rows(n0, d)
    idx.add(dev(x, storage))
    m.add(x)
    kw = {"nprobe": NLIST} if ivf else {}
    for step, op in enumerate(mm.op_sequence(seed, n0, 30)):
        what = (step, op[0])
        if op[0] == "add":
            y = mm.rows_for(op[1], d, seed=op[2])
            idx.add(dev(y, storage) if step % 2 or ivf else y)         # device and host rows in turn
            m.add(y)
        elif op[0] == "remove":
            assert idx.remove_ids(op[1] + offset) == m.remove(op[1] + offset), what
        elif op[0] == "update":
            y = mm.rows_for(op[1].size, d, seed=op[2])
            idx.update_rows(op[1] + offset, dev(y, storage) if step % 2 or ivf else y)
            m.update(op[1] + offset, y)
        elif op[0] == "compact":
            assert np.array_equal(idx.compact(), m.compact()), what
        else:
            check_search(idx, m, what, **kw)
            continue
        check_state(idx, m, what)
        check_search(idx, m, what, **kw)
    idx.close()
