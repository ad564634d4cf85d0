"""An exact host model of the mutating calls of FlatIPIndex / IVFFlatIndex: add, remove_ids,
update_rows, compact.  numpy only; tests/test_mutation_model_host.py checks the model and the catalogues below against
brute force, tests/test_mutation_gpu.py holds the kernels of ts_remove.hip, ts_update.hip, ts_ivf_compact.hip and the
drivers of ts_index.hip / ts_ivf.hip to it.

Rows and queries are ``exact_inputs.gen_ints`` integers in [-63, 63]: exact in f16 / bf16 / f32 storage, every score
exact in fp32 under any summation order (``assert_exactly_summable`` holds up to d = 1024), so every comparison of this
work is ``np.array_equal`` on bits.

  IndexModel        the matrix of every row since the last compaction, the live vector, the id offset
  HOLE_PATTERNS     named sets of rows to remove, (n) -> ids, each aimed at a branch of the compaction kernels
  SIZES             the corpus sizes the patterns are paired with
  UPDATE_SETS       named id sets for update_rows, (n, chunk_rows, rng) -> ids, aimed at ts_update_group_blocks
  op_sequence       seeded interleavings of add / remove / update / compact / search
  emulate_compact   the three-launch prefix count and the chunked move of ts_remove.hip in numpy, with planted defects
"""
import numpy as np

import exact_inputs as xi

ROWS_PER_BLOCK = 32                 # TS_ROWS_PER_BLOCK: a word of the tombstone bitmap is a row block
TILE_WORDS = 256                    # kTile of ts_remove.hip: words per workgroup of the prefix count
TILE_ROWS = TILE_WORDS * 32         # 8192
SCAN_THREADS = 1024                 # tile_scan_kernel's one workgroup
REMOVE_CHUNK_IDS = 1 << 22          # ids per upload of ts_index_remove
COMPACT_STAGE_BYTES = 256 << 20     # kCompactStageBytes
UPDATE_STAGE_BYTES = 64 << 20       # kUpdateStageBytes
HOST_STAGE_BYTES = 64 << 20         # the staging of host rows (ts_index_add / ts_index_update)
FILTER_FLOOR = 32768                # below this many rows a search takes the dense path

SIZES = (1, 31, 32, 33, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 5, FILTER_FLOOR + 37)


def rows_for(n, d, seed):
    """[n, d] float32 integers in [-63, 63] (gen_ints)."""
    return xi.gen_ints(n, d, 1, seed=seed)[0]


def queries_for(B, d, seed):
    return xi.gen_ints(1, d, B, seed=seed)[1]


# ------------------------------------------------------------------------------------------------ the tiled layout
def block_bytes(d, storage):
    """Bytes of a 32-row block (ts_make_layout / ts_block_bytes): d padded to 8 k groups of 16 bytes per lane."""
    esize = 4 if storage == "f32" else 2
    gk = 2 * (16 // esize)
    q = gk * 8
    dpad = (d + q - 1) // q * q
    return (dpad // gk) * 1024


def compact_chunk_rows(d, storage):
    """Rows per staging chunk of ts_compact_corpus: whole row blocks in 256 MiB."""
    return max(1, COMPACT_STAGE_BYTES // block_bytes(d, storage)) * ROWS_PER_BLOCK


def update_chunk_rows(d, storage, host_elem_bytes=None):
    """Rows per staging chunk of ts_index_update for ids that are not one run: 64 MiB over the block bytes, and for
    host rows (``host_elem_bytes`` = 4 or 2) at most 64 MiB over the row bytes, in whole row blocks."""
    chunk = max(1, UPDATE_STAGE_BYTES // block_bytes(d, storage)) * ROWS_PER_BLOCK
    if host_elem_bytes is not None:
        host = HOST_STAGE_BYTES // (d * host_elem_bytes) // ROWS_PER_BLOCK * ROWS_PER_BLOCK
        chunk = min(chunk, max(ROWS_PER_BLOCK, host))
    return chunk


# ------------------------------------------------------------------------------------------------------- the model
class IndexModel:
    """What an index holds.  Ids are row numbers plus ``offset``; removed rows keep their content (and their ids) until
    ``compact``, as FlatIPIndex.remove_ids and IVFFlatIndex.remove_ids document."""

    def __init__(self, d, offset=0):
        self.d = int(d)
        self.offset = int(offset)
        self.rows = np.zeros((0, self.d), dtype=np.float32)
        self.live = np.zeros(0, dtype=bool)

    @property
    def ntotal(self):
        return int(self.live.shape[0])

    @property
    def nlive(self):
        return int(self.live.sum())

    def add(self, x):
        x = np.asarray(x, np.float32)
        assert x.ndim == 2 and x.shape[1] == self.d
        self.rows = np.concatenate([self.rows, x])
        self.live = np.concatenate([self.live, np.ones(x.shape[0], bool)])

    def remove(self, ids):
        """The number of rows removed: unknown, repeated and already removed ids are not counted."""
        r = np.unique(np.asarray(ids, np.int64).reshape(-1) - self.offset)
        r = r[(r >= 0) & (r < self.ntotal)]
        r = r[self.live[r]]
        self.live[r] = False
        return int(r.size)

    def update(self, ids, x):
        """All or nothing: an id out of range, given twice or removed raises ValueError and nothing changes."""
        r = np.asarray(ids, np.int64).reshape(-1) - self.offset
        x = np.asarray(x, np.float32)
        assert x.shape == (r.size, self.d)
        if ((r < 0) | (r >= self.ntotal)).any():
            raise ValueError("update: an id is not an id of this index")
        if np.unique(r).size != r.size:
            raise ValueError("update: an id is given twice")
        if not self.live[r].all():
            raise ValueError("update: an id was removed")
        self.rows[r] = x

    def compact(self):
        """old -> new, int64 [old ntotal], -1 for a removed row; the survivors keep their order."""
        old2new = np.where(self.live, np.cumsum(self.live) - 1, -1).astype(np.int64)
        self.rows = self.rows[self.live]
        self.live = np.ones(self.rows.shape[0], bool)
        return old2new

    def expected_state(self):
        return {"ntotal": self.ntotal, "nlive": self.nlive, "live": self.live.copy(), "rows": self.rows}

    def expected_topk(self, q, k, allowed=None):
        D, I = xi.expected_topk(self.rows, q, k, live=self.live, allowed=allowed)
        return D, np.where(I >= 0, I + self.offset, -1)


# ------------------------------------------------------------------------------------------------- hole patterns
def _clip(ids, n):
    ids = np.asarray(ids, np.int64)
    return ids[(ids >= 0) & (ids < n)]


def _word(n, w):
    return _clip(np.arange(32 * w, 32 * w + 32), n)


def _middle_word(n):
    return (n // 32) // 2            # a whole word wherever n >= 32


def middle_tile(n):
    return ((n + TILE_ROWS - 1) // TILE_ROWS) // 2


def whole_tile(t):
    def f(n):
        tt = middle_tile(n) if t == "middle" else t
        return _clip(np.arange(TILE_ROWS * tt, TILE_ROWS * (tt + 1)), n)
    return f


def _trailing_run(n):
    """From a block border to the end: the new corpus ends where the first hole begins, so the gather loop of
    ts_compact_corpus does not run and only its memset does."""
    nblocks = (n + 31) // 32
    return np.arange(32 * (nblocks // 2), n, dtype=np.int64)


def _hole_only_in_last_block(n):
    first = 32 * ((n - 1) // 32)
    return np.array([(first + n - 1) // 2], dtype=np.int64)


HOLE_PATTERNS = {
    "none": lambda n: np.zeros(0, np.int64),
    "first_row": lambda n: np.array([0], np.int64),
    "last_row": lambda n: np.array([n - 1], np.int64),
    "last_word": lambda n: _word(n, (n - 1) // 32),
    "trailing_run": _trailing_run,
    "one_word": lambda n: _word(n, _middle_word(n)),
    "word_minus_one": lambda n: _word(n, _middle_word(n))[:-1],
    "whole_tile_0": whole_tile(0),
    "whole_tile_middle": whole_tile("middle"),
    "across_tile_border": lambda n: _clip(np.arange(TILE_ROWS - 1, TILE_ROWS + 2), n),
    "alternate_rows": lambda n: np.arange(0, n, 2, dtype=np.int64),
    "alternate_words": lambda n: np.flatnonzero((np.arange(n) // 32) % 2 == 1).astype(np.int64),
    "all_but_first": lambda n: np.arange(1, n, dtype=np.int64),
    "all_but_last": lambda n: np.arange(0, n - 1, dtype=np.int64),
    "all_but_middle": lambda n: np.delete(np.arange(n, dtype=np.int64), n // 2),
    "everything": lambda n: np.arange(n, dtype=np.int64),
    "hole_only_in_last_block": _hole_only_in_last_block,
}


# --------------------------------------------------------------------------------------------------- update sets
# (n, chunk_rows, rng) -> ids (row numbers, in the order given to update_rows).  BLOCK is the row block the small sets
# sit around; every set needs n >= update_rows_needed(name, chunk_rows).
BLOCK = 3


def _block_rows(b):
    return np.arange(32 * b, 32 * b + 32, dtype=np.int64)


def _straddle(n, chunk_rows, rng):
    """chunk_rows + 64 ids, shuffled, with the 32 rows of one block at the positions chunk_rows - 16 ... + 15: that
    block is split 16 / 16 between the two staging chunks, and the 64 shuffled rows that land in the second chunk
    leave 31 of their block in the first."""
    m = chunk_rows + 64
    planted = _block_rows(m // 64)                    # a block in the middle of the rows used
    rest = rng.permutation(np.setdiff1d(np.arange(m, dtype=np.int64), planted))
    at = chunk_rows - 16
    return np.concatenate([rest[:at], rng.permutation(planted), rest[at:]])


UPDATE_SETS = {
    "one_id": lambda n, c, rng: np.array([32 * BLOCK + 7], np.int64),
    "block_31": lambda n, c, rng: _block_rows(BLOCK)[[0] + list(range(2, 32))],          # 31 of 32: partial, not a run
    "block_32_swapped": lambda n, c, rng: _block_rows(BLOCK)[[1, 0] + list(range(2, 32))],   # all 32, not a run
    "block_33": lambda n, c, rng: np.concatenate([_block_rows(BLOCK)[::-1], [32 * BLOCK + 32]]),   # full + 1 of the next
    "block_shuffled": lambda n, c, rng: rng.permutation(_block_rows(BLOCK)),
    "block_descending": lambda n, c, rng: _block_rows(BLOCK)[::-1].copy(),
    "two_blocks_interleaved": lambda n, c, rng: np.stack([_block_rows(BLOCK), _block_rows(BLOCK + 2)], 1).reshape(-1),
    "every_row": lambda n, c, rng: rng.permutation(n).astype(np.int64),
    "every_row_ascending": lambda n, c, rng: np.arange(n, dtype=np.int64),               # one run from row 0
    "unaligned_run": lambda n, c, rng: np.arange(32 * BLOCK + 17, 32 * BLOCK + 17 + 70, dtype=np.int64),
    "run_of_one": lambda n, c, rng: np.array([n - 1], np.int64),
    "ascending_not_a_run": lambda n, c, rng: np.arange(5, min(n, 32 * (BLOCK + 3)), 3, dtype=np.int64),
    "straddle_chunk_border": _straddle,
}


def update_rows_needed(name, chunk_rows):
    return chunk_rows + 64 if name == "straddle_chunk_border" else 32 * (BLOCK + 3) + 5


# ------------------------------------------------------------------------------------------------- op sequences
def op_sequence(seed, n0, steps=30):
    """A list of ops on an index that starts with ``n0`` rows.  Ids are row numbers (the runner adds the id offset);
    rows come from ``rows_for(count, d, rowseed)``.
      ("add", count, rowseed) ("remove", ids) ("update", ids, rowseed) ("compact",) ("search", k)
    Removal sets come from HOLE_PATTERNS as well as at random, and carry a few unknown, repeated and already removed ids;
    updates name live ids only, each once.  Every sequence contains
      remove -> add at an unaligned row -> remove        compact -> add -> remove -> search
      remove everything -> add -> compact (-> add)              compact -> compact        update -> compact -> update
    and random ops between them, up to about ``steps`` ops."""
    rng = np.random.default_rng([seed, n0, 77])
    live = np.ones(n0, bool)
    ops = []
    rowseed = [1000 * (seed + 1)]
    names = sorted(HOLE_PATTERNS)

    def add(count):
        nonlocal live
        rowseed[0] += 1
        ops.append(("add", int(count), rowseed[0]))
        live = np.concatenate([live, np.ones(count, bool)])

    def remove(ids=None):
        n = live.size
        if n == 0:
            return add(37)
        if ids is None:
            if rng.random() < 0.5:
                name = names[rng.integers(len(names))]
                ids = HOLE_PATTERNS["alternate_rows" if name == "everything" else name](n)
            else:
                ids = np.flatnonzero(rng.random(n) < rng.choice([0.01, 0.3]))
        ids = np.asarray(ids, np.int64)
        junk = np.array([-1, n, n + 12345, 10 ** 12], np.int64)
        gone = np.flatnonzero(~live)[:3]
        ids = rng.permutation(np.concatenate([ids, ids[:5], junk, gone]))
        ops.append(("remove", ids))
        live[ids[(ids >= 0) & (ids < n)]] = False

    def update():
        alive = np.flatnonzero(live)
        if alive.size == 0:
            return add(50)
        kind = rng.integers(3)
        if kind == 0:     # random ids, shuffled
            ids = rng.permutation(alive[rng.random(alive.size) < 0.05])
        elif kind == 1:   # every live row of a few blocks: full where nothing of the block is removed
            b = rng.integers(0, (live.size + 31) // 32, size=3)
            ids = rng.permutation(alive[np.isin(alive // 32, b)])
        else:             # a run of live rows
            s = alive[rng.integers(alive.size)]
            e = s
            while e < live.size and live[e] and e - s < 100:
                e += 1
            ids = np.arange(s, e, dtype=np.int64)
        if ids.size == 0:
            ids = alive[:1]
        rowseed[0] += 1
        ops.append(("update", ids.astype(np.int64), rowseed[0]))

    def compact():
        nonlocal live
        ops.append(("compact",))
        live = np.ones(int(live.sum()), bool)

    def search():
        if live.size == 0:
            add(33)
        ops.append(("search", int(rng.choice([1, 50]))))

    def s_unaligned():
        if live.size % 32 == 0:
            add(5)
        remove()
        add(37)
        remove()

    def s_compact_add():
        compact()
        add(50)
        remove()
        search()

    def s_everything():
        remove(np.arange(live.size))
        add(n0 // 8 + 13)     # an unaligned row count, below the filter path's floor
        compact()
        add(n0)               # and back above the size it started with

    def s_twice():
        compact()
        compact()

    def s_update():
        update()
        compact()
        update()

    scripts = [s_unaligned, s_compact_add, s_everything, s_twice, s_update]
    random_ops = [lambda: add(int(rng.choice([1, 17, 50, n0 // 4 + 3]))), remove, update, compact, search]
    fill = max(0, steps - 15)
    for i in rng.permutation(len(scripts)):
        for _ in range(fill // len(scripts)):
            random_ops[rng.choice(5, p=[0.2, 0.3, 0.2, 0.1, 0.2])]()
        scripts[i]()
    search()
    return ops


# -------------------------------------------------------------------------- the compaction of ts_remove.hip, emulated
DEFECTS = ("inclusive_scan", "tile_prefix_dropped", "per_rounded_down", "valid_mask_forgotten", "first_hole_late")


def emulate_compact(live, tile_words=TILE_WORDS, threads=SCAN_THREADS, chunk_rows=1 << 30, defect=None):
    """ts_compact_corpus in numpy, launch by launch: word_count_kernel (popcount per word under the valid mask, sums per
    tile of ``tile_words`` words, the first hole), tile_scan_kernel (exclusive scan of the tile sums by ``threads``
    threads with ``per`` tiles each), word_scan_kernel (offsets of the words in their tile plus the tile's prefix),
    compact_map_kernel, then the chunked move from block first_hole / 32 on and the trailing memset.

    The bitmap it builds has the bits beyond ntotal SET: the library keeps them clear, and the valid mask is what makes
    the count right when they are not.  Returns ``(old2new, nlive, moved)``; ``moved[s]`` is the old row whose content
    slot s of the corpus holds afterwards, -1 for zeros, over the old number of blocks.
    ``defect``: one of DEFECTS, a kernel that is subtly wrong."""
    live = np.asarray(live, bool)
    n = live.size
    words = (n + 31) // 32
    bits = np.ones(words * 32, bool)          # (padding bits set on purpose)
    bits[:n] = live
    bits = bits.reshape(words, 32)
    valid = (np.arange(words * 32).reshape(words, 32) < n)
    if defect == "valid_mask_forgotten":
        valid = np.ones_like(valid)
    # launch 1
    lw = bits & valid
    cnt = lw.sum(axis=1).astype(np.int64)
    tiles = (words + tile_words - 1) // tile_words
    padded = np.zeros(tiles * tile_words, np.int64)
    padded[:words] = cnt
    tile_sum = padded.reshape(tiles, tile_words).sum(axis=1)
    holes = np.flatnonzero((~lw & valid).reshape(-1))
    first_hole = int(holes[0]) if holes.size else n
    # launch 2: thread t owns the tiles [t * per, t * per + per)
    per = tiles // threads if defect == "per_rounded_down" else (tiles + threads - 1) // threads
    t0 = np.minimum(tiles, np.arange(threads) * per)
    t1 = np.minimum(tiles, t0 + per)
    sums = np.array([tile_sum[a:b].sum() for a, b in zip(t0, t1)], np.int64)
    run = np.cumsum(sums) - (0 if defect == "inclusive_scan" else sums)
    tile_pre = tile_sum.copy()                # (a tile no thread owns keeps its sum, as the kernel would leave it)
    for t in range(threads):
        r = run[t]
        for i in range(t0[t], t1[t]):
            tile_pre[i] = r
            r += tile_sum[i]
    # launch 3
    in_tile = padded.reshape(tiles, tile_words)
    x = (np.cumsum(in_tile, axis=1) - in_tile)
    pre = (x + (0 if defect == "tile_prefix_dropped" else tile_pre[:, None])).reshape(-1)[:words]
    # launch 4
    rows = np.arange(n)
    below = (np.cumsum(bits, axis=1) - bits).reshape(-1)[:n]      # popcount(lw & (bit - 1))
    old2new = np.where(live, pre[rows // 32] + below, -1).astype(np.int64)
    nlive = int(pre[-1] + cnt[-1]) if words else 0
    # the move: chunks of whole new blocks through a staging image, then the memset of the blocks left over
    old_blocks = (n + 31) // 32
    new_blocks = (nlive + 31) // 32
    moved = np.full(max(old_blocks, new_blocks) * 32, -1, np.int64)   # (a defect may count rows that do not exist)
    moved[:n] = rows
    new2old = np.full(max(nlive, 0), -1, np.int64)
    ok = live & (old2new >= 0) & (old2new < new2old.size)
    new2old[old2new[ok]] = rows[ok]
    b = first_hole // 32 + (1 if defect == "first_hole_late" else 0)
    cb = max(1, chunk_rows // 32)
    while b < new_blocks:
        nb = min(cb, new_blocks - b)
        j = np.arange(32 * b, 32 * (b + nb))
        src = np.full(j.size, -1, np.int64)
        src[j < new2old.size] = new2old[j[j < new2old.size]]
        stage = np.where(src >= 0, moved[np.maximum(src, 0)], -1)
        moved[32 * b:32 * (b + nb)] = stage
        b += cb
    if old_blocks > new_blocks:
        moved[32 * max(new_blocks, 0):] = -1
    return old2new, nlive, moved[:old_blocks * 32]


def expected_compact(live):
    """What emulate_compact must return, from the model: boolean indexing and nothing else."""
    live = np.asarray(live, bool)
    n = live.size
    old2new = np.where(live, np.cumsum(live) - 1, -1).astype(np.int64)
    nlive = int(live.sum())
    moved = np.full((n + 31) // 32 * 32, -1, np.int64)
    moved[:nlive] = np.flatnonzero(live)
    # Beyond nlive every slot is zero: with a hole below nlive the chunk loop rewrites the last new block and zeroes
    # its padding; with only a tail removed nlive is the first hole, and either it ends a block or its block is the
    # one chunk the loop takes; with no hole nothing moves and the padding was never written.
    return old2new, nlive, moved
