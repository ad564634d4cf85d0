"""The host model of the mutating calls (tests/mutation_model.py) without a GPU: the model against brute
force, every catalogue entry against the property its name claims at every listed size, the chunk sizes derived from
the rules of the drivers, the op sequences against their promises, and a sensitivity check: a numpy emulation of the
three-launch prefix count and the chunked move of ts_remove.hip, with planted defects, each of which some (pattern,
size) pair of the catalogue must expose.

Two of the five defects leave old2new right: the forgotten valid mask shows in the live count (the new ntotal), the
late first hole in the rows that were not moved.  The emulation therefore returns all three of (old2new, nlive, the
corpus after the move), and the GPU file compares all three after every compaction (ntotal, old2new, reconstruct_n)."""
import numpy as np
import pytest

import exact_inputs as xi
import mutation_model as mm
from mutation_model import HOLE_PATTERNS, SIZES, TILE_ROWS, UPDATE_SETS, IndexModel


# ------------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("d", [40, 96, 128, 1024])
def test_inputs_are_exactly_summable(d):
    c, q = mm.rows_for(2000, d, seed=d), mm.queries_for(5, d, seed=d + 1)
    assert np.abs(c).max() <= 63 and np.array_equal(c, np.rint(c))
    assert np.array_equal(c.astype(np.float16).astype(np.float32), c)           # f16: 11 bits; bf16: 8 bits, 63 < 2^6
    assert np.array_equal((c.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32), c)
    assert xi.assert_exactly_summable(c, q, 1.0) < 24


# ------------------------------------------------------------------------------------------------------- the model
def _brute_topk(rows, live, q, k, offset):
    """Boolean indexing of the final matrix and a fresh expected_topk over what is left."""
    ids = np.flatnonzero(live)
    D, I = xi.expected_topk(rows[live], q, k)
    return D, np.where(I >= 0, ids[np.maximum(I, 0)] + offset if ids.size else -1, -1)


@pytest.mark.parametrize("offset", [0, 1000])
def test_model_against_brute_force(offset):
    d = 40
    rng = np.random.default_rng(offset + 1)
    m = IndexModel(d, offset)
    x0 = mm.rows_for(500, d, seed=1)
    m.add(x0)
    assert (m.ntotal, m.nlive) == (500, 500)
    # remove: unknown, repeated and already removed ids are not counted
    assert m.remove(np.array([5, 5, 7, -1, 500, 10 ** 12]) + offset) == 2
    assert m.remove(np.array([5, 7]) + offset) == 0
    assert m.remove(np.arange(100, 164) + offset) == 64
    live = np.ones(500, bool)
    live[[5, 7]] = False
    live[100:164] = False
    st = m.expected_state()
    assert st["ntotal"] == 500 and st["nlive"] == 434 and np.array_equal(st["live"], live)
    assert np.array_equal(st["rows"], x0)                       # removed rows keep their content
    # update: refused calls change nothing
    y = mm.rows_for(3, d, seed=2)
    for bad in ([1, 2, 500], [1, 2, -1], [1, 2, 1], [1, 2, 5]):
        with pytest.raises(ValueError):
            m.update(np.array(bad) + offset, y)
        assert np.array_equal(m.rows, x0) and np.array_equal(m.live, live)
    m.update(np.array([9, 3, 499]) + offset, y)
    want = x0.copy()
    want[[9, 3, 499]] = y
    assert np.array_equal(m.rows, want)
    q = mm.queries_for(5, d, seed=3)
    for k in (1, 50, 600):
        D, I = m.expected_topk(q, k)
        Db, Ib = _brute_topk(want, live, q, k, offset)
        assert np.array_equal(I, Ib) and np.array_equal(D.view(np.uint32), Db.view(np.uint32))
    allowed = rng.random(500) < 0.5
    D, I = m.expected_topk(q, 50, allowed=allowed)
    Db, Ib = _brute_topk(want, live & allowed, q, 50, offset)
    assert np.array_equal(I, Ib) and np.array_equal(D.view(np.uint32), Db.view(np.uint32))
    # compact, then add: ids continue from the new ntotal
    o2n = m.compact()
    assert np.array_equal(o2n[live], np.arange(434)) and (o2n[~live] == -1).all()
    assert m.ntotal == m.nlive == 434 and np.array_equal(m.rows, want[live])
    x1 = mm.rows_for(50, d, seed=4)
    m.add(x1)
    final = np.concatenate([want[live], x1])
    D, I = m.expected_topk(q, 50)
    Db, Ib = _brute_topk(final, np.ones(484, bool), q, 50, offset)
    assert np.array_equal(I, Ib) and np.array_equal(D.view(np.uint32), Db.view(np.uint32))
    assert m.remove(np.arange(484) + offset) == 484
    D, I = m.expected_topk(q, 5)
    assert (I == -1).all() and (D == -xi.FLT_MAX).all()
    assert m.compact().tolist() == [-1] * 484 and m.ntotal == 0


def test_ties_take_the_ascending_id():
    """At d = 40 a few per cent of neighbouring scores tie: the tie rule is exercised without planting anything."""
    c, q = mm.rows_for(SIZES[-1], 40, seed=0), mm.queries_for(5, 40, seed=1)
    m = IndexModel(40)
    m.add(c)
    D, I = m.expected_topk(q, 2000)
    tie = D[:, 1:] == D[:, :-1]
    assert 0.01 < tie.mean() < 0.2
    assert (I[:, 1:][tie] > I[:, :-1][tie]).all()


# ------------------------------------------------------------------------------------------------ the hole patterns
def _props(name, n, ids):
    """The property the name claims, with the clipping to [0, n) each entry documents."""
    live = np.ones(n, bool)
    live[ids] = False
    words = (np.arange(n) // 32)
    last_word = (n - 1) // 32
    if name == "none":
        return ids.size == 0
    if name == "first_row":
        return ids.tolist() == [0]
    if name == "last_row":
        return ids.tolist() == [n - 1]
    if name == "last_word":
        return np.array_equal(ids, np.flatnonzero(words == last_word)) and ids[-1] == n - 1
    if name == "trailing_run":
        # a run to the end that begins at a block border: nlive blocks == first hole's block, the gather loop is idle
        return ids[0] % 32 == 0 and np.array_equal(ids, np.arange(ids[0], n)) and ids[0] // 32 >= (live.sum() + 31) // 32
    if name == "one_word":
        w = ids[0] // 32
        return np.array_equal(ids, np.flatnonzero(words == w)) and (ids.size == 32 or n < 32)
    if name == "word_minus_one":
        w = (n // 32) // 2
        return np.array_equal(ids, np.flatnonzero(words == w)[:-1]) and (ids.size == 31 or n < 32)
    if name == "whole_tile_0":
        return np.array_equal(ids, np.arange(min(n, TILE_ROWS)))
    if name == "whole_tile_middle":
        t = mm.middle_tile(n)
        full = np.array_equal(ids, np.arange(TILE_ROWS * t, min(n, TILE_ROWS * (t + 1)))) and ids.size > 0
        return full and (t > 0 or n <= TILE_ROWS) and (ids.size == TILE_ROWS or n < 2 * TILE_ROWS)
    if name == "across_tile_border":
        return ids.tolist() == [r for r in (TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1) if r < n]
    if name == "alternate_rows":
        return np.array_equal(live, np.arange(n) % 2 == 1)
    if name == "alternate_words":
        return np.array_equal(live, words % 2 == 0)
    if name == "all_but_first":
        return np.flatnonzero(live).tolist() == [0]
    if name == "all_but_last":
        return np.flatnonzero(live).tolist() == [n - 1]
    if name == "all_but_middle":
        return np.flatnonzero(live).tolist() == [n // 2]
    if name == "everything":
        return not live.any()
    if name == "hole_only_in_last_block":
        return ids.size == 1 and ids[0] // 32 == last_word
    raise AssertionError(name)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(HOLE_PATTERNS))
def test_every_pattern_has_the_property_its_name_claims(name, n):
    ids = HOLE_PATTERNS[name](n)
    assert ids.dtype == np.int64 and ids.ndim == 1
    assert ((ids >= 0) & (ids < n)).all() and np.unique(ids).size == ids.size
    assert np.array_equal(ids, np.sort(ids))
    assert _props(name, n, ids), (name, n)


def test_the_sizes_cover_the_word_and_tile_edges():
    assert {n % 32 for n in SIZES} >= {0, 1, 31}
    assert {TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1} <= set(SIZES)
    assert max(SIZES) > mm.FILTER_FLOOR and max(SIZES) % 32 != 0
    # somewhere: one survivor, none, a whole tile gone with tiles behind it, a run across a tile border
    assert any(HOLE_PATTERNS["whole_tile_0"](n).size == TILE_ROWS < n for n in SIZES)
    assert any(HOLE_PATTERNS["whole_tile_middle"](n)[0] >= TILE_ROWS and HOLE_PATTERNS["whole_tile_middle"](n).size == TILE_ROWS for n in SIZES)
    assert any(HOLE_PATTERNS["across_tile_border"](n).size == 3 for n in SIZES)


# ------------------------------------------------------------------------------------------------- the update sets
def test_chunk_rows_follow_the_two_rules_of_the_driver():
    # ts_make_layout: d padded to 8 k groups (128 elements of 2 bytes, 64 of 4); a block is 32 padded rows
    assert mm.block_bytes(40, "f16") == 32 * 128 * 2 and mm.block_bytes(128, "bf16") == 32 * 128 * 2
    assert mm.block_bytes(96, "f32") == 32 * 128 * 4 and mm.block_bytes(1024, "f32") == 128 << 10
    assert mm.block_bytes(1024, "f16") == 64 << 10
    for d, st in ((40, "f16"), (128, "bf16"), (96, "f32"), (1024, "f16"), (1024, "f32")):
        bb = mm.block_bytes(d, st)
        assert mm.update_chunk_rows(d, st) * bb == 32 * mm.UPDATE_STAGE_BYTES          # rule 1: 64 MiB of row blocks
        assert mm.compact_chunk_rows(d, st) * bb == 32 * mm.COMPACT_STAGE_BYTES
        host = mm.update_chunk_rows(d, st, host_elem_bytes=4)
        assert host % 32 == 0 and host <= mm.update_chunk_rows(d, st)
        assert host * d * 4 <= mm.HOST_STAGE_BYTES                                       # rule 2: 64 MiB of host rows
        assert host == mm.update_chunk_rows(d, st) or (host + 32) * d * 4 > mm.HOST_STAGE_BYTES
    # float32 host rows into f16 storage at d = 1024: the host rule gives the smaller chunk, and 20 000 ids cross it
    assert mm.update_chunk_rows(1024, "f16", host_elem_bytes=4) < mm.update_chunk_rows(1024, "f16")
    assert mm.update_chunk_rows(1024, "f16", host_elem_bytes=4) < 20_000 < 2 * mm.update_chunk_rows(1024, "f16", 4)
    # f32 storage at d = 1024: 100 000 rows with more than one staging chunk of survivors
    assert mm.compact_chunk_rows(1024, "f32") < 0.9 * 100_000


def _is_run(ids):
    return bool((np.diff(ids) == 1).all())


@pytest.mark.parametrize("name", sorted(UPDATE_SETS))
def test_every_update_set_has_the_property_its_name_claims(name):
    chunk = 4096                                        # (a stand-in: the sets take the chunk rows as a parameter)
    n = mm.update_rows_needed(name, chunk) + 3
    ids = UPDATE_SETS[name](n, chunk, np.random.default_rng(0))
    assert ids.dtype == np.int64 and ((ids >= 0) & (ids < n)).all() and np.unique(ids).size == ids.size
    blocks, counts = np.unique(ids // 32, return_counts=True)
    B = mm.BLOCK
    if name == "one_id":
        assert ids.size == 1
    elif name == "block_31":
        assert ids.size == 31 and blocks.tolist() == [B] and not _is_run(ids)
    elif name == "block_32_swapped":
        assert counts.tolist() == [32] and blocks.tolist() == [B] and not _is_run(ids)
    elif name == "block_33":
        assert blocks.tolist() == [B, B + 1] and counts.tolist() == [32, 1] and not _is_run(ids)
    elif name == "block_shuffled":
        assert counts.tolist() == [32] and not _is_run(ids) and not _is_run(ids[::-1])
    elif name == "block_descending":
        assert counts.tolist() == [32] and _is_run(ids[::-1])
    elif name == "two_blocks_interleaved":
        assert counts.tolist() == [32, 32] and (np.diff(ids // 32) != 0).all()
    elif name == "every_row":
        assert ids.size == n and not _is_run(ids)
    elif name == "every_row_ascending":
        assert ids.size == n and _is_run(ids) and ids[0] == 0
    elif name == "unaligned_run":
        assert _is_run(ids) and ids[0] % 32 != 0 and (ids[-1] + 1) % 32 != 0 and ids.size > 64
    elif name == "run_of_one":
        assert ids.tolist() == [n - 1]
    elif name == "ascending_not_a_run":
        assert (np.diff(ids) > 1).all() and (counts < 32).all()
    elif name == "straddle_chunk_border":
        assert ids.size > chunk and not _is_run(ids)
        first, second = ids[:chunk], ids[chunk:]
        split = np.intersect1d(first // 32, second // 32)
        halves = [b for b in split if (first // 32 == b).sum() == 16 and (second // 32 == b).sum() == 16]
        assert len(halves) == 1 and len(split) > 1      # the planted block, and blocks that leave 31 rows behind
        assert (np.bincount(first // 32) == 32).any()   # full blocks too
    else:
        raise AssertionError(name)


# -------------------------------------------------------------------------------------------------- the sequences
def _has(kinds, sub):
    return any(kinds[i:i + len(sub)] == sub for i in range(len(kinds)))


@pytest.mark.parametrize("n0", [3000, 40_000])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_op_sequences_keep_their_promises(seed, n0):
    ops = mm.op_sequence(seed, n0, 30)
    assert [o[0] for o in ops] == [o[0] for o in mm.op_sequence(seed, n0, 30)]     # seeded
    kinds = [o[0] for o in ops]
    assert 25 <= len(ops) <= 45
    for sub in (["remove", "add", "remove"], ["compact", "add", "remove", "search"], ["remove", "add", "compact"],
                ["compact", "compact"], ["update", "compact", "update"]):
        assert _has(kinds, sub), sub
    d = 8
    m = IndexModel(d)
    m.add(mm.rows_for(n0, d, seed=5))
    unaligned = everything = False
    sizes = [m.ntotal]
    for i, op in enumerate(ops):
        if op[0] == "add":
            if kinds[i - 1:i + 2] == ["remove", "add", "remove"] and m.ntotal % 32 and m.nlive < m.ntotal:
                unaligned = True
            m.add(mm.rows_for(op[1], d, seed=op[2]))
        elif op[0] == "remove":
            m.remove(op[1])
            everything = everything or (m.nlive == 0 and m.ntotal > 0)
        elif op[0] == "update":
            m.update(op[1], mm.rows_for(op[1].size, d, seed=op[2]))          # raises if a pre-condition is broken
        elif op[0] == "compact":
            m.compact()
        else:
            assert m.ntotal > 0 and op[1] in (1, 50)
        sizes.append(m.ntotal)
    assert unaligned and everything
    if n0 > mm.FILTER_FLOOR:   # across the filter path's floor in both directions
        below = [s < mm.FILTER_FLOOR for s in sizes]
        assert any(a and not b for a, b in zip(below, below[1:])) and any(b and not a for a, b in zip(below, below[1:]))
    else:
        assert max(sizes) < mm.FILTER_FLOOR


# ------------------------------------------------------------------------------------- sensitivity: planted defects
EMU = dict(tile_words=4, threads=8, chunk_rows=64)      # 128-row tiles: per > 1 from 1025 rows on, many staging chunks


def _emu_cases():
    for n in SIZES:
        for name in sorted(HOLE_PATTERNS):
            live = np.ones(n, bool)
            live[HOLE_PATTERNS[name](n)] = False
            yield name, n, live


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_the_emulation_is_right_without_a_defect():
    reached_per = 0
    for name, n, live in _emu_cases():
        want = mm.expected_compact(live)
        assert _same(mm.emulate_compact(live, **EMU), want), (name, n)
        tiles = ((n + 31) // 32 + EMU["tile_words"] - 1) // EMU["tile_words"]
        reached_per = max(reached_per, (tiles + EMU["threads"] - 1) // EMU["threads"])
        if n <= 2 * TILE_ROWS + 5:   # the library's own widths too (per = 1 at these sizes)
            assert _same(mm.emulate_compact(live), want), (name, n)
    assert reached_per > 1


@pytest.mark.parametrize("defect", mm.DEFECTS)
def test_every_planted_defect_is_caught_by_a_named_entry(defect):
    caught = [(name, n) for name, n, live in _emu_cases()
              if not _same(mm.emulate_compact(live, defect=defect, **EMU), mm.expected_compact(live))]
    assert caught, defect
    # and in the part of the result the defect is about: old2new, the live count, the rows after the move
    part = {"inclusive_scan": 0, "tile_prefix_dropped": 0, "per_rounded_down": 0, "valid_mask_forgotten": 1,
            "first_hole_late": 2}[defect]
    assert any(not np.array_equal(mm.emulate_compact(live, defect=defect, **EMU)[part], mm.expected_compact(live)[part])
               for _, _, live in _emu_cases()), defect
    print(defect, "caught by", len(caught), "pairs, first", caught[0])
