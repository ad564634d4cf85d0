"""Wide coalesced passes, host side (no GPU): groups per wide pass, the corpus size where the queue switches to them,
and the flags / entry points the binding uses."""
import re

from tristage_rag_amd import _lib

F32, F16, BF16 = 0, 1, 2


def test_wide_groups_do_not_depend_on_the_dimension():
    lib = _lib.load()
    for d in (64, 384, 700, 768, 1024, 2048, 4096):
        assert lib.ts_coalesce_groups_wide(d, F16) == 6, d
        assert lib.ts_coalesce_groups_wide(d, BF16) == 6, d
    assert lib.ts_coalesce_groups_wide(768, F32) == 0   # fp32 storage has no multi-group scan
    assert lib.ts_coalesce_groups_wide(0, F16) == 0
    # the LDS-resident group counts are unchanged
    assert [lib.ts_coalesce_groups(d, F16) for d in (384, 768, 1024)] == [4, 3, 2]


def _corpus_bytes(rows, d):
    dpad = -(-d // 128) * 128
    return -(-rows // 32) * 32 * dpad * 2


def test_auto_policy_threshold():
    lib = _lib.load()
    t = lib.ts_coalesce_wide_min_bytes()
    assert t == 256 << 20   # the Infinity Cache: below it a pass saved saves no HBM bytes
    # 100 k x 768 (154 MB, test_coalesce_gpu.py::test_scans_are_shared) keeps the LDS-resident passes
    assert _corpus_bytes(100_000, 768) <= t
    # 200 k x 1024 and the bench's 10 M x 768 take wide passes (400 k x 384 would too, but its resident passes take
    # 4 groups: the auto policy keeps those; test_coalesce_wide_gpu.py checks both)
    assert _corpus_bytes(200_000, 1024) > t
    assert _corpus_bytes(10_000_000, 768) > t


def test_flags_and_abi():
    src = open(_lib.HEADER_PATH).read()
    for name in ("TS_FLAG_WIDE_PASSES", "TS_FLAG_NO_WIDE_PASSES"):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, src).group(1)) == getattr(_lib, name)
    used = {_lib.TS_FLAG_HOST_PTR, _lib.TS_FLAG_NO_FILTER, _lib.TS_FLAG_NORMALIZE, _lib.TS_FLAG_ASYNC,
            _lib.TS_FLAG_PIPELINE, _lib.TS_FLAG_CLASSIC, _lib.TS_FLAG_ONE_LAUNCH, _lib.TS_FLAG_COALESCE}
    assert not {_lib.TS_FLAG_WIDE_PASSES, _lib.TS_FLAG_NO_WIDE_PASSES} & used
    assert _lib.TS_FLAG_WIDE_PASSES != _lib.TS_FLAG_NO_WIDE_PASSES
    for name in ("ts_coalesce_groups_wide", "ts_coalesce_wide_min_bytes"):
        assert name in _lib.SIGNATURES
    assert "#define TS_ABI_VERSION 4" in src


def test_wide_pass_flags():
    import pytest
    from tristage_rag_amd.index import wide_pass_flags
    assert wide_pass_flags("auto") == 0
    assert wide_pass_flags(True) == _lib.TS_FLAG_WIDE_PASSES
    assert wide_pass_flags(False) == _lib.TS_FLAG_NO_WIDE_PASSES
    for bad in ("on", 1, 0, None):
        with pytest.raises(ValueError):
            wide_pass_flags(bad)
