"""Query-stationary coalesced passes, host side (no GPU): where the kernel exists, the flags and entry point the binding
uses, and the policy attribute's values."""
import re

import pytest

from tristage_rag_amd import _lib

F32, F16, BF16, FP8 = 0, 1, 2, 3


def test_groups_per_stationary_pass():
    lib = _lib.load()
    for dt in (F16, BF16):
        for d in (576, 640, 700, 768, 513):
            assert lib.ts_coalesce_groups_stationary(d, dt) == 8, (d, dt)
        for d in (384, 512, 769, 1024, 2048, 0, -3):
            assert lib.ts_coalesce_groups_stationary(d, dt) == 0, (d, dt)
    for d in (640, 768):
        assert lib.ts_coalesce_groups_stationary(d, F32) == 0
        assert lib.ts_coalesce_groups_stationary(d, FP8) == 0
    # the other widths are unchanged
    for d in (64, 384, 700, 768, 1024):
        assert lib.ts_coalesce_groups_wide(d, F16) == 6 and lib.ts_coalesce_groups_wide(d, BF16) == 6
    assert [lib.ts_coalesce_groups(d, F16) for d in (384, 768, 1024)] == [4, 3, 2]


def test_header_and_binding_agree():
    src = open(_lib.HEADER_PATH).read()
    for name in ("TS_FLAG_STATIONARY_PASSES", "TS_FLAG_NO_STATIONARY_PASSES"):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, src).group(1)) == getattr(_lib, name)
    every = [int(v) for v in re.findall(r"^#define\s+TS_FLAG_\w+\s+(\d+)u", src, flags=re.M)]
    assert len(every) == len(set(every)) and all(v & (v - 1) == 0 for v in every), every   # distinct single bits
    assert (_lib.TS_FLAG_STATIONARY_PASSES, _lib.TS_FLAG_NO_STATIONARY_PASSES) == (1024, 2048)
    assert re.search(r"int32_t\s+ts_coalesce_groups_stationary\(int32_t dim, int32_t storage_dtype\);", src)
    assert "ts_coalesce_groups_stationary" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["ts_coalesce_groups_stationary"]
    assert (restype, argtypes) == _lib.SIGNATURES["ts_coalesce_groups_wide"]
    assert "#define TS_ABI_VERSION 4" in src


def test_stationary_pass_flags():
    from tristage_rag_amd.index import stationary_pass_flags, wide_pass_flags
    assert stationary_pass_flags("auto") == 0
    assert stationary_pass_flags(True) == _lib.TS_FLAG_STATIONARY_PASSES
    assert stationary_pass_flags(False) == _lib.TS_FLAG_NO_STATIONARY_PASSES
    for bad in ("on", "AUTO", 1, 0, None, 8):
        with pytest.raises(ValueError):
            stationary_pass_flags(bad)
    assert wide_pass_flags(True) | wide_pass_flags(False) == 768   # untouched
