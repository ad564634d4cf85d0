"""Coalesced passes, host side (no GPU): groups per pass by dimension, and the flag / ABI the binding uses."""
import re

from tristage_rag_amd import _lib


def test_groups_per_pass_follow_the_lds_budget():
    lib = _lib.load()
    f16, bf16, f32 = 1, 2, 0
    # padded dimension <= 512: 4 groups; 640 and 768: 3; from 896: 2 (no coalescing)
    for d, g in ((64, 4), (384, 4), (512, 4), (513, 3), (640, 3), (768, 3), (769, 2), (896, 2), (1024, 2)):
        assert lib.ts_coalesce_groups(d, f16) == g, d
        assert lib.ts_coalesce_groups(d, bf16) == g, d
    assert lib.ts_coalesce_groups(768, f32) == 0   # fp32 storage has no multi-group scan
    assert lib.ts_coalesce_groups(0, f16) == 0


def test_flag_and_abi():
    src = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define\s+TS_FLAG_COALESCE\s+(\d+)u", src).group(1)) == _lib.TS_FLAG_COALESCE == 128
    for name in ("ts_index_flush", "ts_coalesce_groups"):
        assert name in _lib.SIGNATURES
    used = {_lib.TS_FLAG_HOST_PTR, _lib.TS_FLAG_NO_FILTER, _lib.TS_FLAG_NORMALIZE, _lib.TS_FLAG_ASYNC,
            _lib.TS_FLAG_PIPELINE, _lib.TS_FLAG_CLASSIC, _lib.TS_FLAG_ONE_LAUNCH}
    assert _lib.TS_FLAG_COALESCE not in used


def test_index_defaults_to_coalescing_and_sharded_never_does():
    import inspect
    from tristage_rag_amd import index, sharded
    assert "self.coalesce = True" in inspect.getsource(index.FlatIPIndex.__init__)
    assert "coalesce = False" in inspect.getsource(sharded.ShardedFlatIPIndex.__init__)
