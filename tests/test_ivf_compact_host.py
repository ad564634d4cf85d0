"""IVF compaction, host side (no GPU): ts_compact_ivf is declared, bound and exported within ABI version 4 and checks
its arguments before touching a device, its kernels live in their own source file and use no scratch, and the Python
surface exists."""
import ctypes
import os
import re
import subprocess

from tristage_rag_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")


def test_compact_ivf_is_declared_bound_and_exported_within_version_4():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tristage.h")).read(), flags=re.S)
    assert "ts_compact_ivf" in set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", text))
    assert "ts_compact_ivf" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ts_compact_ivf")
    assert not "ts_compact_ivf".startswith("ts_ivf_")   # (tests/test_ivf_host.py fixes that set of names)
    assert _lib.header_abi_version() == 4
    assert _lib.load().ts_abi_version() == 4


def test_compact_ivf_arguments_are_checked_without_a_gpu():
    lib = _lib.load()
    assert lib.ts_compact_ivf(None, None, None) == _lib.TS_ERR_INVALID
    assert "bad arguments" in _lib.last_error()
    out = (ctypes.c_int64 * 4)()
    assert lib.ts_compact_ivf(None, out, None) == _lib.TS_ERR_INVALID


def test_compaction_kernels_have_their_own_file_and_use_no_scratch():
    assert "ts_ivf_compact.hip" in open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                          "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "-c", "ts_ivf_compact.hip",
                          "-o", os.devnull], cwd=CSRC, capture_output=True, text=True, check=True).stderr
    kernels, found, name = set(), {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels.add(name)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and re.search(r"ivfc_\w+_kernel", name):
            found[name] = int(m.group(1))
    assert len(found) == 3, found   # classify, tables, move
    assert set(found) == kernels    # every kernel of the file carries the prefix
    assert all(v == 0 for v in found.values()), found
    # and none of them is counted among the removal or the update kernels (test_remove_host.py and
    # test_update_host.py fix those sets)
    removal = r"(live_set|live_clear|and_live|word_count|tile_scan|word_scan|compact_map|compact_gather|ivf_remove)_kernel"
    assert not [n for n in found if re.search(removal, n) or re.search(r"upd_\w+_kernel", n)]


def test_python_surface_exists():
    from tristage_rag_amd.index import FlatIPIndex, IVFFlatIndex
    from tristage_rag_amd.stage1_retriever import Stage1Retriever
    import inspect
    assert callable(IVFFlatIndex.compact)
    assert inspect.signature(IVFFlatIndex.compact) == inspect.signature(FlatIPIndex.compact)
    assert "NotImplementedError" not in inspect.getsource(Stage1Retriever.remove_documents)
