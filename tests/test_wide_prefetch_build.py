"""The wide scans' window loop keeps G B-operand register sets rolling: a set is re-read with the next ring slot's
operand as soon as its MFMA has issued, so an LDS read is G - 1 MFMAs ahead of its use.  The compiled loop shows it:
a v_mfma whose nearest preceding LDS wait is `s_waitcnt lgkmcnt(0)` waits for its own read.  The serial form gave
that for all 16 x G MFMAs of the window pair; the rolling form only for the last MFMA of each window, where no
later read is in flight.  All of it must fit the register file: the inline-asm corpus ring is correct only while
no instantiation, tombstone ones included, uses scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")
WIDE = re.compile(r"^_Z\d+(scan_wide_kernel|scan_wide_tomb_kernel)ILi(\d+)ELi(\d+)EEv")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(resource-usage remarks, device ISA) of ts_scan.hip, built as the library builds it."""
    out = tmp_path_factory.mktemp("wide_prefetch")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = str(out / "ts_scan.s")
    run = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                          "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                          os.path.join(CSRC, "ts_scan.hip"), "-o", asm],
                         cwd=str(out), capture_output=True, text=True, check=True)
    return run.stderr, open(asm).read()


def test_all_wide_kernels_use_no_scratch(compiled):
    remarks, _ = compiled
    found = {}
    name = None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and WIDE.match(name):
            found[name] = int(m.group(1))
    assert len(found) == 20, found   # plain / tombstone x f16 / bf16 x G = 2..6
    assert all(v == 0 for v in found.values()), found


def _kernels(isa):
    """name -> instruction lines of every wide instantiation"""
    out = {}
    name = None
    for line in isa.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1) if WIDE.match(m.group(1)) else None
            if name:
                out[name] = []
            continue
        if name:
            if line.startswith(".Lfunc_end"):
                name = None
            else:
                out[name].append(line.strip())
    return out


def test_mfmas_do_not_wait_for_their_own_read(compiled):
    _, isa = compiled
    kernels = _kernels(isa)
    assert len(kernels) == 20, sorted(kernels)
    for name, lines in kernels.items():
        G = int(WIDE.match(name).group(3))
        last = None    # lgkmcnt of the nearest preceding wait that names it
        mfmas, own = 0, 0
        for ins in lines:
            if ins.startswith("s_waitcnt"):
                m = re.search(r"lgkmcnt\((\d+)\)", ins)
                if m:
                    last = int(m.group(1))
            elif ins.startswith("v_mfma"):
                mfmas += 1
                assert last is not None, (name, "an MFMA before any LDS wait")
                if last == 0:
                    own += 1
        print(f"{name}: {mfmas} MFMAs, {own} after lgkmcnt(0)")
        assert mfmas == 16 * G, (name, mfmas)   # two windows of TS_RING = 8 slots
        # one per window of the pair (its last MFMA); every other MFMA follows a wait with lgkmcnt >= 1
        assert own <= 2, (name, own)
