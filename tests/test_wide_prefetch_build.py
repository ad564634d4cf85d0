"""The wide scans' window loop keeps G B-operand register sets rolling: a set is re-read with the next ring slot's
operand as soon as its MFMA has issued, so an LDS read is G - 1 MFMAs ahead of its use.  The compiled loop shows it:
a v_mfma whose nearest preceding LDS wait is `s_waitcnt lgkmcnt(0)` waits for its own read.  The serial form gave
that for all 16 x G MFMAs of the window pair; the rolling form only for the last MFMA of each window, where no
later read is in flight.  All of it must fit the register file: scan_wide_kernel's corpus ring is inline asm whose
destination registers fill in up to two windows after the load statement, correct only while the compiler neither
spills nor copies them.  It spills nothing at present; a change that makes any coalesced instantiation
(scan_multi_kernel<DT, G, TOMB>, scan_wide_kernel<DT, G, TOMB>; TOMB: the tombstone passes of an index with removed
rows) use scratch must not build into the library unnoticed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")
# family, DT, G, TOMB
COALESCED = re.compile(r"^_Z\d+scan_(multi|wide)_kernelILi(\d+)ELi(\d+)ELb([01])EEv")
WIDE = re.compile(r"^_Z\d+scan_(wide)_kernelILi(\d+)ELi(\d+)ELb([01])EEv")


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


def test_coalesced_kernels_use_no_scratch(compiled):
    remarks, _ = compiled
    found = {}
    name = None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and COALESCED.match(name):
            found[name] = int(m.group(1))
    count = {}
    for name in found:
        family, _, _, tomb = COALESCED.match(name).groups()
        count[family, tomb] = count.get((family, tomb), 0) + 1
    # f16 / bf16 x G = 1..4 (multi), G = 2..6 (wide), each plain ("0") and tombstone ("1")
    assert count == {("multi", "0"): 8, ("multi", "1"): 8, ("wide", "0"): 10, ("wide", "1"): 10}, found
    assert len(found) == 36, found
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
