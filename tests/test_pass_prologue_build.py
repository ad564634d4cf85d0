"""scan_qstat_sample_kernel, the sample mode of the query-stationary pass, holds a group's whole query image in
registers as scan_qstat_kernel does.  The resource-usage remarks of ts_scan_qstat.hip, compiled as the library compiles
it, must show its four instantiations (f16 / bf16 x padded d = 640 / 768), each with no scratch and at most 256
registers (two waves per SIMD: one 8-wave workgroup per CU needs them).  Nothing else of the build is read."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")
SAMPLE = re.compile(r"^_Z\d+scan_qstat_sample_kernelILi(\d+)ELi(\d+)EEv")   # DT, NWIN


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("pass_prologue_build")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                          "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                          os.path.join(CSRC, "ts_scan_qstat.hip"), "-o", str(out / "ts_scan_qstat.o")],
                         cwd=str(out), capture_output=True, text=True, check=True)
    found = {}
    name = None
    for line in run.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1) if SAMPLE.match(m.group(1)) else None
            if name:
                found[name] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs|AGPRs): (\d+)", line)
        if m and name:
            found[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return found


def test_the_four_sample_instantiations(remarks):
    got = sorted(tuple(int(x) for x in SAMPLE.match(n).groups()) for n in remarks)
    assert got == [(1, 5), (1, 6), (2, 5), (2, 6)], sorted(remarks)   # TS_F16 = 1, TS_BF16 = 2; NWIN = 5, 6


def test_no_scratch_and_at_most_256_registers(remarks):
    assert len(remarks) == 4, sorted(remarks)
    for name, r in remarks.items():
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] + r["AGPRs"] <= 256, (name, r)
        assert r["Occupancy"] == 2, (name, r)
