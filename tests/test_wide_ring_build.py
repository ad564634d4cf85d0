"""scan_wide_kernel's corpus ring is inline asm whose destination registers fill in up to two windows after the load
statement: correct only while the compiler neither spills nor copies them.  It spills nothing at present; a change
that makes any wide instantiation use scratch must not build into the library unnoticed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")


def test_wide_kernels_use_no_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall",
                          "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "-c", "ts_scan.hip",
                          "-o", os.devnull], cwd=CSRC, capture_output=True, text=True, check=True).stderr
    found = {}
    name = None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "scan_wide_kernel" in name:
            found[name] = int(m.group(1))
    assert len(found) == 10, found   # f16 / bf16 x G = 2..6
    assert all(v == 0 for v in found.values()), found
