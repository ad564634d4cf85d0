"""The ring of the query-stationary passes without a GPU (tristage-rag_amd/csrc/ts_scan_qstat_ring.h):
tests/qstat_ring.hip, a stand-alone program, takes the arithmetic the kernels use (the slot of a window, the source of
the n-th request, the main/tail split of the walk, the counted wait) through every walk of 1..64 steps at both widths,
on grids whose workgroups differ by one step, and checks that every window is requested exactly once into slot
W % depth from its bytes of the corpus, that requests past the walk read the dead address, that no slot is restaged
before the barrier after its last read, that block s + 1 has landed when step s waits, and that every step issues NWIN
requests.  It runs once as built plainly and once with the host compile under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")


def _build_and_run(tmp, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp / name)
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-I", CSRC,
                    *extra, os.path.join(ROOT, "tests", "qstat_ring.hip"), "-o", exe],
                   capture_output=True, text=True, check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("qstat_ring")


def _held(run):
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok"
    seen = set()
    for l in lines[:-1]:
        m = re.fullmatch(r"nwin=(\d) depth=15 lead=(\d) grid=(\d+) blk0=\d+ stride=\d+ walks=(\d+) requests=(\d+)", l)
        assert m, l
        nwin, lead, grid, walks, requests = (int(x) for x in m.groups())
        assert lead == 15 - 2 * nwin
        assert walks >= 64 and requests > walks * 15   # (a vacuous run would print zeros)
        seen.add((nwin, grid))
    assert {(5, 1), (6, 1), (5, 256), (6, 256)} <= seen


def test_every_walk_holds(tmp):
    _held(_build_and_run(tmp, "qstat_ring", []))


def test_every_walk_holds_under_host_sanitizers(tmp):
    run = _build_and_run(tmp, "qstat_ring_san", ["-Xarch_host", "-fsanitize=address,undefined",
                                                  "-Xarch_host", "-fno-sanitize-recover=all"])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    _held(run)
