"""The launch geometry of the ring scan (ts_scan_dev.h ``ts_scan_admits`` / ``ts_scan_geom``): the one
host function every stage-1 format's launcher takes its LDS byte count and grid from, held to the rule as it was
written in each format's own launcher before they were merged.  A stand-alone program (tests/scan_launch_geom.hip,
no HIP call) prints it for every format, dimension, query-half count, mode and walk; no GPU is needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")
LDS = 160 * 1024
SCAN_WAVES = 8
NUM_CUS = 256
DIMS = (16, 128, 768, 1024, 1040, 2048, 4096)
NWORK = (1, 8, 9, 100000)
DENSE, FILTER = 0, 1


def _pad(d, q):
    return (d + q - 1) // q * q


def image_kib(fmt, d):
    """KiB of the query image per 32 queries, from the layouts of ts_common.h."""
    if fmt in ("f16", "bf16"):
        return _pad(d, 128) // 16          # kg: 16 dimensions per k group, rings of 8
    if fmt == "f32":
        return _pad(d, 64) // 8            # kg: 8 dimensions per k group
    if fmt == "fp8":
        return 2 * (_pad(d, 256) // 32)    # the bf16 image of the padded dimension: 2 * kg
    if fmt == "fp4":
        return 4 * (_pad(d, 256) // 64)    # the bf16 image of the padded dimension: 4 per code unit
    raise ValueError(fmt)


def expected_lines(stage):
    """Every line the program prints, from the rule restated."""
    out = []
    for masked in (0, 1):
        combos = []
        for d in DIMS:
            for fmt in ("f16", "bf16", "f32", "fp8", "fp4"):
                if (fmt == "f32" and masked) or (fmt == "fp4" and d > 2048):
                    continue
                combos.append((fmt, d, image_kib(fmt, d)))
        combos += [("prefix", 16 * kg, kg) for kg in (8, 16, 48)]
        for fmt, d, kib in combos:
            for qh in (1, 2):
                for mode in (DENSE, FILTER):
                    head = f"{fmt} d={d} kib={kib} qh={qh} mode={mode} masked={masked}"
                    if kib * qh * 1024 + stage > LDS:      # admission: the filter form has to fit
                        out.append(head + " refused")
                        continue
                    flt = mode == FILTER or masked         # a masked walk is filter-only
                    lds = kib * qh * 1024 + (stage if flt else 0)
                    wg = 2 if (not flt and 2 * lds <= LDS) else 1
                    for nwork in NWORK:
                        grid = min(max((nwork + SCAN_WAVES - 1) // SCAN_WAVES, 1), NUM_CUS * wg)
                        out.append(f"{head} nwork={nwork} -> mode={FILTER if flt else DENSE} lds={lds} grid={grid}")
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path_factory.mktemp("scan_launch") / "scan_launch_geom")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-I", CSRC,
                    os.path.join(ROOT, "tests", "scan_launch_geom.hip"), "-o", exe],
                   capture_output=True, text=True, check=True)
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()


def test_geometry_is_the_rule_of_the_former_launchers(printed):
    m = re.fullmatch(r"stage (\d+)", printed[0])
    assert m, printed[0]
    stage = int(m.group(1))
    assert 0 < stage < LDS
    want = expected_lines(stage)
    assert len(printed) - 1 == len(want)
    for got, exp in zip(printed[1:], want):
        assert got == exp


def test_the_cases_cover_both_sides_of_every_rule(printed):
    """Refusals, one and two workgroups per CU, grids at, below and above their cap, and masked walks asked for a dense
    scan all occur among the printed cases (else the comparison above would hold vacuously)."""
    body = printed[1:]
    assert any(l.startswith("f16 d=2048 ") and "qh=2" in l and l.endswith("refused") for l in body)
    assert any(l.startswith("f16 d=2048 ") and "qh=1" in l and "grid=" in l for l in body)
    grids = {int(l.rsplit("grid=", 1)[1]) for l in body if "grid=" in l}
    assert {1, 2, NUM_CUS, 2 * NUM_CUS} <= grids
    assert any(" mode=0 masked=1 " in l and "-> mode=1 " in l for l in body)
    assert not any("masked=1" in l and "-> mode=0" in l for l in body)
    # no request exceeds the LDS, and a filter request always has room for the staging behind the image
    stage = int(printed[0].split()[1])
    for l in body:
        if "lds=" in l:
            lds = int(re.search(r"lds=(\d+)", l).group(1))
            kib, qh = (int(x) for x in re.search(r"kib=(\d+) qh=(\d+)", l).groups())
            assert lds <= LDS
            assert lds == kib * qh * 1024 + (stage if "-> mode=1" in l else 0)
