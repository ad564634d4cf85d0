"""The step loop of scan_qstat_kernel, as compiled (DESIGN.md 4.2c "step tail"): between two blocks of MFMAs a wave
issues the group maximum, one counted wait with an immediate count, the barrier and the step's NWIN requests, and the
ring's state moves by scalar additions.  ts_scan_qstat.hip is compiled as the library compiles it, to assembly, and the
main loop of each of the four instantiations (the first loop that holds MFMAs) is read.  No GPU.

What is counted.  The loop's blocks are the ones the compiler's own block comments put under the loop's header.  The
"straight" blocks are those that can be reached from the header without entering a block that narrows the execution
mask (s_and_saveexec_b64): that leaves out the survivor path's staging code, in line or out of line, and nothing else,
since every other branch of the loop is wave-uniform.  All figures below are taken over the straight blocks."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tristage-rag_amd", "csrc")
KERNEL = re.compile(r"^(_Z17scan_qstat_kernelILi(\d+)ELi(\d+)EEv14WideScanParamsi+):")
BLOCK = re.compile(r"^(?:(\.LBB\d+_\d+):|; %bb\.(\d+):)")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")

# straight_other() of scan_qstat_kernel<f16, 6> and <f16, 5> as compiled from the commit before the step tail became
# straight-line (9235327, "Stage-1 scans: one launch rule, dtype dispatch and ingest geometry"), by this file's
# loop_figures(): the figure the issue asks to halve.  (Both dtypes compile to the same counts.)
PARENT_STRAIGHT_OTHER = {6: 453, 5: 400}   # (with 61 and 57 branches, 54 and 45 scalar multiplies, 9 vmcnt waits)


def kernels(asm):
    """{(DT, NWIN): lines of the kernel's body}"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = KERNEL.match(line)
        if m:
            cur = out.setdefault((int(m.group(2)), int(m.group(3))), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        if cur is not None:
            cur.append(line)
    return out


def blocks_of(lines):
    """[(name, header_of_its_loop or None, is_header, [(mnemonic, operands)])] in text order"""
    out = []
    for line in lines:
        m = BLOCK.match(line)
        if m:
            name = m.group(1) or "bb." + m.group(2)
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", line)
            out.append([name, ".L" + h.group(1) if h else None, "Loop Header" in line, []])
            continue
        m = INSTR.match(line)
        if m and out and not m.group(1).startswith("sched_barrier"):
            out[-1][3].append((m.group(1), m.group(2).strip()))
    return out


def loop_figures(lines):
    """The figures of the kernel's main loop: the first loop, in text order, that holds MFMAs."""
    blocks = blocks_of(lines)
    headers = [b[0] for b in blocks if b[2]]
    for header in headers:
        member = [i for i, b in enumerate(blocks) if b[0] == header or b[1] == header]
        if any(op.startswith("v_mfma") for i in member for op, _ in blocks[i][3]):
            break
    else:
        raise AssertionError("no loop with MFMAs")
    inside = set(member)
    index = {blocks[i][0]: i for i in member}

    def successors(i):
        succ = []
        for op, args in blocks[i][3]:
            if op.startswith("s_cbranch") or op == "s_branch":
                t = args.split()[-1]
                if t in index:
                    succ.append(index[t])
                if op == "s_branch":
                    return succ
            if op == "s_endpgm":
                return succ
        if i + 1 in inside:
            succ.append(i + 1)
        return succ

    narrows = {i for i in member if any(op == "s_and_saveexec_b64" for op, _ in blocks[i][3])}
    straight, todo = set(), [index[header]]
    while todo:
        i = todo.pop()
        if i in straight or i in narrows:
            continue
        straight.add(i)
        todo.extend(successors(i))
    ins = [x for i in sorted(straight) for x in blocks[i][3]]
    every = [x for i in member for x in blocks[i][3]]

    def n(pred, seq=ins):
        return sum(1 for op, args in seq if pred(op, args))

    barriers = n(lambda op, a: op == "s_barrier")
    excluded = n(lambda op, a: op.startswith("v_mfma") or op == "ds_read_b128" or
                 (op == "s_waitcnt" and "lgkmcnt" in a and "vmcnt" not in a and "expcnt" not in a))
    return {
        "barriers": barriers,
        "mfma": n(lambda op, a: op.startswith("v_mfma")),
        "mfma_whole_loop": n(lambda op, a: op.startswith("v_mfma"), every),
        "requests": n(lambda op, a: op == "global_load_lds_dwordx4"),
        "requests_whole_loop": n(lambda op, a: op == "global_load_lds_dwordx4", every),
        "vmcnt_waits": [a for op, a in ins if op == "s_waitcnt" and "vmcnt" in a],
        "scalar_multiplies": n(lambda op, a: op.startswith("s_mul")),
        "branches": n(lambda op, a: op.startswith("s_cbranch") or op == "s_branch"),
        "straight_other": len(ins) - excluded,
        "staging_blocks": len(member) - len(straight),
    }


def compile_to_asm(src, out_dir):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(str(out_dir), "ts_scan_qstat.s")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                    "--cuda-device-only", "-S", src, "-o", out], cwd=str(out_dir), capture_output=True, text=True,
                   check=True)
    return open(out).read()


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    asm = compile_to_asm(os.path.join(CSRC, "ts_scan_qstat.hip"), tmp_path_factory.mktemp("qstat_tail_build"))
    found = {k: loop_figures(v) for k, v in kernels(asm).items()}
    assert sorted(found) == [(1, 5), (1, 6), (2, 5), (2, 6)], sorted(found)
    for k, f in sorted(found.items()):
        print(k, f)
    return found


def test_the_main_loop_holds_whole_steps(figures):
    for (dt, nwin), f in figures.items():
        u = f["barriers"]
        assert u >= 1, (dt, nwin, f)
        assert f["mfma"] == nwin * 8 * u and f["mfma_whole_loop"] == f["mfma"], (dt, nwin, f)
        assert f["requests"] == nwin * u and f["requests_whole_loop"] == f["requests"], (dt, nwin, f)
        assert f["staging_blocks"] >= 16, (dt, nwin, f)   # (else "straight" left nothing out and the counts mean less)


def test_one_counted_wait_with_an_immediate_per_step(figures):
    for (dt, nwin), f in figures.items():
        assert len(f["vmcnt_waits"]) == f["barriers"], (dt, nwin, f)
        for w in f["vmcnt_waits"]:
            assert w.replace(" ", "") == "vmcnt(%d)" % (15 - 2 * nwin), (dt, nwin, f)


def test_no_scalar_multiply_and_few_branches(figures):
    for (dt, nwin), f in figures.items():
        assert f["scalar_multiplies"] == 0, (dt, nwin, f)
        # the group test, the 16 per-register tests, the owner test, the back edge and one to spare
        assert f["branches"] <= 20 * f["barriers"], (dt, nwin, f)


def test_the_step_tail_is_at_most_half_of_what_it_was(figures):
    """Every instruction of the straight blocks per barrier, without the MFMAs, the ds_read_b128 and their lgkmcnt
    waits, against the same count of the parent's kernel."""
    for (dt, nwin), f in figures.items():
        per_step = f["straight_other"] / f["barriers"]
        print((dt, nwin), per_step, PARENT_STRAIGHT_OTHER[nwin])
        assert 2 * per_step <= PARENT_STRAIGHT_OTHER[nwin], (dt, nwin, f)
