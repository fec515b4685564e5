"""Static guard (no GPU): the integrate role's rounds keep their record
gathers in flight together.

A round of the wide integrate role (IntegrateRoleWide in vbg_stream.hip)
projects the lane's voxels into kGroupChunk frames and requests one 8-byte
record per voxel and frame, then applies the frames from registers. The
gathers of a round are meant to be outstanding at the same time, so that a
round costs ONE memory round trip. hipcc's wait-count pass used to put an
`s_waitcnt vmcnt(0)` at the top of every frame's issue block (the frames sit
behind wave-uniform branches and the previous round's record registers are
reused as temporaries), which turned a round into kGroupChunk dependent round
trips. This test reads the assembly and fails if any vmcnt wait sits between
the first and the last record gather of a round."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open3d_amd", "csrc")

# a record gather: a global load from a wave-uniform base (scalar register
# pair) at a per-lane 32-bit offset
GATHER = re.compile(
    r"^global_load_(?:dword|dwordx2)\s+v(?:\d+|\[\d+:\d+\]),\s*v\d+,\s*s\[\d+:\d+\]")
VMWAIT = re.compile(r"^s_waitcnt\b.*\bvmcnt\(\d+\)")
LOOP = re.compile(r"in Loop: Header=(\S+) Depth=(\d+)")
BLOCK = re.compile(r"^(?:\.LBB\d+_\d+:|; %bb\.\d+:)")

# The forms the headline and the chunk launch's records path run in: the
# frame stream's step kernel with colour (<weight, colour, kColor = true,
# kDiv = 2>) and the chunk launch's records form with colour. (The colourless
# and raw-image forms gather 4- / 2-byte values into single registers; the
# register allocator can pair such a register with a packed operand of the
# next frame's projection, which then waits for that one load. Not covered.)
FORMS = {
    "step": r"FrameStepKernelI(?:tt|ff)Lb1ELi2E",
    "chunk_records": r"ChunkIntegrateKernelI(?:tt|ff)Lb1ELi2ELb0E",
}


def _group_chunk():
    src = open(os.path.join(CSRC, "stream_path.h")).read()
    return int(re.search(r"constexpr int kGroupChunk = (\d+);", src).group(1))


def _bodies(asm):
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n", asm, re.M):
        end = asm.find(".Lfunc_end", m.end())
        out[m.group(1)] = asm[m.end():end].splitlines()
    return out


def round_loop_events(lines):
    """innermost loop (header label, depth) -> the record gathers and vmcnt
    waits of its basic blocks, in layout order"""
    loops, cur = {}, None
    for ln in lines:
        if BLOCK.match(ln):
            h = LOOP.search(ln)
            cur = (h.group(1), int(h.group(2))) if h else None
            continue
        code = ln.split(";")[0].strip()
        if cur is not None and (GATHER.match(code) or VMWAIT.match(code)):
            loops.setdefault(cur, []).append(code)
    return loops


def waits_inside_rounds(asm, name_pattern, gathers_per_round):
    """kernel -> vmcnt waits found between the first and the last record
    gather of its round loop (the loop holding >= gathers_per_round gathers)"""
    out = {}
    for name, lines in _bodies(asm).items():
        if not re.search(name_pattern, name):
            continue
        rounds = []
        for ev in round_loop_events(lines).values():
            g = [i for i, t in enumerate(ev) if GATHER.match(t)]
            if len(g) >= gathers_per_round:
                rounds.append([t for t in ev[g[0]:g[-1]] if VMWAIT.match(t)])
        assert len(rounds) == 1, (name, len(rounds))
        out[name] = rounds[0]
    return out


@pytest.fixture(scope="module")
def stream_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc here: the ISA guard needs the compiler")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    out = str(tmp_path_factory.mktemp("isa") / "vbg_stream.s")
    return open(isa_scan.compile_to_asm(
            os.path.join(CSRC, "vbg_stream.hip"), out)).read()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_round_issues_all_record_gathers_before_any_wait(stream_asm, form):
    # kV = 2 voxels per lane: 2 record gathers per frame of the round
    per_round = 2 * _group_chunk()
    found = waits_inside_rounds(stream_asm, FORMS[form], per_round)
    assert len(found) == 2, sorted(found)  # float and uint16 state
    bad = {k: v for k, v in found.items() if v}
    assert not bad, bad


def test_round_scanner_on_a_made_up_listing():
    """The scanner itself: gathers of one loop with a wait between them are
    reported, a wait after the last gather (the round's apply) is not."""
    def listing(mid):
        return "\n".join([
            "_ZN5o3dmi4KernEv: ; @k",
            ".LBB0_1: ; =>This Inner Loop Header: Depth=1",
            "\ts_nop 0",
            ".LBB0_2: ;   in Loop: Header=BB0_1 Depth=1",
            "\tglobal_load_dwordx2 v[16:17], v16, s[12:13]",
            "\tglobal_load_dwordx2 v[24:25], v24, s[12:13]",
            mid,
            "; %bb.3: ;   in Loop: Header=BB0_1 Depth=1",
            "\tglobal_load_dwordx2 v[18:19], v18, s[12:13]",
            "\tglobal_load_dwordx2 v[26:27], v26, s[12:13]",
            "\ts_waitcnt vmcnt(1)",
            "\ts_waitcnt vmcnt(0)",
            ".LBB0_4:",
            "\tglobal_load_dwordx4 v[2:5], v51, s[4:5]",
            "\ts_waitcnt vmcnt(0)",
            ".Lfunc_end0:"])
    assert waits_inside_rounds(listing("\tv_mov_b32 v1, 0"), "Kern", 4) == \
        {"_ZN5o3dmi4KernEv": []}
    assert waits_inside_rounds(listing("\ts_waitcnt lgkmcnt(0)"), "Kern", 4) \
        == {"_ZN5o3dmi4KernEv": []}
    assert waits_inside_rounds(
            listing("\ts_waitcnt vmcnt(0) lgkmcnt(0)"), "Kern", 4) == \
        {"_ZN5o3dmi4KernEv": ["s_waitcnt vmcnt(0) lgkmcnt(0)"]}
