"""Static guard (no GPU): what a workgroup of the frame stream's step kernels
executes before its first work item, and what it keeps in spilled scalars.

A workgroup of the wide integrate role (IntegrateRoleWide in vbg_stream.hip)
has about one work item, so whatever the compiler hoists out of the item loop
is paid per item. Before round 11 every workgroup began with 113-120 vector
instructions (the role dispatch, three integer reciprocals -- v_rcp_iflag_f32
with their Newton steps -- for divisions that only a non-power-of-two
resolution takes, and 17-21 v_writelane of scalars that did not fit), and a
work item read 10-12 of those scalars back with v_readlane. The source now
works the divisors out in the path that divides and reads the per-item
parameters per item, both behind a zero the optimiser cannot see through;
each of those spots pins a hoisting decision of one compiler version, so this
test reads the assembly and fails if the old shape returns.

The item loop's top is marked by that zero's empty inline assembly, the first
`;;#ASMSTART` of the kernel. Bounds (from the parent commit's figures, not
from today's): before the marker
  * no reciprocal at all (they were 4);
  * at most 60 vector instructions -- the parent's 113-120 less the ~28 of the
    reciprocals' sequences and the ~20 spills is 65-70: below that, both are
    gone (today 21-26);
  * at most 8 v_writelane (17-21 before; today 0-4);
and in the whole kernel at most 21 v_readlane: the parent's 31-33 less the
10-12 of the work item's header (today 15)."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open3d_amd", "csrc")

STEP = re.compile(r"FrameStepKernel(?:Proven)?I(?:tt|ff)Lb[01]ELi[02]E")
MAX_PROLOGUE_VALU, MAX_PROLOGUE_WRITELANE, MAX_READLANE = 60, 8, 21


def _bodies(asm):
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n", asm, re.M):
        end = asm.find(".Lfunc_end", m.end())
        out[m.group(1)] = asm[m.end():end].splitlines()
    return out


def item_loop_figures(lines):
    """(vector instructions, reciprocals, v_writelane) before the kernel's
    first inline-assembly marker, and the kernel's v_readlane count"""
    ops, marker = [], None
    for ln in lines:
        t = ln.strip()
        if t.startswith(";;#ASMSTART") and marker is None:
            marker = len(ops)
        code = t.split(";")[0].strip()
        if code.startswith("v_"):
            ops.append(code.split()[0])
    assert marker is not None, "no inline-assembly marker in the kernel"
    pre = ops[:marker]
    return (len(pre), sum(o.startswith("v_rcp") for o in pre),
            sum(o.startswith("v_writelane") for o in pre),
            sum(o.startswith("v_readlane") for o in ops))


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


def test_step_kernels_start_their_work_item_without_loop_constant_setup(
        stream_asm):
    seen = {}
    for name, lines in _bodies(stream_asm).items():
        if STEP.search(name):
            seen[name] = item_loop_figures(lines)
    assert len(seen) == 12, sorted(seen)  # 3 forms x colour x state type
    print(seen)
    bad = {k: v for k, v in seen.items()
           if v[0] > MAX_PROLOGUE_VALU or v[1] != 0 or
           v[2] > MAX_PROLOGUE_WRITELANE or v[3] > MAX_READLANE}
    assert not bad, bad


def test_scanner_on_a_made_up_listing():
    lines = ["\tv_mov_b32_e32 v1, 0", "\tv_rcp_iflag_f32_e32 v2, v2",
             "\tv_writelane_b32 v68, s2, 0", "\ts_nop 0 ; v_fake",
             "\t;;#ASMSTART", "\t;;#ASMEND", "\tv_readlane_b32 s2, v68, 0",
             "\t;;#ASMSTART", "\tv_min_f32 v1, s2, v3", "\t;;#ASMEND"]
    assert item_loop_figures(lines) == (3, 1, 1, 1)
    with pytest.raises(AssertionError):
        item_loop_figures(lines[:4])
