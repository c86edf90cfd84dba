"""tests/test_kernel_isa.py's checks, and the resource figures the kernel was accepted on, for persist_span_kernel -- the kernel a
static-camera batch of mode 0 runs (svo_persistent.hip.h), which the checks there do not select by name.  No GPU needed:
llvm-objdump / llvm-readelf read the gfx950 code object inside libsvohip.so."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools not installed")
    d = tmp_path_factory.mktemp("isa_span")
    so = shutil.copy(os.path.join(ROOT, "svo-raytracer_amd", "csrc", "libsvohip.so"), d)   # (--offloading writes next to its input)
    subprocess.check_call([OBJDUMP, "--offloading", so], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=d)
    co = [f for f in os.listdir(d) if "gfx950" in f]
    assert len(co) == 1, os.listdir(d)
    return os.path.join(d, co[0])


def _instructions(code_object, tab):
    txt = subprocess.check_output([OBJDUMP, "-d", code_object], text=True)
    want, name, ins = "persist_span_kernelILb%dEE" % tab, None, []
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m and not m.group(1).startswith("_Z"):
            continue   # a label of the inline assembly: still the same kernel
        if m:
            name = m.group(1)
        elif name and want in name and line.strip():
            ins.append(line.split()[0])
    assert ins, want
    return ins


def _metadata(code_object):
    """{kernel name: {key: int}} of the span kernels, from the code object's notes (one map per kernel, opening with `- .agpr_count`)"""
    notes = subprocess.check_output([READELF, "--notes", code_object], text=True)
    out, cur = {}, {}
    for line in notes.splitlines():
        if re.match(r"\s*- \.agpr_count:", line):
            cur = {}
        m = re.match(r"\s*(?:- )?\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        if m.group(2).isdigit():
            cur[m.group(1)] = int(m.group(2))
        elif m.group(1) == "name" and "persist_span_kernel" in m.group(2):
            out[m.group(2)] = cur
    return out


@pytest.mark.parametrize("tab", [0, 1])
def test_span_kernel_zeroes_a_new_ray_s_stack_column(code_object, tab):
    ins = _instructions(code_object, tab)
    levels = 2 * ins.count("ds_write2st64_b64") + ins.count("ds_write_b64")
    assert levels >= 12, {k: ins.count(k) for k in set(ins) if k.startswith("ds_")}
    assert ins.count("ds_write2_b32") >= 1   # the PUSH


def test_span_kernel_keeps_the_parent_kernel_s_resources(code_object):
    """what the kernel it replaces on the benchmark's path had: 80 VGPR and no AGPR (six waves per SIMD), the stack as the only LDS
    object (6 144 bytes), and no more than its 12 bytes of scratch per lane for the kernel that reads the row / column tables
    (the one a launch runs unless SVO_RC_TABLE=0 asks the variants library for the other); the spills that remain are round
    code: a handful of instructions, where a spill inside the traversal loop would show as a jump"""
    meta = _metadata(code_object)
    assert len(meta) == 2, sorted(meta)
    for name, m in meta.items():
        assert m["vgpr_count"] <= 80 and m["agpr_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 12 * 64 * 8, (name, m)
        if "ILb1EE" in name:
            assert m["private_segment_fixed_size"] <= 12, (name, m)
    spills = sum(1 for i in _instructions(code_object, 1) if i.startswith("scratch_"))
    assert spills <= 12, spills
