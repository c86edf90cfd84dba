"""tests/test_kernel_isa_span.py's checks for the two kernels of the primary-hit cache (persist_kept_kernel<true>, the fill, and
persist_kept_kernel<false>, the reuse; svo_persistent.hip.h), which a still camera's submissions run instead of
persist_span_kernel.  No GPU needed: llvm-objdump / llvm-readelf read the gfx950 code object inside libsvohip.so."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

# scratch instructions of the build this was accepted on: fill 5, reuse 3 (all of them round code: spilled once per round, not
# per trip); "plus a few" for a compiler that places them differently
SCRATCH_CAP = {1: 5 + 4, 0: 3 + 4}


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools not installed")
    d = tmp_path_factory.mktemp("isa_kept")
    so = shutil.copy(os.path.join(ROOT, "svo-raytracer_amd", "csrc", "libsvohip.so"), d)   # (--offloading writes next to its input)
    subprocess.check_call([OBJDUMP, "--offloading", so], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=d)
    co = [f for f in os.listdir(d) if "gfx950" in f]
    assert len(co) == 1, os.listdir(d)
    return os.path.join(d, co[0])


@pytest.fixture(scope="module")
def instructions(code_object):
    """{fill (1 / 0): mnemonics of persist_kept_kernel<fill>, "cast": of persist_cast_kernel (the same draw, no shading)}"""
    txt = subprocess.check_output([OBJDUMP, "-d", code_object], text=True)
    out, name = {0: [], 1: [], "cast": []}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m and not m.group(1).startswith("_Z"):
            continue   # a label of the inline assembly: still the same kernel
        if m:
            name = m.group(1)
        elif name and line.strip():
            for fill in (0, 1):
                if "persist_kept_kernelILb%dEE" % fill in name:
                    out[fill].append(line.split()[0])
            if "persist_cast_kernel" in name:
                out["cast"].append(line.split()[0])
    assert out[0] and out[1] and out["cast"]
    return out


def _metadata(code_object):
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
        elif m.group(1) == "name" and ("persist_kept_kernel" in m.group(2) or "persist_cast_kernel" in m.group(2)):
            out[m.group(2)] = cur
    return out


@pytest.mark.parametrize("fill", [0, 1, "cast"])
def test_kept_kernel_zeroes_a_new_ray_s_stack_column(instructions, fill):
    ins = instructions[fill]
    levels = 2 * ins.count("ds_write2st64_b64") + ins.count("ds_write_b64")
    assert levels >= 12, {k: ins.count(k) for k in set(ins) if k.startswith("ds_")}
    assert ins.count("ds_write2_b32") >= 1   # the PUSH


def test_kept_kernels_keep_six_waves_per_simd_and_the_stack_as_their_only_lds(code_object):
    meta = _metadata(code_object)
    assert len(meta) == 3, sorted(meta)
    for name, m in meta.items():
        assert m["vgpr_count"] <= 80 and m["agpr_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 12 * 64 * 8, (name, m)


@pytest.mark.parametrize("fill", [0, 1])
def test_kept_kernel_spills_in_round_code_only(instructions, fill):
    """a tripwire: a spill inside the traversal loop would show as a jump in this count"""
    spills = sum(1 for i in instructions[fill] if i.startswith("scratch_"))
    print("persist_kept_kernel<%d>: %d scratch instructions" % (fill, spills))
    assert spills <= SCRATCH_CAP[fill], spills
