"""The pure half of the dense pass's ray list (svo-raytracer_amd/csrc/svo_persist_plan.h; PersistSettings::list_mode, on by default):
ray_run_reserve / ray_run_take, the arithmetic of persist_runs_kernel's draw; ray_region, the bands' regions of the ray records.  (The
list is compacted, not ordered: no key on a ray's direction is shipped, so none is tested.)
tests/ray_list_cases.cpp, a host program, prints the cases; the expected values below are worked out by hand.  The program is also
built once with -fsanitize=address,undefined and must run clean and print the same."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ray_list_cases.cpp")
INC = os.path.join(ROOT, "svo-raytracer_amd", "csrc")


def _build_and_run(exe, extra=()):
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", *extra, "-I", INC, SRC, "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("ray_list") / "ray_list_cases").stdout.splitlines()


def _fields(line):
    return dict(f.split("=") for f in line.split()[1:] if "=" in f)


@pytest.fixture(scope="module")
def consts(lines):
    (ln,) = [l for l in lines if l.startswith("const ")]
    return {k: int(v) for k, v in _fields(ln).items()}


def test_every_entry_below_the_fill_is_handed_out_exactly_once(lines, consts):
    chunk = consts["chunk"]
    runs = [_fields(ln) for ln in lines if ln.startswith("run ")]
    fills = sorted({int(r["fill"]) for r in runs})
    assert fills == sorted({0, 1, chunk - 1, chunk, chunk + 1, 3000, 7777})
    assert len(runs) == len(fills) * 3 * 3
    for r in runs:
        r = {k: int(v) for k, v in r.items()}
        assert r["handed"] == r["fill"] and r["twice"] == 0 and r["beyond"] == 0 and r["missed"] == 0, r
        # one atomic per chunk, and at most one per wave that finds the band used up
        assert r["reservations"] <= r["fill"] // chunk + 1 + r["waves"], r
        assert r["reservations"] >= -(-r["fill"] // chunk), r


@pytest.mark.parametrize("w,h", [(76, 44), (76, 8), (1920, 1080)])
@pytest.mark.parametrize("frames", [2, 4, 7])
def test_band_regions_tile_the_ray_records(lines, w, h, frames):
    (ln,) = [l for l in lines if l.startswith("region %dx%dx%d " % (w, h, frames))]
    d = _fields(ln)
    tiles_y = (h + 7) // 8
    rows_per_band = (tiles_y + 7) // 8
    assert int(d["dense"]) == 1 and int(d["list"]) == 1 and int(d["rows_per_band"]) == rows_per_band
    assert int(d["records"]) == tiles_y * 8 * w * frames
    bands = [tuple(int(v) for v in b.split(":")) for b in d["bands"].split(",")]
    assert len(bands) == 8
    at = 0
    for b, (first, room) in enumerate(bands):
        rows = min(max(tiles_y - b * rows_per_band, 0), rows_per_band)
        assert first == at, (b, bands)                         # no gap, no overlap
        assert room == rows * 8 * w * frames, (b, bands)       # the band's pixels x frames; a band with no rows is empty
        at += room
    assert at == int(d["records"])


def test_regions_by_hand(lines):
    by = {ln.split()[1]: _fields(ln) for ln in lines if ln.startswith("region ")}
    assert by["76x8x4"]["bands"] == "0:2432," + ",".join(["2432:0"] * 7)
    assert by["76x44x2"]["bands"] == "0:1216,1216:1216,2432:1216,3648:1216,4864:1216,6080:1216,7296:0,7296:0"
    # 135 tile rows: seven bands of 17, one of 16; a tile row of 4 frames = 8 x 1920 x 4 records
    assert by["1920x1080x4"]["bands"].split(",")[7] == "%d:%d" % (119 * 61440, 16 * 61440)
    assert int(by["1920x1080x4"]["records"]) * 24 == 199_065_600


def test_what_does_not_fit_a_record_takes_no_dense_pass(lines, consts):
    by = {ln.split()[1]: _fields(ln) for ln in lines if ln.startswith("region ")}
    assert consts["bytes"] == 24 and consts["slot_bytes"] == 20 and consts["index_bits"] == 24 and consts["max_frames"] == 255
    assert consts["list_default"] == 1      # the keep rule holds on the headline: profiles/ray_list.md
    (ln,) = [l for l in lines if l.startswith("slots 64x64x256 ")]
    assert _fields(ln) == {"records": str(64 * 64 * 256), "dense": "1", "list": "0"}
    assert int(by["64x64x255"]["dense"]) == 1 and int(by["64x64x255"]["records"]) == 64 * 64 * 255
    assert int(by["64x64x256"]["dense"]) == 0 and int(by["64x64x256"]["list"]) == 0 and int(by["64x64x256"]["records"]) == 0
    assert int(by["4096x4096x2"]["dense"]) == 1
    assert int(by["4104x4096x2"]["dense"]) == 0 and int(by["4104x4096x2"]["records"]) == 0


def test_the_case_program_is_clean_under_the_sanitizers(tmp_path, lines):
    r = _build_and_run(tmp_path / "ray_list_cases_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.stdout.splitlines() == lines
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
