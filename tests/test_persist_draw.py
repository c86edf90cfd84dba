"""The pure half of the persistent kernels' draw (svo-raytracer_amd/csrc/svo_persist_plan.h: band_of, slot_tile, slot_pixel;
persist_cast_kernel decodes its slots through this text, a slot per pixel, and tests/test_gpu_dense_shade.py holds that kernel's
bytes against the kernels that keep their own statement of it -- the frame / sample branches run on the host only): tests/persist_draw_cases.cpp, a host program, walks every slot of all 8
bands of a fixed list of launches through it, in both column directions, and counts what does not match the set the launch must
produce -- {frames} x {samples} x {pixels of the launch's rows inside the frame}, each once, at its output index.  The counts
expected below are worked out from the cases' sizes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = tmp_path_factory.mktemp("persist_draw") / "persist_draw_cases"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "svo-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "persist_draw_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    cases = {}
    for ln in out:
        name, *fields = ln.split()
        cases[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return cases


def expect(case, **want):
    got = {k: case[k] for k in want}
    assert got == want


def test_every_case_draws_exactly_its_set(cases):
    assert len(cases) == 9
    for name, c in cases.items():
        assert c["bad"] == 0, (name, c)
        assert c["drawn"] == c["want"] > 0, (name, c)


def test_one_tile(cases):
    # a band of one tile row: the division by the band's rows is no division (udiv_magic declines d <= 1)
    expect(cases["one_tile"], slots=64, drawn=64, rows_per_band=1, full=1, part=0, empty=7, cut_x=0, magics=0)


def test_odd_frame_reaches_every_kind_of_band_and_every_bounds_check(cases):
    # 21 x 130: 3 x 17 tiles; bands 0-4 hold 3 tile rows, band 5 holds 2, bands 6-7 none; 3 of 24 columns and 6 of 136 rows cut
    for name in ("odd", "odd_real_division"):
        expect(cases[name], slots=3 * 17 * 64, drawn=21 * 130, rows_per_band=3, full=5, part=1, empty=2, cut_x=3 * 136,
               cut_y1=6 * 24, cut_h=6 * 24)
    assert cases["odd"]["magics"] >= 2 and cases["cut_by_height"]["cut_y1"] == 0
    expect(cases["cut_by_height"], drawn=21 * 140, cut_h=4 * 24, rows_per_band=3, full=6, part=0, empty=2)


def test_stripe(cases):
    # tile rows at pixel rows 8, 24, 40, 56; y1 = 60 leaves 4 rows of the last: 28 rows of 21 pixels
    expect(cases["stripe"], slots=3 * 4 * 64, drawn=21 * 28, rows_per_band=1, full=4, part=0, empty=4, cut_y1=4 * 24, cut_h=0)


def test_batches(cases):
    expect(cases["batch3_frame_pixel"], span=0, slots=3 * 3 * 17 * 64, drawn=3 * 21 * 130)
    expect(cases["batch3_pixel"], span=1, slots=3 * 17 * 64, drawn=21 * 130)


def test_folded_samples(cases):
    expect(cases["fold3"], fold=3, slots=3 * 9 * 64, drawn=3 * 72 * 8, rows_per_band=1, full=1, empty=7)
    expect(cases["fold3_batch2"], fold=3, span=0, slots=2 * 3 * 3 * 17 * 64, drawn=2 * 3 * 21 * 130)
