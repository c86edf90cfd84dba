"""What a launch of the persistent pipeline decides before it touches the GPU (svo-raytracer_amd/csrc/svo_persist_plan.h::
persist_plan): tests/persist_plan_cases.cpp, a host program, prints the plan of a fixed list of launches; the expected values
below are worked out from the rules the library has always applied, on a device of 256 CUs that holds 20 persistent waves per CU
of the record walk and 24 of the descriptor walk.  (A frame without tiles never reaches the plan: launch_frame returns first.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, PLANES, TILES, SEQUENCE = 0, 1, 2, 3      # PersistPlan::Resolve


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("persist_plan") / "persist_plan_cases"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "svo-raytracer_amd", "csrc"), os.path.join(ROOT, "tests", "persist_plan_cases.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    plans = {}
    for ln in out:
        name, *fields = ln.split()
        plans[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return plans


def expect(plan, **want):
    got = {k: plan[k] for k in want}
    assert got == want


def test_full_hd_by_launch_shape(plans):
    # 240 x 135 tiles = 32 400: more work than waves, so waves = (CUs the stream may use) x (waves per CU)
    expect(plans["hd_plain"], invalid=0, per_cu=24, blocks=6144, thresh=9, tables=1, fold=1, launches=1, span=0, slot_frames=1,
           resolve=NONE, cache=0, rows_per_band=17, facc_floats=0, prim_waves=0, rc_floats=3840 + 8 * 1080, kept_records=0)
    expect(plans["hd_ring"], per_cu=10, blocks=2560, thresh=9, tables=1)
    for sets, per_cu in ((2, 12), (3, 10), (4, 8), (5, 6)):
        expect(plans["hd_overlap%d" % sets], per_cu=per_cu, blocks=256 * per_cu, thresh=9, tables=1)
    expect(plans["hd_records"], per_cu=20, blocks=5120, thresh=9, tables=0, rc_floats=0, span=0, cache=0)


def test_set_tuning_and_reserved_cus(plans):
    for name in ("hd_tuned_plain", "hd_tuned_ring", "hd_tuned_overlap4", "hd_tuned_records"):
        expect(plans[name], per_cu=3, blocks=768, thresh=11)
    expect(plans["hd_reserved_plain"], per_cu=24, blocks=(256 - 16) * 24)
    expect(plans["hd_reserved_ring"], per_cu=10, blocks=(256 - 16) * 10)


def test_one_tile(plans):
    expect(plans["tiny"], per_cu=24, blocks=1, tables=1, rows_per_band=1, rc_floats=16 + 64, fold=1, span=0, magics=0)


def test_static_camera_batch_shares_its_primary_rays(plans):
    # 4 frames of 64 x 64 (64 tiles) as a ring submission: a slot per pixel, so the waves are capped by the tiles of ONE frame;
    # the primary-hit records have room for every wave a launch of this shape can have (256 CUs x 10)
    expect(plans["batch4"], per_cu=10, span=1, slot_frames=1, blocks=64, tables=1, cache=1, prim_waves=2560, fold=1, resolve=NONE,
           rc_floats=4 * (128 + 8 * 64), kept_records=64 * 64)
    # a cache candidate exactly when hit records are off and tables are on
    expect(plans["batch4_hits"], span=1, blocks=64, tables=1, cache=0, kept_records=0)
    expect(plans["batch4_notables"], span=1, blocks=64, tables=0, cache=0, kept_records=0, prim_waves=2560)
    expect(plans["batch4_nocache"], span=1, blocks=64, tables=1, cache=0, kept_records=0)


@pytest.mark.parametrize("case", ["cams", "1bounce", "beam", "mode2", "records", "nospan"])
def test_what_switches_the_shared_primary_off(plans, case):
    # a slot per (frame, pixel) again: 4 x 64 tiles
    expect(plans["batch4_" + case], per_cu=10, span=0, slot_frames=4, blocks=256, cache=0, prim_waves=0, fold=1,
           tables=0 if case == "records" else 1)


def test_samples_switch_the_shared_primary_off(plans):
    expect(plans["batch4_spp4"], span=0, slot_frames=4, fold=4, launches=1, blocks=4 * 64 * 4, resolve=TILES, tables=0, cache=0,
           facc_floats=192 * 4 * 64 * 4, prim_waves=0)


def test_folded_samples_and_sequences(plans):
    expect(plans["spp4"], invalid=0, per_cu=24, fold=4, launches=1, sequence=0, resolve=TILES, tables=0, blocks=64 * 4,
           facc_floats=192 * 4 * 64, span=0, rows_per_band=1, magics=1)
    expect(plans["seq3"], invalid=0, fold=3, launches=1, sequence=1, resolve=SEQUENCE, tables=0, blocks=64 * 3, facc_floats=192 * 3 * 64)
    expect(plans["seq3_spp2"], invalid=1)


def test_fold_budget(plans):
    # 192 floats x 64 samples x 129 600 tiles = 6.4e9 bytes > 4 GiB: a launch per sample, running sums in three planes
    assert 192 * 64 * 129600 * 4 > 2 ** 32
    expect(plans["uhd_spp64"], invalid=0, per_cu=24, blocks=6144, fold=1, launches=64, resolve=PLANES, tables=1, span=0,
           facc_floats=3 * 3840 * 2160, rows_per_band=34)


def test_reciprocals_divide_exactly(plans):
    # every n up to the largest the launch can form, for every reciprocal the plan did not decline
    for name, plan in plans.items():
        assert plan["magic_bad"] == 0, name
        assert (plan["magic_checked"] > 0) == (plan["magics"] > 0), name
    assert plans["hd_plain"]["magics"] == 4         # bands of 17 and 16 tile rows, 4080 and 3840 tile slots per frame
    assert plans["hd_plain"]["magic_checked"] == 2 * (4080 + 1) + 2 * (3840 + 1)
    assert plans["spp4"]["magic_checked"] == 32 + 1   # 8 tiles x 4 samples per band and frame; a band of one tile row needs no division
