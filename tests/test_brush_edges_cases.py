"""The inputs of tests/test_gpu_brush_edges.py are not vacuous: the same stroke sequences through the restatement of
Octree.useSDFBrush alone (oracle/octree_restatement.cpp, no GPU), and what they reach, read from the pools before and after
each stroke and from nothing else.  The refusal case (brush_helpers.REFUSED) is not run: the reference corrupts its pool there."""
import numpy as np
import pytest

import svo_raytracer_amd.scene as scene
import brush_helpers as B


def _facts(pool, strokes, world_size, max_lod, depth, kb=1 << 16):
    chk = B.Checker(pool, kb=kb, depth=depth)
    out, before = [], pool
    for kind, org, size, val in strokes:
        cb, now = chk.stroke(kind, org, size, val, world_size, max_lod)
        f = B.diff_facts(before, now)
        f["cb"], f["len"] = cb, before.size
        assert cb[2] == before.size and cb[3] == now.size
        out.append(f)
        before = now
    return out


def test_the_rule_of_the_generators():
    assert B.restatement_safe(64, 6, 6) and B.restatement_safe(256, 8, 8) and B.restatement_safe(2, 1, 1)
    assert B.restatement_safe(68, 6, 6)                      # 68 -> 34 -> 17 -> 8 -> 4 -> 2 -> 1
    for n, world_size, max_lod, _ in B.LOD_CASES.values():
        assert B.restatement_safe(world_size, max_lod, n.bit_length() - 1)
    assert not B.restatement_safe(B.REFUSED[0], B.REFUSED[1], 6)
    assert not B.restatement_safe(128, 6, 7) and not B.restatement_safe(132, 7, 6)
    with pytest.raises(AssertionError):
        B.Checker(B.two_voxel_pool(False), depth=1).stroke(*B.TWO_VOXEL_STROKE, 4, 1)


@pytest.mark.parametrize("family", B.FAMILIES)
def test_edge_sequence_reaches_the_root_fill_short_leaves_and_an_idle_stroke(family):
    pool = B.family_pool64(family)
    assert pool.size == {"terrain": 77111, "caves": 81909, "dust": 86751}[family]
    facts = _facts(pool, B.EDGE_STROKES, 64, 6, 6)
    assert any(f["root"] for f in facts)
    assert any(f["more127"] > 0 for f in facts)
    assert any(f["appended"] % 56 for f in facts)            # blocks of eight 3-byte leaves at max_lod
    assert any(f["untouched"] for f in facts)
    # what test_gpu_brush_edges.py asserts of the reference as it goes
    for k in B.EDGE_ROOT_FILLS:
        assert facts[k]["root"] and facts[k]["appended"] == 0
    assert facts[B.EDGE_ROOT_FILLS[0]]["more127"] == 8
    assert facts[B.EDGE_GROWS]["appended"] == B.EDGE_GROWTH
    idle = facts[B.EDGE_DUST_IDLE]
    assert (idle["untouched"] and idle["cb"] == [idle["len"], 0, idle["len"], idle["len"]]) == (family == "dust")
    assert facts[-1]["untouched"]


def test_wave_strokes_outgrow_the_first_work_list():
    pool = scene.build_scene(256)[0]
    facts = _facts(pool, B.WAVE_STROKES, 256, 8, 8, kb=1 << 18)
    assert [f["appended"] for f in facts[:2]] == [677448, 2255512]
    cb = facts[1]["cb"]
    assert (cb[3] - cb[2]) // 7 > B.FIRST_CAP == 1 << 18      # a subdivision appends at most 56 bytes and creates 8 work items
    assert 0 < facts[2]["appended"] < 7 * (B.FIRST_CAP // 8)


@pytest.mark.parametrize("case", sorted(B.LOD_CASES))
def test_lod_cases_change_the_pool(case):
    n, world_size, max_lod, strokes = B.LOD_CASES[case]
    facts = _facts(scene.build_scene(n)[0], strokes, world_size, max_lod, n.bit_length() - 1)
    assert not any(f["untouched"] for f in facts)
    assert any(f["appended"] for f in facts)
    if max_lod > n.bit_length() - 1:
        assert all(f["appended"] % 56 == 0 for f in facts)   # no 3-byte leaves: the new size-1 leaves are 7-byte records
    assert any(kind == "box" for kind, *_ in strokes) == (case == "world132_on_128")


@pytest.mark.parametrize("short_first", [True, False])
def test_two_voxel_root_fill_stays_inside_the_pool(short_first):
    pool = B.two_voxel_pool(short_first)
    mask = (int(pool[5]) << 8) | int(pool[6])
    sizes = [{1: 3, 2: 7}[(mask >> (2 * c)) & 3] for c in range(8)]
    assert 7 + sum(sizes) == pool.size == (59 if short_first else 63)
    (f,) = _facts(pool, [B.TWO_VOXEL_STROKE], 2, 1, 1)
    assert f["root"] and f["appended"] == 0 and f["more127"] == 8 and f["cb"] == [0, 7, pool.size, pool.size]
    # the marks follow the RE-TAGGED mask (child 0 as 7 bytes): the last lands at 56 < 59, inside the pool
    chk = B.Checker(pool, depth=1)
    now = chk.stroke(*B.TWO_VOXEL_STROKE, 2, 1)[1]
    assert list(np.nonzero(now == 127)[0]) == list(range(7, 63, 7))
    old = list(7 + np.concatenate([[0], np.cumsum(sizes[:-1])]))
    assert (old != list(range(7, 63, 7))) == short_first      # where a walk of the old mask would have put them


@pytest.mark.parametrize("family", B.FAMILIES)
def test_fuzz_strokes_mostly_do_something(family):
    strokes = B.fuzz_strokes(64, 48, B.FUZZ_SEEDS[family])
    assert len(strokes) == 48 and [s[0] for s in strokes[:3]] == ["sphere", "sphere", "box"]
    assert strokes == B.fuzz_strokes(64, 48, B.FUZZ_SEEDS[family])
    for kind, org, size, val in strokes:
        assert all(-8 <= v < 72 for v in org) and val in (0, 1, 2, 3, 127, 255)
        if kind == "sphere":
            assert size in (0, 1, 2, 3, 5, 8, 13, 16, 32, 128)
        else:
            assert all(v in (0, 1, 2, 8, 64, 256) for v in size)
    facts = _facts(B.family_pool64(family), strokes, 64, 6, 6)
    assert 4 * sum(f["untouched"] for f in facts) <= len(facts)
    assert any(f["root"] for f in facts) and any(f["more127"] > 0 for f in facts) and any(f["appended"] % 56 for f in facts)
    assert {s[3] for s in strokes} >= {0, 127, 255}
