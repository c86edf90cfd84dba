"""The GPU SDF brush (svo_brush_sphere / svo_brush_box, csrc/svo_brush.hip.h) at its edges: a brush that holds the whole world
or crosses its faces, radius 0 and 1, empty and huge boxes, the values 127 and 255, the "caves" and "dust" pools, nodes marched
by several waves, a work list that has to grow, max_lod and world_size away from the tree's depth, the root fill on two-voxel
worlds, and a seeded fuzz over all of it.  The checker throughout is the restatement of Octree.useSDFBrush
(oracle/octree_restatement.cpp) run on a hostlib.Octree that adopted the same bytes: the ChangeBounds, the pool's length and
every byte, nothing with a tolerance.  tests/test_brush_edges_cases.py shows on the CPU that these inputs reach what they claim."""
import numpy as np
import pytest

import svo_raytracer_amd.scene as scene
from svo_raytracer_amd.cameras import CAMERAS
import brush_helpers as B
import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    from svo_raytracer_amd import hiplib
    c = hiplib.HipContext()
    yield c
    c.close()


def _follow(ctx, chk, strokes, world_size, max_lod, before, tag):
    """every stroke on both sides, compared; yields (k, reference cb, reference pool before, after)"""
    for k, (kind, org, size, val) in enumerate(strokes):
        want_cb, want = chk.stroke(kind, org, size, val, world_size, max_lod)
        cb = B.gpu_stroke(ctx, kind, org, size, val, world_size, max_lod)
        got = B.assert_stroke_equal(ctx, cb, want_cb, want, before=before, tag=(tag, k, kind, org, size, val))
        yield k, want_cb, before, want
        before = got


@pytest.mark.parametrize("family", B.FAMILIES)
def test_edge_strokes_on_three_scene_families(ctx, family):
    pool = B.family_pool64(family)
    chk = B.Checker(pool, depth=6)
    ctx.pool_upload(pool)
    for k, want_cb, before, want in _follow(ctx, chk, B.EDGE_STROKES, 64, 6, pool, family):
        f = B.diff_facts(before, want)
        # the reference's side of the case: it must keep reaching the root fill whatever becomes of the generators
        if k in B.EDGE_ROOT_FILLS:
            assert f["root"], (family, k)
        if k == B.EDGE_ROOT_FILLS[0]:
            assert f["more127"] == 8, (family, k, f)
        if k == B.EDGE_GROWS:
            assert f["appended"] == B.EDGE_GROWTH, (family, k, f)
        if k == B.EDGE_DUST_IDLE and family == "dust":
            assert want_cb == [before.size, 0, before.size, before.size] and f["untouched"]
    assert ctx.brush_info()["strokes"] == len(B.EDGE_STROKES)


def test_nodes_marched_by_several_waves_and_a_work_list_that_grows(ctx):
    """256^3: the root's march is split over 16 waves and a level-1 node's over 4 (gridDim.y > 1, with the early-out on what
    another wave has seen); the second stroke visits more than kFirstCap nodes, so that its first plan overflows and is
    repeated with four times the room; the third finds the enlarged list"""
    pool = scene.build_scene(256)[0]
    chk = B.Checker(pool, kb=1 << 18, depth=8)
    ctx.pool_upload(pool)
    for k, want_cb, before, want in _follow(ctx, chk, B.WAVE_STROKES, 256, 8, pool, "waves"):
        visited = ctx.brush_info()["visited"]
        if k == 1:
            # a subdivision appends at most 56 bytes and creates 8 work items
            assert (want_cb[3] - want_cb[2]) // 7 > B.FIRST_CAP, want_cb
            assert visited > B.FIRST_CAP, visited
        elif k == 2:
            assert 8 < visited < B.FIRST_CAP // 8, visited     # a small stroke, on the enlarged list
        assert want.size > before.size, k


@pytest.mark.parametrize("case", sorted(B.LOD_CASES))
def test_max_lod_and_world_size_away_from_the_depth(ctx, case):
    """max_lod 7 on a tree of depth 6: the size-1 leaves a stroke creates are 7-byte records; world_size 132 on the 128^3
    tree: 132 -> 66 -> 33 -> 16 -> ... -> 1, the halving of Constants.WORLD_SIZE = 8196 in small"""
    n, world_size, max_lod, strokes = B.LOD_CASES[case]
    pool = scene.build_scene(n)[0]
    chk = B.Checker(pool, depth=n.bit_length() - 1)
    ctx.pool_upload(pool)
    grew = 0
    for k, want_cb, before, want in _follow(ctx, chk, strokes, world_size, max_lod, pool, case):
        assert not B.diff_facts(before, want)["untouched"], (case, k)
        grew += want.size > before.size
    assert grew


def test_max_lod_below_the_depth_is_refused(ctx):
    """max_lod 4 on the 64^3 terrain: the stroke would subdivide the 3-byte leaves it creates itself at level 4 (size 4).  The
    reference writes a child pointer into such a record and corrupts its own pool, so it is not asked: the GPU must refuse the
    stroke and leave the pool, its length and the stroke count as they were"""
    from svo_raytracer_amd import hiplib
    world_size, max_lod, (kind, org, size, val) = B.REFUSED
    assert not B.restatement_safe(world_size, max_lod, 6)
    pool = scene.build_scene(64)[0]
    ctx.pool_upload(pool)
    n = pool.size
    strokes = ctx.brush_info()["strokes"]
    with pytest.raises(hiplib.SvoError):
        B.gpu_stroke(ctx, kind, org, size, val, world_size, max_lod)
    assert ctx.brush_info()["strokes"] == strokes
    after = ctx.pool_download(n + 64)                            # (a download ends at the pool's length: zeros behind it)
    assert np.array_equal(after[:n], pool) and not after[n:].any()
    assert ctx.brush_sphere((200, 200, 200), 1, 2, 64, 6)[2:] == [n, n]   # outside the world: nothing to do, the length as it was
    # and with max_lod = the depth the same stroke goes through
    want_cb, want = B.Checker(pool, depth=6).stroke(kind, org, size, val, world_size, 6)
    B.assert_stroke_equal(ctx, B.gpu_stroke(ctx, kind, org, size, val, world_size, 6), want_cb, want, before=pool)


@pytest.mark.parametrize("short_first", [True, False], ids=["child0_3_bytes", "all_7_bytes"])
def test_root_fill_on_a_two_voxel_world(ctx, short_first):
    """The reference re-tags the root's child 0 (the root is its own parent) to tag 2 BEFORE it walks the root's children to
    mark them with DELETE_VALUE (Octree.java:797-808), so the walk reads the patched mask: with child 0 a 3-byte record the
    marks land at 7, 14, 21, ..., 56 -- not at the children's records 7, 10, 17, ..., 52."""
    pool = B.two_voxel_pool(short_first)
    assert pool.size == (59 if short_first else 63)
    chk = B.Checker(pool, depth=1)
    ctx.pool_upload(pool)
    kind, org, size, val = B.TWO_VOXEL_STROKE
    want_cb, want = chk.stroke(kind, org, size, val, 2, 1)
    assert want.size == pool.size and list(np.nonzero(want == 127)[0]) == list(range(7, 63, 7)) and want[0] == val
    cb = B.gpu_stroke(ctx, kind, org, size, val, 2, 1)
    B.assert_stroke_equal(ctx, cb, want_cb, want, before=pool, tag=short_first)


@pytest.mark.parametrize("family", B.FAMILIES)
def test_seeded_fuzz_is_byte_equal_and_renders_like_the_oracle(family):
    from oracle import oracle
    pool = B.family_pool64(family)
    chk = B.Checker(pool, depth=6)
    cam = CAMERAS["K1"]
    ctx = helpers.DualContext()
    try:
        ctx.set_pipeline(1)
        ctx.set_derived(1)
        ctx.pool_upload(pool)
        assert ctx.derived_info()["walkable"]
        for k, want_cb, before, want in _follow(ctx.active, chk, B.fuzz_strokes(64, 48, B.FUZZ_SEEDS[family]), 64, 6, pool, family):
            if k % 8 != 7:
                continue
            got = ctx.render(None, 96, 64, cam, 2 + k, 0)
            ref = oracle.render(want, 96, 64, cam, 2 + k, 0)
            assert (got["rgba"] == ref["rgba"]).all(), (family, k)
            assert (got["depth"].view(np.uint32) == ref["depth"].view(np.uint32)).all(), (family, k)
            for key in ("pointer", "value", "raw_normal", "level", "iter"):
                assert (got["hits"][key] == ref["hits"][key]).all(), (family, k, key)
            assert ctx.derived_info()["walkable"], (family, k)
    finally:
        ctx.close()
