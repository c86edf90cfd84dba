"""The inputs of tests/test_gpu_compact.py reach what they claim, shown on the CPU with tests/compact_ref.py (the rule of
svo_pool_compact in plain Python) and the restatement of Octree.useSDFBrush: fresh pools are already in the builder's order,
edited pools shrink by known amounts, compaction is idempotent, the hand-made pools are refused or duplicated as meant, and the
oracle renders the same image from the pool before and after -- everything but the hit records' pointers, which name offsets."""
import numpy as np
import pytest

import svo_raytracer_amd.scene as scene
from svo_raytracer_amd.cameras import CAMERAS
import brush_helpers as B
import compact_helpers as H
import compact_ref

FRESH = {"terrain": 77111, "caves": 81909, "dust": 86751}
AFTER_EDGE = {"terrain": (150919, 49503), "caves": (155717, 49503), "dust": (144191, 37047)}


@pytest.mark.parametrize("family", B.FAMILIES)
def test_a_fresh_pool_is_already_compact(family):
    pool = B.family_pool64(family)
    assert pool.size == FRESH[family]
    assert np.array_equal(compact_ref.compact(pool), pool)


@pytest.mark.parametrize("family", B.FAMILIES)
def test_edge_strokes_leave_two_thirds_unreachable_and_compaction_is_idempotent(family):
    q, c = H.edited64(family)
    assert (q.size, c.size) == AFTER_EDGE[family]
    assert np.array_equal(compact_ref.compact(c), c)
    assert np.array_equal(c[:7], q[:7]) and c[0] == 0         # the root was filled with 0 and keeps its subtree: by tag, not by value
    # without the two root fills there is still something to drop
    q2, c2 = H.edited64(family, 2)
    assert c2.size < q2.size and q2[0] == 1


def test_small_strokes_on_128_leave_little_behind():
    chk = B.Checker(scene.build_scene(128)[0], depth=7)
    for kind, org, size, val in B.stroke_args():
        now = chk.stroke(kind, org, size, val, 128, 7)[1]
    assert (now.size, compact_ref.compact(now).size) == (450631, 442739)


def test_two_voxel_pools_come_back_as_they_are():
    for short_first in (False, True):
        p = B.two_voxel_pool(short_first)
        assert np.array_equal(compact_ref.compact(p), p)


def test_the_refused_inputs_are_refused_by_the_rule():
    p = B.two_voxel_pool(True)
    for pointer in (60, 8):                                   # the root's block starts past the end / ends one byte past it
        bad = p.copy()
        bad[4] = pointer
        with pytest.raises(compact_ref.Refused):
            compact_ref.compact(bad)
    with pytest.raises(compact_ref.Refused):
        compact_ref.compact(H.cyclic_pool())
    deep = scene.embed_deep(B.family_pool64("terrain"), compact_ref.MAX_LEVELS - 6)
    assert np.array_equal(compact_ref.compact(deep), deep)   # 13 levels of block owners: the bound itself
    with pytest.raises(compact_ref.Refused):
        compact_ref.compact(scene.embed_deep(B.family_pool64("terrain"), compact_ref.MAX_LEVELS - 5))


def test_a_shared_block_is_copied_twice():
    p = H.shared_pool()
    c = compact_ref.compact(p)
    assert (p.size, c.size) == (119, 175)
    assert np.array_equal(c[63:119], p[63:119]) and np.array_equal(c[119:175], p[63:119])
    assert np.array_equal(compact_ref.compact(c), c)


@pytest.mark.parametrize("family", B.FAMILIES)
def test_the_oracle_renders_the_same_image_before_and_after(family):
    from oracle import oracle
    q, c = H.edited64(family)
    for cam in ("K0", "K1", "K2"):
        for mode in (0, 2):
            a = oracle.render(q, 96, 64, CAMERAS[cam], 2, mode)
            b = oracle.render(c, 96, 64, CAMERAS[cam], 2, mode)
            hit = H.same_frame_but_pointers(a, b, (family, cam, mode))
            assert 327 <= int(hit.sum()) <= 6144, (family, cam, mode, int(hit.sum()))
            assert (a["hits"]["pointer"][hit] != b["hits"]["pointer"][hit]).any(), (family, cam, mode)   # the offsets did move
