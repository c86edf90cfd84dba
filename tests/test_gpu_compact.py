"""svo_pool_compact (csrc/svo_compact.hip.h): the device pool rewritten as exactly its reachable records, in the builder's
order.  The checker is tests/compact_ref.py, the rule in plain Python: every byte and the length, nothing with a tolerance.
Frames before and after are the same but for the hit records' pointers, which must be the oracle's on the compacted bytes.
tests/test_compact_cases.py shows on the CPU that these inputs reach what they claim."""
import ctypes

import numpy as np
import pytest

import svo_raytracer_amd.scene as scene
from svo_raytracer_amd.cameras import CAMERAS
import brush_helpers as B
import compact_helpers as H
import compact_ref

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    from svo_raytracer_amd import hiplib
    c = hiplib.HipContext()
    yield c
    c.close()


def _compact_equals_ref(ctx, want, old_size, tag=None):
    """one call: the lengths it reports, the pool's length and every byte are compact_ref's; zeros behind the end"""
    old, new = ctx.pool_compact()
    assert (old, new) == (old_size, want.size), (tag, old, new, old_size, want.size)
    got = ctx.pool_download(want.size + 64)                  # (a download ends at the pool's length: zeros behind it)
    bad = np.nonzero(got[:want.size] != want)[0]
    assert bad.size == 0, (tag, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
    assert not got[want.size:].any(), tag
    return got[:want.size]


def _strokes(ctx, strokes, world_size, max_lod):
    for kind, org, size, val in strokes:
        cb = B.gpu_stroke(ctx, kind, org, size, val, world_size, max_lod)
    return cb[3]


@pytest.mark.parametrize("short_first", [False, True], ids=["all_7_bytes", "child0_3_bytes"])
def test_two_voxel_pools(ctx, short_first):
    """the root and one block; with child 0 a 3-byte record the other seven sit at 10, 17, ... instead of 14, 21, ..."""
    pool = B.two_voxel_pool(short_first)
    ctx.pool_upload(pool)
    got = _compact_equals_ref(ctx, compact_ref.compact(pool), pool.size, short_first)
    assert np.array_equal(got, pool)
    info = ctx.compact_info()
    assert (info["calls"], info["records"], info["levels"]) == (1, 9, 1), info


@pytest.mark.parametrize("family", B.FAMILIES)
def test_a_fresh_pool_comes_back_unchanged(ctx, family):
    pool = B.family_pool64(family)
    ctx.pool_upload(pool)
    got = _compact_equals_ref(ctx, compact_ref.compact(pool), pool.size, family)
    assert np.array_equal(got, pool)
    assert ctx.compact_info()["levels"] == 6


@pytest.mark.parametrize("family", B.FAMILIES)
def test_after_the_edge_strokes_twice_in_a_row_and_a_brush_behind_it(ctx, family):
    """the 13 EDGE_STROKES on the GPU, the root filled twice; a second call changes nothing; then strokes land on the
    compacted pool as the restatement's land on compact_ref's -- a wrong length, a stale capacity or a stale stroke base
    shows here -- and the result compacts again"""
    pool = B.family_pool64(family)
    edited, want = H.edited64(family)
    ctx.pool_upload(pool)
    assert _strokes(ctx, B.EDGE_STROKES, 64, 6) == edited.size
    _compact_equals_ref(ctx, want, edited.size, family)
    _compact_equals_ref(ctx, want, want.size, (family, "again"))
    assert ctx.compact_info()["calls"] == 2
    chk = B.Checker(want, depth=6)
    before = want
    for k, (kind, org, size, val) in enumerate(B.fuzz_strokes(64, 6, B.FUZZ_SEEDS[family])):
        want_cb, now = chk.stroke(kind, org, size, val, 64, 6)
        cb = B.gpu_stroke(ctx, kind, org, size, val, 64, 6)
        before = B.assert_stroke_equal(ctx, cb, want_cb, now, before=before, tag=(family, k))
    _compact_equals_ref(ctx, compact_ref.compact(before), before.size, (family, "after the strokes"))
    assert ctx.compact_info()["calls"] == 3


def test_small_strokes_on_128(ctx):
    ctx.pool_upload(scene.build_scene(128)[0])
    n = _strokes(ctx, B.stroke_args(), 128, 7)
    edited = ctx.pool_download(n)
    want = compact_ref.compact(edited)
    assert (n, want.size) == (450631, 442739)
    _compact_equals_ref(ctx, want, n)


def test_level_lists_longer_than_one_scan_tile(ctx):
    """256^3 after WAVE_STROKES: the deepest levels hold far more than the 1024 nodes one block scans, and the second stroke's
    work list outgrew the brush's first item cap"""
    ctx.pool_upload(scene.build_scene(256)[0])
    n = _strokes(ctx, B.WAVE_STROKES, 256, 8)
    edited = ctx.pool_download(n)
    want = compact_ref.compact(edited)
    assert want.size < n
    _compact_equals_ref(ctx, want, n)
    info = ctx.compact_info()
    assert info["levels"] == 8 and info["records"] > 8 * 4 * 1024, info


def _frame(c, mode, use_beam, frame=2):
    return c.render(None, 96, 64, CAMERAS["K1"], frame, mode, use_beam=use_beam)


@pytest.mark.parametrize("use_beam", [0, 1])
@pytest.mark.parametrize("derived", [1, 0], ids=["table", "records"])
def test_frames_before_and_after(ctx, derived, use_beam):
    """caves after a carve-and-fill sequence that leaves the root alone: the frame is the same but for the pointers, which are
    the oracle's on the compacted bytes.  A descriptor table or a liveness table that was not rebuilt shows here."""
    from oracle import oracle
    edited, want = H.edited64("caves", 2)
    ctx.set_pipeline(1)
    ctx.set_derived(derived)
    ctx.pool_upload(B.family_pool64("caves"))
    assert _strokes(ctx, B.EDGE_STROKES[2:], 64, 6) == edited.size
    before = {mode: _frame(ctx, mode, use_beam) for mode in (0, 2)}
    if derived:
        assert ctx.derived_info()["walkable"]
    _compact_equals_ref(ctx, want, edited.size)
    for mode in (0, 2):
        after = _frame(ctx, mode, use_beam)
        hit = H.same_frame_but_pointers(before[mode], after, (derived, use_beam, mode))
        assert hit.any()
        ref = oracle.render(want, 96, 64, CAMERAS["K1"], 2, mode, use_beam=bool(use_beam))
        assert (after["hits"]["pointer"] == ref["hits"]["pointer"]).all(), (derived, use_beam, mode)
        assert (after["rgba"] == ref["rgba"]).all(), (derived, use_beam, mode)
    if derived:
        assert ctx.derived_info()["walkable"]


def test_a_ring_slot_in_flight_is_waited_for(ctx):
    from oracle import oracle
    edited, want = H.edited64("caves", 2)
    ctx.pool_upload(edited)
    ctx.resize(96, 64)
    ctx.set_camera(CAMERAS["K1"])
    ctx.set_params(2, 0, 0, 0, 2, 0, 1)
    ctx.ring_create(2, 1, want_hits=True)
    s0 = ctx.ring_submit(2, 1)
    _compact_equals_ref(ctx, want, edited.size)
    assert ctx.ring_query(s0)["done"]
    first = ctx.ring_read(s0, 0, want_hits=True)
    s1 = ctx.ring_submit(3, 1)
    assert s1 != s0
    got = ctx.ring_read(s1, 0, want_hits=True)
    ref = oracle.render(want, 96, 64, CAMERAS["K1"], 3, 0)
    assert (got["rgba"] == ref["rgba"]).all() and (got["depth"].view(np.uint32) == ref["depth"].view(np.uint32)).all()
    for key in ("pointer", "value", "raw_normal", "level", "iter"):
        assert (got["hits"][key] == ref["hits"][key]).all(), key
    old = oracle.render(edited, 96, 64, CAMERAS["K1"], 2, 0)
    assert (first["hits"]["pointer"] == old["hits"]["pointer"]).all()     # the frame in flight saw the old pool, whole


def _refused_inputs():
    p = B.two_voxel_pool(True)
    past = p.copy()
    past[4] = 60                                               # the root's block starts past the end
    crossing = B.family_pool64("terrain").copy()
    crossing = crossing[:crossing.size - 1]                    # the last block's last record crosses len
    return {"root_pointer_past_the_end": past, "last_record_crosses_len": crossing, "cycle": H.cyclic_pool(),
            "one_level_too_deep": scene.embed_deep(B.family_pool64("terrain"), compact_ref.MAX_LEVELS - 5)}


@pytest.mark.parametrize("case", ["root_pointer_past_the_end", "last_record_crosses_len", "cycle", "one_level_too_deep"])
def test_refusals_leave_everything_as_it_was(ctx, case):
    from svo_raytracer_amd import hiplib
    pool = _refused_inputs()[case]
    with pytest.raises(compact_ref.Refused):
        compact_ref.compact(pool)
    ctx.pool_upload(pool)
    derived, brush = ctx.derived_info(), ctx.brush_info()
    with pytest.raises(hiplib.SvoError) as err:
        ctx.pool_compact()
    assert err.value.code == -1, err.value                     # SVO_E_INVALID
    after = ctx.pool_download(pool.size + 64)
    assert np.array_equal(after[:pool.size], pool) and not after[pool.size:].any()
    assert ctx.derived_info() == derived and ctx.brush_info() == brush    # (build_ms included: the table was not rebuilt)
    assert ctx.compact_info()["calls"] == 0


def test_the_deepest_pool_the_walk_supports_goes_through(ctx):
    deep = scene.embed_deep(B.family_pool64("terrain"), compact_ref.MAX_LEVELS - 6)
    ctx.pool_upload(deep)
    got = _compact_equals_ref(ctx, compact_ref.compact(deep), deep.size)
    assert np.array_equal(got, deep) and ctx.compact_info()["levels"] == compact_ref.MAX_LEVELS


def test_a_shared_block_is_copied_twice(ctx):
    pool = H.shared_pool()
    want = compact_ref.compact(pool)
    ctx.set_pipeline(1)
    ctx.pool_upload(pool)
    before = _frame(ctx, 0, 0)
    got = _compact_equals_ref(ctx, want, pool.size)
    assert got.size == 175 and np.array_equal(got[63:119], got[119:175])
    H.same_frame_but_pointers(before, _frame(ctx, 0, 0))


def test_a_fan_of_shared_blocks_and_a_node_list_that_outgrows_its_cap(ctx):
    """four chained blocks whose records all share the next one: 1 + 8 + 64 + 512 nodes as a tree.  Thirteen of them would be
    8^12 nodes at the last level: the lists pass 2^27 nodes at level 9 and the call is refused, the pool as it was."""
    from svo_raytracer_amd import hiplib
    pool = H.fan_pool(4)
    want = compact_ref.compact(pool)
    assert (pool.size, want.size) == (7 + 4 * 56, 7 + 585 * 56)
    ctx.pool_upload(pool)
    _compact_equals_ref(ctx, want, pool.size)
    assert ctx.compact_info()["records"] == 1 + 8 * 585
    pool = H.fan_pool(13)
    ctx.pool_upload(pool)
    with pytest.raises(hiplib.SvoError) as err:
        ctx.pool_compact()
    assert err.value.code == -5, err.value                     # SVO_E_TOOLARGE
    after = ctx.pool_download(pool.size + 64)
    assert np.array_equal(after[:pool.size], pool) and not after[pool.size:].any()
    assert ctx.compact_info()["calls"] == 1


def test_group_members_compact_alike():
    from svo_raytracer_amd import hiplib
    pool = B.family_pool64("caves")
    strokes = [B.EDGE_STROKES[2], B.EDGE_STROKES[10], B.EDGE_STROKES[9]]   # a corner filled, a ball, a slab carved through both
    chk = B.Checker(pool, depth=6)
    for kind, org, size, val in strokes:
        edited = chk.stroke(kind, org, size, val, 64, 6)[1]
    edited = edited.copy()
    want = compact_ref.compact(edited)
    assert want.size < edited.size - 1000
    g = hiplib.HipGroup([0, 0, 0])
    try:
        g.pool_upload(pool)
        for kind, org, size, val in strokes:
            cb = g.brush_sphere(org, size, val, 64, 6) if kind == "sphere" else g.brush_box(org, size[0], size[1], size[2], val, 64, 6)
        assert cb[3] == edited.size
        # through the JNI-typed export, what HipRenderer.Group.compactPool calls
        f = hiplib.lib().Java_src_engine_HipRenderer_nGroupPoolCompact
        f.restype, f.argtypes = ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
        sizes = np.zeros(2, np.int64)
        assert f(None, None, g._h.value, sizes.ctypes.data) == 0
        assert list(sizes) == [edited.size, want.size]
        for r in range(3):
            m = g.member(r)
            assert m.pool_device_ptr()[1] == want.size
            assert np.array_equal(m.pool_download(want.size), want), r
        assert g.pool_compact() == (want.size, want.size)
    finally:
        g.close()
