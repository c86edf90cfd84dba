"""SDF brush strokes applied to the pool on the GPU (svo_brush_sphere / svo_brush_box: Main.placeSDF, Main.java:338-353,
without the host's copy of the pool).  The checker throughout is the restatement of Octree.useSDFBrush
(oracle/octree_restatement.cpp; parity with the Java unpinned, no JDK) run on a hostlib.Octree that adopted the same pool:
after every stroke the pool, its length and the ChangeBounds must be byte for byte the restatement's."""
import ctypes

import numpy as np
import pytest

import svo_raytracer_amd.scene as scene
from svo_raytracer_amd.cameras import CAMERAS
import brush_helpers as B
import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool64():
    return scene.build_scene(64)[0]


@pytest.fixture(scope="module")
def pool128():
    return scene.build_scene(128)[0]


@pytest.fixture()
def ctx():
    from svo_raytracer_amd import hiplib
    c = hiplib.HipContext()
    yield c
    c.close()


def test_edits_sequence_is_byte_equal_and_stays_inside_the_written_ranges(ctx, pool64):
    chk = B.Checker(pool64)
    ctx.pool_upload(pool64)
    before = pool64
    for k, (kind, org, size, val) in enumerate(B.edits64()):
        want_cb, want = chk.stroke(kind, org, size, val, 64, 6)
        cb = B.gpu_stroke(ctx, kind, org, size, val, 64, 6)
        info = ctx.brush_info()
        before = B.assert_stroke_equal(ctx, cb, want_cb, want, before=before, tag=(k, kind))
        assert info["strokes"] == k + 1 and info["visited"] >= 9 and info["lo"] <= info["hi"] <= cb[2]
    assert (before == 127).any()      # the fill marked children with DELETE_VALUE: outside cb's first range or not, inside [lo, hi)


def test_stroke_sequence_with_the_table_renders_like_the_oracle(pool128):
    from oracle import oracle
    from derived_edits import brush_strokes
    import derived_ref as R
    from test_sdf_edit import KEDIT
    cams = [KEDIT, CAMERAS["K1"]]
    args = B.stroke_args(128, 14, 11)
    chk = B.Checker(pool128)
    ctx = helpers.DualContext()
    try:
        ctx.set_pipeline(1)
        ctx.set_derived(1)
        ctx.pool_upload(pool128)
        assert ctx.derived_info()["walkable"]
        followed = 0
        for (stroke, host, want_cb, root_changed), (kind, org, size, val) in zip(brush_strokes(pool128, n=128, lod=7, strokes=14, seed=11), args):
            cb2, mine = chk.stroke(kind, org, size, val, 128, 7)
            assert cb2 == want_cb and np.array_equal(mine, host), stroke     # the arguments are the generator's
            refreshes = ctx.derived_refresh_info()["refreshes"]
            cb = B.gpu_stroke(ctx.active, kind, org, size, val, 128, 7)
            B.assert_stroke_equal(ctx.active, cb, want_cb, host, tag=stroke)
            info = ctx.brush_info()
            wrote = (info["hi"] > info["lo"]) + (cb[3] > cb[2])
            if not root_changed and wrote:
                assert ctx.derived_refresh_info()["refreshes"] - refreshes == wrote, (stroke, cb, info)   # followed, not rebuilt
                followed += 1
            for cam in cams:
                got = ctx.render(None, 128, 80, cam, 2 + stroke, 0)
                ref = oracle.render(host, 128, 80, cam, 2 + stroke, 0)
                assert (got["rgba"] == ref["rgba"]).all(), stroke
                assert (got["depth"].view(np.uint32) == ref["depth"].view(np.uint32)).all(), stroke
                for k in ("pointer", "value", "raw_normal", "level", "iter"):
                    assert (got["hits"][k] == ref["hits"][k]).all(), (stroke, k)
            assert ctx.derived_info()["walkable"]
        assert followed >= 5, followed
    finally:
        ctx.close()


@pytest.mark.parametrize("world", [68])
def test_root_that_is_no_power_of_two(ctx, pool64, world):
    """68 -> 34 -> 17 -> 8 -> 4 -> 2 -> 1: the halving of Constants.WORLD_SIZE = 8196 in small"""
    chk = B.Checker(pool64)
    ctx.pool_upload(pool64)
    for kind, org, size, val in [("sphere", (22, 25, 41), 7, 2), ("sphere", (45, 20, 25), 6, 0)]:
        want_cb, want = chk.stroke(kind, org, size, val, world, 6)
        assert want.size > pool64.size
        cb = B.gpu_stroke(ctx, kind, org, size, val, world, 6)
        B.assert_stroke_equal(ctx, cb, want_cb, want, tag=(world, org))


def test_nodes_that_meet_only_the_corner_of_the_bounding_box(ctx, pool128):
    """origin = 64 +- (r + 1): the brush's bounding box ends on the planes between the top-level nodes, which the inclusive
    intersection test still lets in: they are marched row by row over their whole width"""
    r = 9
    chk = B.Checker(pool128)
    ctx.pool_upload(pool128)
    for org, val in [((64 + r + 1,) * 3, 0), ((64 - r - 1,) * 3, 2), ((64 + r + 1,) * 3, 2), ((64 - r - 1,) * 3, 0)]:
        want_cb, want = chk.stroke("sphere", org, r, val, 128, 7)
        cb = B.gpu_stroke(ctx, "sphere", org, r, val, 128, 7)
        B.assert_stroke_equal(ctx, cb, want_cb, want, tag=(org, val))


def test_growth_after_a_fresh_upload_and_a_frame_in_flight(ctx, pool64):
    chk = B.Checker(pool64)
    ctx.pool_upload(pool64)          # capacity: what the upload left
    cam = CAMERAS["K1"]
    want_frame = ctx.render(None, 96, 64, cam, 2, 0)
    ctx.dispatch_async()             # the same frame again, in flight when the stroke starts
    for k, (org, r, val) in enumerate([((20, 24, 40), 7, 2), ((40, 22, 28), 10, 0)]):
        want_cb, want = chk.stroke("sphere", org, r, val, 64, 6)
        cb = ctx.brush_sphere(org, r, val, 64, 6)
        assert cb[3] > cb[2]         # it appended
        B.assert_stroke_equal(ctx, cb, want_cb, want, tag=k)
        if k == 0:
            assert (ctx.read_color() == want_frame["rgba"]).all()
            assert (ctx.read_depth().view(np.uint32) == want_frame["depth"].view(np.uint32)).all()


def test_a_host_copy_kept_in_step_by_ranged_downloads(ctx, pool64):
    ctx.pool_upload(pool64)
    mirror = np.zeros(pool64.size * 4, np.uint8)
    mirror[:pool64.size] = pool64
    n = pool64.size
    for kind, org, size, val in B.edits64():
        cb = B.gpu_stroke(ctx, kind, org, size, val, 64, 6)
        info = ctx.brush_info()
        if info["hi"] > info["lo"]:
            ctx.pool_download_range(mirror, info["lo"], info["hi"])
        if cb[3] > cb[2]:
            ctx.pool_download_range(mirror, cb[2], cb[3])
        n = cb[3]
        assert np.array_equal(mirror[:n], ctx.pool_download(n))
    assert not mirror[n:].any()
    from svo_raytracer_amd import hiplib
    with pytest.raises(hiplib.SvoError):
        ctx.pool_download_range(mirror, n, n + 1)       # past the pool's end
    with pytest.raises(hiplib.SvoError):
        ctx.pool_download_range(mirror, 8, 8)


def test_refusals_leave_the_pool_alone(ctx, pool64):
    from svo_raytracer_amd import hiplib
    from derived_edits import _short40
    L = hiplib.lib()
    org = (ctypes.c_int * 3)(20, 24, 40)
    cb = (ctypes.c_int32 * 4)()
    assert L.svo_brush_sphere(ctx._h, org, 5, 2, 64, 6, cb) == -2                       # SVO_E_NOPOOL
    assert L.svo_brush_box(ctx._h, org, 3, 3, 3, 2, 64, 6, cb) == -2
    ctx.pool_upload(pool64)
    for value in (-1, 256):
        assert L.svo_brush_sphere(ctx._h, org, 5, value, 64, 6, cb) == -1               # SVO_E_INVALID
        assert L.svo_brush_box(ctx._h, org, 3, 3, 3, value, 64, 6, cb) == -1
    assert L.svo_brush_sphere(ctx._h, None, 5, 2, 64, 6, cb) == -1
    assert L.svo_brush_box(ctx._h, None, 3, 3, 3, 2, 64, 6, cb) == -1
    assert np.array_equal(ctx.pool_download(pool64.size), pool64)
    # hand-made pools: one-byte leaves the stroke would have to subdivide, and a root whose child block lies past the end
    short = _short40()
    past = short.copy()
    past[1:5] = np.frombuffer((100).to_bytes(4, "big"), np.uint8)
    for bad in (short, past):
        ctx.pool_upload(bad)
        before = ctx.pool_download(bad.size)
        with pytest.raises(hiplib.SvoError):
            ctx.brush_sphere((16, 16, 16), 5, 2, 64, 6)
        assert ctx.brush_sphere((200, 200, 200), 5, 2, 64, 6)[2:] == [bad.size, bad.size]   # outside the world: nothing to do
        assert np.array_equal(ctx.pool_download(bad.size + 64)[:bad.size], before)
        assert not ctx.pool_download(bad.size + 64)[bad.size:].any()


def test_group_stroke_reaches_every_member(ctx, pool64):
    from svo_raytracer_amd import hiplib
    ctx.pool_upload(pool64)
    kind, org, r, val = B.edits64()[0]
    cb1 = ctx.brush_sphere(org, r, val, 64, 6)
    want = ctx.pool_download(cb1[3])
    g = hiplib.HipGroup([0, 0])
    try:
        g.pool_upload(pool64)
        cb = g.brush_sphere(org, r, val, 64, 6)
        assert cb == cb1
        for m in range(2):
            assert np.array_equal(g.member(m).pool_download(cb[3]), want)
        cbb = g.brush_box(*B.BOX_EDIT[1:2], *B.BOX_EDIT[2], B.BOX_EDIT[3], 64, 6)
        cb2 = ctx.brush_box(B.BOX_EDIT[1], *B.BOX_EDIT[2], B.BOX_EDIT[3], 64, 6)
        assert cbb == cb2
        for m in range(2):
            assert np.array_equal(g.member(m).pool_download(cb2[3]), ctx.pool_download(cb2[3]))
    finally:
        g.close()


def test_jni_typed_brush_natives(pool64):
    """the natives as the JVM calls them (JNIEnv*, jclass, then primitives and memAddress() longs), with no tuning call"""
    from svo_raytracer_amd import hiplib
    L = hiplib.lib()
    vp, jint, jlong = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    P = "Java_src_engine_HipRenderer_"

    def fn(name, res, *args):
        f = getattr(L, P + name)
        f.restype = res
        f.argtypes = [vp, vp] + list(args)
        return lambda *a: f(None, None, *a)

    nCreate, nDestroy = fn("nCreate", jlong, jint), fn("nDestroy", jint, jlong)
    nPoolUpload = fn("nPoolUpload", jint, jlong, jlong, jlong)
    nPoolDownload = fn("nPoolDownload", jint, jlong, jlong, jlong)
    nPoolDownloadRange = fn("nPoolDownloadRange", jint, jlong, jlong, jlong, jlong)
    nBrushSphere = fn("nBrushSphere", jint, jlong, *([jint] * 7), jlong)
    nBrushBox = fn("nBrushBox", jint, jlong, *([jint] * 9), jlong)
    nBrushInfo = fn("nBrushInfo", jlong, jlong, jlong, jlong)
    chk = B.Checker(pool64)
    j = nCreate(0)
    assert j != 0
    try:
        assert nPoolUpload(j, pool64.ctypes.data, pool64.size) == 0
        mirror = np.zeros(pool64.size * 4, np.uint8)
        mirror[:pool64.size] = pool64
        cb = np.zeros(4, np.int32)
        counts, ms = np.zeros(4, np.int64), np.zeros(1, np.float32)
        for k, (kind, org, size, val) in enumerate(B.edits64()):
            want_cb, want = chk.stroke(kind, org, size, val, 64, 6)
            if kind == "sphere":
                assert nBrushSphere(j, *org, size, val, 64, 6, cb.ctypes.data) == 0
            else:
                assert nBrushBox(j, *org, *size, val, 64, 6, cb.ctypes.data) == 0
            assert [int(v) for v in cb] == want_cb
            assert nBrushInfo(j, counts.ctypes.data, ms.ctypes.data) == k + 1
            if counts[3] > counts[2]:
                assert nPoolDownloadRange(j, mirror.ctypes.data, int(counts[2]), int(counts[3])) == 0
            if cb[3] > cb[2]:
                assert nPoolDownloadRange(j, mirror.ctypes.data, int(cb[2]), int(cb[3])) == 0
            got = np.zeros(want.size, np.uint8)
            assert nPoolDownload(j, got.ctypes.data, got.size) == 0
            assert np.array_equal(got, want) and np.array_equal(mirror[:want.size], want)
            assert ms[0] > 0
        assert nBrushSphere(j, 1, 1, 1, 2, 300, 64, 6, 0) == -1
        assert nPoolDownloadRange(j, mirror.ctypes.data, -1, 4) == -1
    finally:
        assert nDestroy(j) == 0
