"""One context walked through every edge at which state of the host library ends -- the image size (svo_resize), the pool's
contents (svo_pool_upload), the context (svo_destroy) -- with every feature that keeps state of that lifetime in use: the beam
pre-pass's images and live-node table, the pick and its mail, the {stream, images} sets of svo_dispatch_async, the ring, the
persistent pipeline's buffers and its primary-hit cache, the descriptor table.  After every step the frames are the bytes a fresh
context gives, and (the dispatches) the oracle's.

A frame with the beam pre-pass carries no pick launch (include/svo_hip.h, svo_set_pick), so the pick of step 1 is read twice: at
the beam frames through the waiting path, and from the mail at one more dispatch without the pre-pass.  Step 5's waiting
svo_dispatch is a beam frame again: its read-back at the pick position waits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (40, 24))          # the second: 5 x 3 tiles and 10 x 6 beam blocks, no tile row and no tile column is whole
MODE = 0
SVO_E_INVALID = -1


@pytest.fixture(scope="module")
def pools():
    import svo_raytracer_amd.scene as scene
    return {"A": scene.build_scene(64, 1)[0], "B": scene.build_scene(64, 2)[0]}


def _cams():
    from svo_raytracer_amd.cameras import CAMERAS
    return CAMERAS["K1"], CAMERAS["K2"]


_fresh_cache = {}


def _fresh(pools, name, w, h):
    """every frame the walk compares, from a context that does nothing else: (camera index, frame number, use_beam) -> frame"""
    key = (name, w, h)
    if key not in _fresh_cache:
        from svo_raytracer_amd import hiplib
        c = hiplib.HipContext(0)
        try:
            c.set_overlap(0)
            c.pool_upload(pools[name])
            c.resize(w, h)
            out = {}
            for cam, fn, beam in ((0, 6, 1), (0, 7, 0), (0, 8, 1), (0, 10, 0), (0, 11, 0), (0, 1, 0), (1, 5, 0)):
                out[(cam, fn, beam)] = c.render(None, None, None, _cams()[cam], fn, MODE, use_beam=beam)
                if (cam, fn, beam) == (0, 6, 1):
                    out["beam"] = c.read_beam()
        finally:
            c.close()
        _fresh_cache[key] = out
    return _fresh_cache[key]


def _same(got, want, tag, hits=True):
    assert np.array_equal(got["rgba"], want["rgba"]), tag
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32)), tag
    if hits:
        assert np.array_equal(got["hits"].view(np.uint8), want["hits"].view(np.uint8)), tag


def _frame(ctx):
    return {"rgba": ctx.read_color(), "depth": ctx.read_depth(), "hits": ctx.read_hits()}


def _pixel_is(px, img, x, y, tag):
    rgba, depth, hit = px
    assert (rgba == img["rgba"][y, x]).all(), tag
    assert np.float32(depth).view(np.uint32) == img["depth"].view(np.uint32)[y, x], tag
    assert hit.tobytes() == img["hits"][y, x].tobytes(), tag


def _dispatches(ctx, pools, name, w, h, tag):
    """step 1: five overlapped beam frames on four sets (set 1 is used twice), the pick by waiting; one frame without the
    pre-pass, the pick from the mail"""
    from oracle import oracle
    fresh, (k1, _) = _fresh(pools, name, w, h), _cams()
    px, py = w // 2 + 3, h // 2 - 2
    ctx.set_camera(k1)
    ctx.set_overlap(4)
    ctx.set_pick(px, py)
    for fn in range(2, 7):
        ctx.set_params(fn, MODE, 0, 1, 2, 0, 1)
        ctx.dispatch_async()
    i0 = ctx.pick_info()
    pixel = ctx.read_pixel(px, py)
    i1 = ctx.pick_info()
    assert (i1["from_mail"], i1["waited"]) == (i0["from_mail"], i0["waited"] + 1), (tag, i0, i1)
    got = _frame(ctx)
    _pixel_is(pixel, got, px, py, tag)
    _same(got, fresh[(0, 6, 1)], tag + ("beam frame / fresh",))
    ref = oracle.render(pools[name], w, h, k1, 6, MODE, use_beam=True)
    _same(got, ref, tag + ("beam frame / oracle",))
    beam = ctx.read_beam()
    assert np.array_equal(beam.view(np.uint32), fresh["beam"].view(np.uint32)), tag
    assert np.array_equal(beam.view(np.uint32), ref["beam"].view(np.uint32)), tag
    ctx.set_params(7, MODE, 0, 0, 2, 0, 1)
    ctx.dispatch_async()
    pixel = ctx.read_pixel(px, py)
    i2 = ctx.pick_info()
    assert (i2["from_mail"], i2["waited"]) == (i1["from_mail"] + 1, i1["waited"]), (tag, i1, i2)
    got = _frame(ctx)
    _pixel_is(pixel, got, px, py, tag)
    _same(got, fresh[(0, 7, 0)], tag + ("frame / fresh",))
    _same(got, oracle.render(pools[name], w, h, k1, 7, MODE), tag + ("frame / oracle",))
    ctx.sync()


def _ring(ctx, pools, name, w, h, tag, create):
    """step 2: a ring of 2 slots x 2 frames; one submission of the context's camera, one of two cameras; then three waited
    submissions without hit records, which the primary-hit cache serves"""
    fresh, (k1, k2) = _fresh(pools, name, w, h), _cams()
    ctx.set_camera(k1)
    ctx.set_params(2, MODE, 0, 0, 2, 0, 1)
    if create:
        ctx.ring_create(2, 2, want_hits=True)
    s = ctx.ring_submit(10, 2)
    for k in range(2):
        _same(ctx.ring_read(s, k, want_hits=True), fresh[(0, 10 + k, 0)], tag + ("submit", k))
    s = ctx.ring_submit_cams(np.stack([k1, k2]), [1, 5])
    for k, key in enumerate(((0, 1, 0), (1, 5, 0))):
        _same(ctx.ring_read(s, k, want_hits=True), fresh[key], tag + ("submit_cams", k))
    ctx.set_hit_records(False)
    before = ctx.primary_cache_info()
    for b in range(3):
        s = ctx.ring_submit(10, 2)
        ctx.ring_wait(s)
        for k in range(2):
            _same(ctx.ring_read(s, k), fresh[(0, 10 + k, 0)], tag + ("cached", b, k), hits=False)
    after = ctx.primary_cache_info()
    ctx.set_hit_records(True)
    assert after["fills"] > before["fills"] and after["reuses"] > before["reuses"], (tag, before, after)


def test_one_context_through_every_lifetime_edge(pools):
    from svo_raytracer_amd import hiplib
    (w1, h1), (w2, h2) = SIZES
    ctx = hiplib.HipContext(0)
    try:
        ctx.pool_upload(pools["A"])
        ctx.resize(w1, h1)
        _dispatches(ctx, pools, "A", w1, h1, ("1",))
        _ring(ctx, pools, "A", w1, h1, ("2",), create=True)
        # 3. the image size ends: the ring is gone, everything else is made anew at the new size
        ctx.resize(w2, h2)
        with pytest.raises(hiplib.SvoError) as err:
            ctx.ring_submit(10, 2)
        assert err.value.code == SVO_E_INVALID
        _dispatches(ctx, pools, "A", w2, h2, ("3.1",))
        with pytest.raises(hiplib.SvoError) as err:
            ctx.ring_submit(10, 2)
        assert err.value.code == SVO_E_INVALID
        _ring(ctx, pools, "A", w2, h2, ("3.2",), create=True)
        # 4. the pool's contents end: the live-node table, the descriptor table and the primary-hit cache follow (the ring stays)
        ctx.pool_upload(pools["B"])
        assert not np.array_equal(_fresh(pools, "A", w2, h2)[(0, 7, 0)]["rgba"], _fresh(pools, "B", w2, h2)[(0, 7, 0)]["rgba"])
        _dispatches(ctx, pools, "B", w2, h2, ("4.1",))
        _ring(ctx, pools, "B", w2, h2, ("4.2",), create=False)
        # 5. one set, a waiting dispatch (a beam frame: no pick launch), the pick position by waiting
        ctx.set_overlap(0)
        ctx.set_params(8, MODE, 0, 1, 2, 0, 1)
        ctx.dispatch()
        i0 = ctx.pick_info()
        px, py = i0["x"], i0["y"]
        assert (px, py) == (w2 // 2 + 3, h2 // 2 - 2)
        pixel = ctx.read_pixel(px, py)
        i1 = ctx.pick_info()
        assert (i1["from_mail"], i1["waited"]) == (i0["from_mail"], i0["waited"] + 1), (i0, i1)
        got = _frame(ctx)
        _pixel_is(pixel, got, px, py, ("5",))
        _same(got, _fresh(pools, "B", w2, h2)[(0, 8, 1)], ("5",))
    finally:
        ctx.close()
    # 6. the context ended with all of it alive; a second one in the same process
    ctx = hiplib.HipContext(0)
    try:
        got = ctx.render(pools["B"], w2, h2, _cams()[0], 7, MODE)
        _same(got, _fresh(pools, "B", w2, h2)[(0, 7, 0)], ("6",))
    finally:
        ctx.close()
