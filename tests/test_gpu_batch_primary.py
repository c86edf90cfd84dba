"""A static-camera batch (svo_ring_submit: consecutive frame numbers under one camera) casts the primary ray of a pixel ONCE for
all its frames in render mode 0 (persist_span_kernel, svo_persistent.hip.h): a band slot is a pixel, the lane runs frame 0's
path, frame 1's, ... from the one primary hit.  Every byte of colour, depth and hit record must be what a launch per frame
writes, and what the CPU oracle computes.  Small shapes only: 76x44 has partial tiles on the right and bottom edge, K0 sees sky
(primary misses), 7 frames per submission in 3 slots leaves a partial last batch and makes the slots wrap."""
import numpy as np
import pytest

import poolcache

pytestmark = pytest.mark.gpu

W, H = 76, 44
FIRST = 2
NFRAMES = 24           # 7 + 7 + 7 + 3: a partial last batch, and the fourth submission goes into a slot used before
TILES = ((W + 7) // 8) * ((H + 7) // 8)      # 60
SETTINGS = [(2, 0), (3, 0), (2, 0b1000), (3, 0b1000)]      # (bounces, mirror mask)


def _pool(name):
    import svo_raytracer_amd.scene as scene
    return poolcache.pool("terrain", 256) if name == "terrain" else poolcache.pool("dust", 128, dens=scene.DUST_DENS)


@pytest.fixture(scope="module")
def ctx():
    from svo_raytracer_amd import hiplib
    c = hiplib.HipContext(0)
    c.set_pipeline(1)
    yield c
    c.close()


def _ring_frames(ctx, first, count, batch, slots=3, mode=0, bounces=2, mirror=0, spp=1, cams=None, shapes=None):
    """frames first .. first + count - 1 through a ring of `slots` slots, `batch` frames per submission (the last one may be
    partial); as many submissions in flight as there are slots, a slot is read just before it is used again.
    cams: a camera per frame -> svo_ring_submit_cams.
    shapes: a list that receives (frames, persistent waves launched) of every submission (svo_launch_info): a launch never has
    more waves than tile slots, so at these sizes the figure tells a slot per pixel (tiles) from a slot per frame and pixel
    (tiles x frames x samples)."""
    ctx.set_params(first, mode, 0, 0, bounces, mirror, spp)
    ctx.ring_create(slots, batch, want_hits=True)
    out, pending, f, end = {}, [], first, first + count
    try:
        while f < end or pending:
            if f < end and len(pending) < slots:
                n = min(batch, end - f)
                if cams is None:
                    slot = ctx.ring_submit(f, n)
                else:
                    slot = ctx.ring_submit_cams([cams[k - first] for k in range(f, f + n)], list(range(f, f + n)))
                pending.append((slot, f, n))
                if shapes is not None:
                    shapes.append((n, ctx.launch_info()["waves"]))
                f += n
                continue
            slot, f0, n = pending.pop(0)
            ctx.ring_wait(slot)
            for k in range(n):
                out[f0 + k] = ctx.ring_read(slot, k, want_hits=True)
    finally:
        ctx.ring_destroy()
    return out


def _same(a, b):
    return (np.array_equal(a["rgba"], b["rgba"]) and np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
            and a["hits"].tobytes() == b["hits"].tobytes())


def _check_oracle(got, ref, tag):
    assert np.array_equal(got["rgba"], ref["rgba"]), tag
    assert np.array_equal(got["depth"].view(np.uint32), ref["depth"].view(np.uint32)), tag
    for k in ("pointer", "value", "raw_normal", "level", "iter"):
        assert np.array_equal(got["hits"][k], ref["hits"][k]), (tag, k)


_alone = {}


def _references(ctx, pool_name, cam_name, bounces, mirror, w=W, h=H, count=NFRAMES):
    """the frames one per launch (batch 1), checked against the oracle; computed once per case and shared"""
    from oracle import oracle
    from svo_raytracer_amd.cameras import CAMERAS
    key = (pool_name, cam_name, bounces, mirror, w, h)
    if key not in _alone:
        one = _ring_frames(ctx, FIRST, count, 1, bounces=bounces, mirror=mirror)
        for fn, got in one.items():
            ref = oracle.render(_pool(pool_name), w, h, CAMERAS[cam_name], fn, 0, bounces=bounces, mirror_mask=mirror)
            _check_oracle(got, ref, (key, fn))
        _alone[key] = one
    return _alone[key]


def _setup(ctx, pool_name, cam_name, w=W, h=H):
    from svo_raytracer_amd.cameras import CAMERAS
    ctx.pool_upload(_pool(pool_name))
    ctx.resize(w, h)
    ctx.set_camera(CAMERAS[cam_name])


@pytest.mark.parametrize("bounces,mirror", SETTINGS)
@pytest.mark.parametrize("cam_name", ["K1", "K0"])
@pytest.mark.parametrize("pool_name", ["terrain", "dust"])
def test_frames_of_a_batch_equal_frames_rendered_alone(ctx, pool_name, cam_name, bounces, mirror):
    """batches of 2, 3, 4 and 7 frames == the same frame numbers with one frame per launch == the oracle: colour, depth bits,
    hit records.  Batches of 2, 3 and 4 render the first 8 frames (several consecutive submissions: both walking directions);
    batches of 7 render all 24 (7 + 7 + 7 + 3 in three slots)."""
    _setup(ctx, pool_name, cam_name)
    alone = _references(ctx, pool_name, cam_name, bounces, mirror)
    if cam_name == "K0":
        assert (alone[FIRST]["hits"]["pointer"] == 0).any(), "K0 must see sky"
    assert not np.array_equal(alone[FIRST]["rgba"], alone[FIRST + 1]["rgba"])     # frames of a batch really differ
    for batch, count in ((2, 8), (3, 8), (4, 8), (7, NFRAMES)):
        shapes = []
        got = _ring_frames(ctx, FIRST, count, batch, bounces=bounces, mirror=mirror, shapes=shapes)
        assert sorted(got) == list(range(FIRST, FIRST + count))
        # the kernel that casts the primary once really ran: one slot per pixel = 60 tiles' worth of waves, whatever the batch
        assert [n for n, _ in shapes] == [min(batch, count - k) for k in range(0, count, batch)]
        assert all(waves == TILES for _, waves in shapes), shapes
        for fn in got:
            assert _same(got[fn], alone[fn]), (batch, fn)


def test_two_consecutive_submissions_walk_both_ways(ctx):
    """consecutive launches walk a band's columns in opposite directions (PersistArgs::reverse): two submissions of 4 frames"""
    _setup(ctx, "terrain", "K1")
    alone = _references(ctx, "terrain", "K1", 2, 0)
    ctx.set_params(FIRST, 0, 0, 0, 2, 0, 1)
    ctx.ring_create(2, 4, want_hits=True)
    try:
        s0 = ctx.ring_submit(FIRST, 4)
        assert ctx.launch_info()["waves"] == TILES          # one slot per pixel: the primary is cast once
        s1 = ctx.ring_submit(FIRST + 4, 4)
        assert ctx.launch_info()["waves"] == TILES
        for s, f0 in ((s0, FIRST), (s1, FIRST + 4)):
            ctx.ring_wait(s)
            for k in range(4):
                assert _same(ctx.ring_read(s, k, want_hits=True), alone[f0 + k]), (s, k)
    finally:
        ctx.ring_destroy()


def test_stripes_of_one_rank_of_three(ctx):
    """rank 1 of 3 renders every third tile row, packed, into buffers bound to the slots (what FrameRing sets up)"""
    import torch
    from svo_raytracer_amd import hiplib
    from svo_raytracer_amd.tiles import stripe_layout
    _setup(ctx, "terrain", "K1")
    alone = _references(ctx, "terrain", "K1", 2, 0)
    first, step, n, _, rows = stripe_layout(H, 3, 1)
    nb = 4
    col = [torch.zeros((nb, rows, W), dtype=torch.int32, device="cuda") for _ in range(2)]
    dep = [torch.zeros((nb, rows, W), dtype=torch.float32, device="cuda") for _ in range(2)]
    hit = [torch.zeros((nb, rows, W, 4), dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    ctx.set_stripes(first, step, n, 0)
    ctx.set_params(FIRST, 0, 0, 0, 2, 0, 1)
    ctx.ring_create(2, nb, want_hits=True)
    try:
        for b in range(2):
            ctx.ring_bind_slot(b, col[b].data_ptr(), dep[b].data_ptr(), hit[b].data_ptr(), rows * W)
        slots = []
        for b in range(2):
            slots.append(ctx.ring_submit(FIRST + b * nb, nb))
            assert ctx.launch_info()["waves"] == n * ((W + 7) // 8)      # one slot per pixel of the rank's n tile rows
        for b, s in enumerate(slots):
            ctx.ring_wait(s)
            for k in range(nb):
                want = alone[FIRST + b * nb + k]
                c = col[s][k].cpu().numpy().view(np.uint8).reshape(rows, W, 4)
                d = dep[s][k].cpu().numpy().view(np.uint32)
                hr = hit[s][k].cpu().numpy().reshape(-1, 4).copy().view(hiplib.HIT_DTYPE).reshape(rows, W)
                for j in range(n):
                    y = (first + j * step) * 8
                    ys = min(8, H - y)
                    assert np.array_equal(c[8 * j:8 * j + ys], want["rgba"][y:y + ys]), (b, k, j)
                    assert np.array_equal(d[8 * j:8 * j + ys], want["depth"].view(np.uint32)[y:y + ys]), (b, k, j)
                    assert hr[8 * j:8 * j + ys].tobytes() == want["hits"][y:y + ys].tobytes(), (b, k, j)
    finally:
        ctx.ring_destroy()
        ctx.set_rows(0, H)


@pytest.mark.parametrize("cam_name", ["K1", "K0"])
def test_a_frame_of_one_tile_row(ctx, cam_name):
    """76x8: one tile row, so seven of the eight bands are empty and every wave off the first XCD steals"""
    _setup(ctx, "terrain", cam_name, W, 8)
    alone = _references(ctx, "terrain", cam_name, 2, 0, W, 8, 8)
    shapes = []
    got = _ring_frames(ctx, FIRST, 8, 4, shapes=shapes)
    assert shapes == [(4, (W + 7) // 8)] * 2, shapes       # one slot per pixel
    for fn in got:
        assert _same(got[fn], alone[fn]), fn


def test_paths_that_keep_a_slot_per_frame(ctx):
    """frames with their own cameras (svo_ring_submit_cams), a mode-2 batch, a batch with 4 samples per pixel and a batch of
    primary rays alone (bounces 1): a slot per frame and pixel as before (the launch shape says so), bytes as before"""
    from svo_raytracer_amd.cameras import CAMERAS
    _setup(ctx, "terrain", "K1")
    cams = [CAMERAS[n] for n in ("K1", "K0", "K1", "K0", "K1", "K1")]
    alone = _ring_frames(ctx, FIRST, 6, 1, cams=cams)
    shapes = []
    got = _ring_frames(ctx, FIRST, 6, 3, cams=cams, shapes=shapes)
    assert shapes == [(3, 3 * TILES)] * 2, shapes
    for fn in got:
        assert _same(got[fn], alone[fn]), ("cams", fn)
    assert not np.array_equal(alone[FIRST]["rgba"], alone[FIRST + 1]["rgba"])
    ctx.set_camera(CAMERAS["K1"])
    for tag, kw, per_pixel in (("mode 2", dict(mode=2), 1), ("spp 4", dict(spp=4), 4), ("bounces 1", dict(bounces=1), 1)):
        alone = _ring_frames(ctx, FIRST, 6, 1, **kw)
        shapes = []
        got = _ring_frames(ctx, FIRST, 6, 3, shapes=shapes, **kw)
        assert shapes == [(3, 3 * per_pixel * TILES)] * 2, (tag, shapes)
        for fn in got:
            assert _same(got[fn], alone[fn]), (tag, fn)
