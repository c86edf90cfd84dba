"""The primary-hit cache of a still camera (svo_set_primary_cache, persist_kept_kernel in svo_persistent.hip.h): consecutive
static-camera batches under one camera, pool and frame keep the primary hits of one submission (the fill) and shade later
submissions from them (reuse).  Every byte must be what the same frames are with the cache switched off, which are checked
against the CPU oracle (colour and depth bits).  Small shapes: 76x44 has partial tiles right and below, 76x8 is one tile row
(every wave off the first XCD steals), K0 sees sky; hit records are off (with them a submission stays on persist_span_kernel)."""
import numpy as np
import pytest

import poolcache

pytestmark = pytest.mark.gpu

W, H = 76, 44
FIRST = 2
NFRAMES = 24


def _pool(name):
    import svo_raytracer_amd.scene as scene
    return poolcache.pool("terrain", 256) if name == "terrain" else poolcache.pool("dust", 128, dens=scene.DUST_DENS)


def _cam(name):
    from svo_raytracer_amd.cameras import CAMERAS
    return CAMERAS[name]


@pytest.fixture(scope="module")
def ctx():
    from svo_raytracer_amd import hiplib
    c = hiplib.HipContext(0)
    c.set_pipeline(1)
    yield c
    c.close()


def _frames(ctx, count, batch, slots=3, wait_first=False, first=FIRST, mode=0, bounces=2, mirror=0, spp=1, cams=None,
            want_hits=False, log=None):
    """frames first .. first + count - 1 through a ring, `batch` per submission, as many submissions in flight as there are
    slots; wait_first: the first submission is waited for before the second is made.  log receives svo_primary_cache_info
    after every submission."""
    ctx.set_params(first, mode, 0, 0, bounces, mirror, spp)
    ctx.ring_create(slots, batch, want_hits=want_hits)
    out, pending, f, end = {}, [], first, first + count
    try:
        while f < end or pending:
            if f < end and len(pending) < slots:
                n = min(batch, end - f)
                if cams is None:
                    slot = ctx.ring_submit(f, n)
                else:
                    slot = ctx.ring_submit_cams([cams[k - first] for k in range(f, f + n)], list(range(f, f + n)))
                if log is not None:
                    log.append(ctx.primary_cache_info())
                pending.append((slot, f, n))
                f += n
                if not (wait_first and f == first + n):
                    continue
            slot, f0, n = pending.pop(0)
            ctx.ring_wait(slot)
            for k in range(n):
                out[f0 + k] = ctx.ring_read(slot, k)
    finally:
        ctx.ring_destroy()
    return out


def _same(a, b):
    return np.array_equal(a["rgba"], b["rgba"]) and np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))


def _off(ctx, count, batch, **kw):
    """the reference bytes: the same frames with the cache switched off (the cache is empty afterwards)"""
    ctx.set_primary_cache(False)
    try:
        return _frames(ctx, count, batch, **kw)
    finally:
        ctx.set_primary_cache(True)


def _check_oracle(frames, pool, w, h, cam, bounces=2, mirror=0, only=None):
    from oracle import oracle
    for fn in (sorted(frames) if only is None else only):
        ref = oracle.render(pool, w, h, cam, fn, 0, bounces=bounces, mirror_mask=mirror, want_hits=False)
        assert _same(frames[fn], ref), fn


def _setup(ctx, pool_name, cam_name, w=W, h=H):
    ctx.pool_upload(_pool(pool_name))
    ctx.resize(w, h)
    ctx.set_rows(0, h)
    ctx.set_camera(_cam(cam_name))
    assert ctx.primary_cache_info()["state"] == 0


_refs = {}


def _reference(ctx, pool_name, cam_name, w, h):
    """24 frames with the cache off, checked against the oracle; once per case, shared"""
    key = (pool_name, cam_name, w, h)
    if key not in _refs:
        off = _off(ctx, NFRAMES, 4)
        _check_oracle(off, _pool(pool_name), w, h, _cam(cam_name))
        _refs[key] = off
    return _refs[key]


CASES = [("terrain", "K1", W, H), ("terrain", "K0", W, H), ("dust", "K1", W, H), ("dust", "K0", W, H),
         ("terrain", "K1", W, 8), ("terrain", "K0", W, 8)]


@pytest.mark.parametrize("pool_name,cam_name,w,h", CASES)
def test_steady_state_fills_once_and_reuses(ctx, pool_name, cam_name, w, h):
    _setup(ctx, pool_name, cam_name, w, h)
    off = _reference(ctx, pool_name, cam_name, w, h)
    if cam_name == "K0":
        assert (off[FIRST]["depth"] == 0).any()
    for batch in (2, 4, 7):
        ctx.set_primary_cache(False); ctx.set_primary_cache(True)      # empty: this batch size fills for itself
        before, log = ctx.primary_cache_info(), []
        got = _frames(ctx, NFRAMES, batch, wait_first=True, log=log)
        after = ctx.primary_cache_info()
        submissions = -(-NFRAMES // batch)
        assert after["fills"] - before["fills"] == 1, (batch, before, after)
        assert log[0]["fills"] - before["fills"] == 1 and log[0]["state"] in (1, 2), log[0]
        assert after["reuses"] - before["reuses"] >= submissions - 1, (batch, before, after)
        assert after["state"] == 2 and after["bytes"] >= 48 * w * h
        assert sorted(got) == sorted(off)
        for fn in got:
            assert _same(got[fn], off[fn]), (batch, fn)


@pytest.mark.parametrize("pool_name,cam_name,w,h", CASES)
def test_nothing_waited_for(ctx, pool_name, cam_name, w, h):
    """all slots in flight from the start: whichever kernel a submission ran, the bytes are the same"""
    _setup(ctx, pool_name, cam_name, w, h)
    off = _reference(ctx, pool_name, cam_name, w, h)
    for batch in (2, 4, 7):
        ctx.set_primary_cache(False); ctx.set_primary_cache(True)
        got = _frames(ctx, NFRAMES, batch)
        for fn in off:
            assert _same(got[fn], off[fn]), (batch, fn)


def _centre_hit(pool, cam, w, h):
    """world position (voxels of the 256^3 terrain) of what the centre pixel's primary ray hits"""
    from oracle import oracle
    t = float(oracle.render(pool, w, h, cam, FIRST, 3, want_hits=False)["depth"][h // 2, w // 2])
    assert t > 0
    c = np.asarray(cam, dtype=np.float64).reshape(5, 3)
    u, v = (w // 2 + 0.5) / w, (h // 2 + 0.5) / h
    a, b = c[1] + (c[2] - c[1]) * v, c[3] + (c[4] - c[3]) * v
    d = a + (b - a) * u
    d /= np.linalg.norm(d)
    return tuple(int(x) for x in ((c[0] + d * t - 1.0) * 256.0))


def _round(ctx, ref_pool=None, w=W, h=H, cam="K1", bounces=2, mirror=0, expect_fill=True):
    """after a change: three waited submissions of 4 frames.  The first is no reuse, a later one fills (unless the caller
    expects reuse to go on: expect_fill False), and the frames are those of the cache switched off; returns them."""
    before, log = ctx.primary_cache_info(), []
    got = _frames(ctx, 12, 4, slots=1, log=log, bounces=bounces, mirror=mirror)
    if expect_fill:
        assert log[0]["reuses"] == before["reuses"], (before, log)
        assert log[-1]["fills"] > before["fills"], (before, log)
        assert log[-1]["reuses"] > before["reuses"], (before, log)      # and the one behind the fill reuses
    else:
        assert log[-1]["fills"] == before["fills"] and log[-1]["reuses"] - before["reuses"] == 3, (before, log)
    off = _off(ctx, 12, 4, slots=1, bounces=bounces, mirror=mirror)
    for fn in off:
        assert _same(got[fn], off[fn]), fn
    if ref_pool is not None:
        _check_oracle(off, ref_pool, w, h, _cam(cam), bounces, mirror, only=[FIRST])
    # (_off left the cache empty: fill it again, so that the next change meets a ready cache)
    _frames(ctx, 8, 4, slots=1)
    assert ctx.primary_cache_info()["state"] == 2
    return off


def test_invalidation(ctx):
    import torch
    from svo_raytracer_amd.tiles import stripe_layout
    A = _pool("terrain")
    _setup(ctx, "terrain", "K1")
    base = _round(ctx, A)
    # camera
    ctx.set_camera(_cam("K0"))
    k0 = _round(ctx, A, cam="K0")
    assert not _same(k0[FIRST], base[FIRST])
    ctx.set_camera(_cam("K1"))
    assert _same(_round(ctx)[FIRST], base[FIRST])
    # a brush sphere in view, on the device
    org = _centre_hit(A, _cam("K1"), W, H)
    cb = ctx.brush_sphere(org, 12, 3, 256, 8)
    B = ctx.pool_download(cb[3])
    brushed = _round(ctx, B)
    assert not _same(brushed[FIRST], base[FIRST]), "the stroke must be in view"
    ctx.pool_upload(A)
    assert _same(_round(ctx)[FIRST], base[FIRST])
    # the same stroke as the host's two ranged updates, and back
    ctx.pool_update(B, cb[0], cb[1])
    if cb[3] > cb[2]:
        ctx.pool_update(B, cb[2], cb[3])
    assert _same(_round(ctx)[FIRST], brushed[FIRST])
    ctx.pool_update(A, cb[0], cb[1])
    assert _same(_round(ctx)[FIRST], base[FIRST])
    # compaction (the stroke's records are unreachable now): other offsets, the same image
    ctx.pool_compact()
    assert _same(_round(ctx)[FIRST], base[FIRST])
    # bounces and the mirror mask are no part of the key
    ctx.pool_upload(A)
    _round(ctx)
    _round(ctx, A, bounces=3, expect_fill=False)
    _round(ctx, A, mirror=0b1000, expect_fill=False)
    # resize, and back
    ctx.resize(W, 8)
    _round(ctx, A, h=8)
    ctx.resize(W, H)
    assert _same(_round(ctx)[FIRST], base[FIRST])
    # a row band
    ctx.set_rows(8, 32)
    rows = _round(ctx)
    assert np.array_equal(rows[FIRST]["rgba"][8:32], base[FIRST]["rgba"][8:32])
    ctx.set_rows(0, H)
    assert _same(_round(ctx)[FIRST], base[FIRST])
    # rank 1 of 3's stripes, packed into bound outputs
    first, step, n, _, srows = stripe_layout(H, 3, 1)
    col = torch.zeros((4, srows, W), dtype=torch.int32, device="cuda")
    dep = torch.zeros((4, srows, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.set_stripes(first, step, n, 0)
    ctx.set_params(FIRST, 0, 0, 0, 2, 0, 1)
    ctx.ring_create(1, 4, want_hits=False)
    try:
        ctx.ring_bind_slot(0, col.data_ptr(), dep.data_ptr(), 0, srows * W)
        infos = [ctx.primary_cache_info()]
        for b in range(3):
            ctx.ring_wait(ctx.ring_submit(FIRST + 4 * b, 4))
            infos.append(ctx.primary_cache_info())
            for k in range(4):
                want = base[FIRST + 4 * b + k]
                c = col[k].cpu().numpy().view(np.uint8).reshape(srows, W, 4)
                d = dep[k].cpu().numpy().view(np.uint32)
                for j in range(n):
                    y = (first + j * step) * 8
                    ys = min(8, H - y)
                    assert np.array_equal(c[8 * j:8 * j + ys], want["rgba"][y:y + ys]), (b, k, j)
                    assert np.array_equal(d[8 * j:8 * j + ys], want["depth"].view(np.uint32)[y:y + ys]), (b, k, j)
        assert infos[1]["reuses"] == infos[0]["reuses"] and infos[1]["fills"] == infos[0]["fills"] + 1, infos
        assert infos[3]["reuses"] == infos[0]["reuses"] + 2, infos
    finally:
        ctx.ring_destroy()
        ctx.set_rows(0, H)
    assert _same(_round(ctx)[FIRST], base[FIRST])


def test_camera_change_with_launches_in_flight(ctx):
    """nothing is waited for between the views: earlier submissions show the old view, later ones the new"""
    _setup(ctx, "terrain", "K1")
    k1 = _reference(ctx, "terrain", "K1", W, H)
    ctx.set_camera(_cam("K0"))
    k0 = _reference(ctx, "terrain", "K0", W, H)
    ctx.set_camera(_cam("K1"))
    _frames(ctx, 8, 4, slots=1)                      # the cache holds K1
    assert ctx.primary_cache_info()["state"] == 2
    ctx.set_params(FIRST, 0, 0, 0, 2, 0, 1)
    ctx.ring_create(6, 4, want_hits=False)
    try:
        slots = []
        for b in range(6):
            if b == 3:
                ctx.set_camera(_cam("K0"))
            slots.append(ctx.ring_submit(FIRST + 4 * b, 4))
        for b, s in enumerate(slots):
            ctx.ring_wait(s)
            for k in range(4):
                want = (k1 if b < 3 else k0)[FIRST + 4 * b + k]
                assert _same(ctx.ring_read(s, k), want), (b, k)
    finally:
        ctx.ring_destroy()
        ctx.set_camera(_cam("K1"))


def test_a_camera_that_sees_only_sky(ctx):
    """every primary misses: a reuse launch never traverses, must still end, and writes the sky into every frame"""
    from oracle import oracle
    cam = np.array(_cam("K0"), dtype=np.float32).reshape(5, 3).copy()
    mean = cam[1:].sum(axis=0)
    cam[0] = 1.5 + 4.0 * mean / np.linalg.norm(mean)     # K0's corner rays from an eye that has the cube [1, 2)^3 behind it
    _setup(ctx, "terrain", "K0")
    ctx.set_camera(cam)
    ref = oracle.render(_pool("terrain"), W, H, cam, FIRST, 3, want_hits=False)
    assert (ref["depth"] == 0).all(), "the oracle must see only misses"
    before, log = ctx.primary_cache_info(), []
    got = _frames(ctx, 12, 4, slots=1, log=log)
    assert log[-1]["fills"] - before["fills"] == 1 and log[-1]["reuses"] - before["reuses"] == 2, (before, log)
    off = _off(ctx, 12, 4, slots=1)
    _check_oracle(off, _pool("terrain"), W, H, cam, only=[FIRST, FIRST + 5])
    for fn in off:
        assert _same(got[fn], off[fn]), fn
        assert (got[fn]["depth"] == 0).all()
    ctx.set_camera(_cam("K1"))


def test_ineligible_paths_do_not_use_the_cache(ctx):
    _setup(ctx, "terrain", "K1")
    before = ctx.primary_cache_info()
    cams = [_cam(n) for n in ("K1", "K0", "K1", "K0", "K1", "K1", "K1", "K1")]
    _frames(ctx, 8, 4, slots=1, want_hits=True)
    ctx.set_primary_cache(False)
    _frames(ctx, 8, 4, slots=1)
    ctx.set_primary_cache(True)
    _frames(ctx, 8, 4, slots=1, cams=cams)
    ctx.set_camera(_cam("K1"))
    for kw in (dict(mode=2), dict(spp=4), dict(bounces=1)):
        _frames(ctx, 8, 4, slots=1, **kw)
    after = ctx.primary_cache_info()
    assert after["reuses"] == before["reuses"] == after["reuses"] and after["fills"] == before["fills"], (before, after)
    assert after["state"] == 0


def test_settings_and_counts_survive_a_resize(ctx):
    """svo_resize frees the persistent pipeline's buffers, not what the host set: svo_set_tuning's launch shape, the cache's
    opt-out and the counts svo_primary_cache_info reports are the same after a resize to another size and back."""
    _setup(ctx, "terrain", "K1", 64, 64)
    _frames(ctx, 4, 2, slots=1)                        # a fill and a reuse: the counts are not zero
    before = ctx.primary_cache_info()
    assert before["fills"] >= 1 and before["reuses"] >= 1, before
    ctx.set_tuning(3, 11)
    ctx.set_primary_cache(False)
    try:
        ctx.resize(32, 32)
        ctx.resize(64, 64)
        ctx.set_params(FIRST, 0, 0, 0, 2, 0, 1)
        ctx.dispatch()
        assert ctx.launch_info() == {"waves": 64, "waves_per_cu": 3, "round_threshold_sixteenths": 11}   # 64 tiles < 3 waves x CUs
        _frames(ctx, 2, 2, slots=1)                    # a static-camera batch: would fill
        after = ctx.primary_cache_info()
        assert after["fills"] == before["fills"] and after["reuses"] == before["reuses"], (before, after)
        assert after["state"] == 0
    finally:
        ctx.set_tuning(0, 0)
        ctx.set_primary_cache(True)
