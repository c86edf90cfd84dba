"""The dense shading pass of a still camera's submissions (bounce_rays_kernel + persist_cast_kernel in svo_persistent.hip.h): a
launch that reads the primary-hit cache and whose paths are primary + one bounce shades every (pixel, frame) ahead of the walk and
casts the prepared rays.  Every byte must be what the same frames are with the cache switched off (persist_span_kernel), which are
checked against the CPU oracle (colour and depth bits).  The frame of tests/test_gpu_primary_cache.py, whose helpers and reference
frames this module shares: 76x44 has partial tiles right and below, 76x8 is one tile row (every wave off the first XCD steals), K0
sees sky.  The generator's small scenes give no primary hit with normal code 0 (terrain, dust and caves at 64^3 - 256^3, seeds
1 - 3, K0 / K1 / K2 on the CPU oracle: none); tests/fuzzpool.py's pools do, and one of them is a case here."""
import numpy as np
import pytest

import test_gpu_primary_cache as pc
from test_gpu_primary_cache import FIRST, H, NFRAMES, W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from svo_raytracer_amd import hiplib
    c = hiplib.HipContext(0)
    c.set_pipeline(1)
    yield c
    c.close()


def _equal(got, off, what):
    assert sorted(got) == sorted(off), what
    for fn in off:
        assert pc._same(got[fn], off[fn]), (what, fn)


@pytest.mark.parametrize("pool_name,cam_name,w,h", pc.CASES)
def test_steady_state_takes_the_dense_pass(ctx, pool_name, cam_name, w, h):
    pc._setup(ctx, pool_name, cam_name, w, h)
    off = pc._reference(ctx, pool_name, cam_name, w, h)
    if cam_name == "K0":
        assert (off[FIRST]["depth"] == 0).any()
    for batch in (2, 4, 7):          # 24 frames: the last submission of 7 is partial
        ctx.set_primary_cache(False); ctx.set_primary_cache(True)
        cache0, dense0 = ctx.primary_cache_info(), ctx.dense_shade_info()
        got = pc._frames(ctx, NFRAMES, batch, slots=3, wait_first=True)
        cache1, dense1 = ctx.primary_cache_info(), ctx.dense_shade_info()
        submissions = -(-NFRAMES // batch)
        rose = dense1["launches"] - dense0["launches"]
        assert rose >= submissions - 3 and rose >= 1, (batch, dense0, dense1)
        assert cache1["fills"] - cache0["fills"] == 1, (batch, cache0, cache1)
        assert dense1["bytes"] >= 20 * w * h * batch
        _equal(got, off, batch)


def test_longer_paths_and_hit_records_stay_in_the_walk(ctx):
    pc._setup(ctx, "terrain", "K1")
    for kw in (dict(bounces=3), dict(want_hits=True)):
        off = pc._off(ctx, 12, 4, slots=1, **kw)
        before = ctx.dense_shade_info()
        got = pc._frames(ctx, 12, 4, slots=1, **kw)
        assert ctx.dense_shade_info()["launches"] == before["launches"], kw
        _equal(got, off, kw)
    pc._check_oracle(pc._off(ctx, 4, 4, slots=1, bounces=3), pc._pool("terrain"), W, H, pc._cam("K1"), bounces=3, only=[FIRST])


def test_a_mirror_material_takes_the_dense_pass(ctx):
    pc._setup(ctx, "terrain", "K1")
    off = pc._off(ctx, 12, 4, slots=1, mirror=0b1000)
    pc._check_oracle(off, pc._pool("terrain"), W, H, pc._cam("K1"), mirror=0b1000, only=[FIRST, FIRST + 5])
    assert not pc._same(off[FIRST], pc._off(ctx, 4, 4, slots=1)[FIRST]), "the mirror material must be in view"
    before = ctx.dense_shade_info()
    got = pc._frames(ctx, 12, 4, slots=1, mirror=0b1000)
    assert ctx.dense_shade_info()["launches"] - before["launches"] == 2      # a fill, then two that read
    _equal(got, off, "mirror")


def test_a_stripe_of_rows(ctx):
    """set_rows(8, 32): the cache's and the ray records' index starts at the launch's first output row (kept_origin != 0)"""
    pc._setup(ctx, "terrain", "K1")
    full = pc._reference(ctx, "terrain", "K1", W, H)
    ctx.set_rows(8, 32)
    try:
        off = pc._off(ctx, 12, 4, slots=1)
        before = ctx.dense_shade_info()
        got = pc._frames(ctx, 12, 4, slots=1)
        assert ctx.dense_shade_info()["launches"] - before["launches"] == 2
        for fn in off:
            assert np.array_equal(got[fn]["rgba"][8:32], off[fn]["rgba"][8:32]), fn
            assert np.array_equal(got[fn]["depth"].view(np.uint32)[8:32], off[fn]["depth"].view(np.uint32)[8:32]), fn
            assert np.array_equal(got[fn]["rgba"][8:32], full[fn]["rgba"][8:32]), fn
    finally:
        ctx.set_rows(0, H)


def test_a_pool_update_between_two_submissions(ctx):
    """the cache drops and refills; the bytes follow the new pool"""
    A = pc._pool("terrain")
    pc._setup(ctx, "terrain", "K1")
    org = pc._centre_hit(A, pc._cam("K1"), W, H)
    pc._frames(ctx, 8, 4, slots=1)
    assert ctx.primary_cache_info()["state"] == 2
    cb = ctx.brush_sphere(org, 12, 3, 256, 8)
    B = ctx.pool_download(cb[3])
    ctx.pool_upload(A)
    old = pc._off(ctx, 20, 4, slots=1)
    pc._frames(ctx, 8, 4, slots=1)                  # the cache holds A again
    cache0, dense0 = ctx.primary_cache_info(), ctx.dense_shade_info()
    ctx.set_params(FIRST, 0, 0, 0, 2, 0, 1)
    ctx.ring_create(1, 4, want_hits=False)
    got = {}
    try:
        for b in range(5):
            if b == 2:
                ctx.pool_update(B, cb[0], cb[1])
                if cb[3] > cb[2]:
                    ctx.pool_update(B, cb[2], cb[3])
            s = ctx.ring_submit(FIRST + 4 * b, 4)
            ctx.ring_wait(s)
            for k in range(4):
                got[FIRST + 4 * b + k] = ctx.ring_read(s, k)
    finally:
        ctx.ring_destroy()
    cache1, dense1 = ctx.primary_cache_info(), ctx.dense_shade_info()
    assert cache1["fills"] - cache0["fills"] == 1, (cache0, cache1)                 # submission 2 refills
    assert dense1["launches"] - dense0["launches"] == 4, (dense0, dense1)        # ... every other one shades ahead of the walk
    new = pc._off(ctx, 20, 4, slots=1)
    pc._check_oracle(new, B, W, H, pc._cam("K1"), only=[FIRST + 8])
    assert not pc._same(new[FIRST + 8], old[FIRST + 8]), "the stroke must be in view"
    for fn in got:
        assert pc._same(got[fn], (old if fn < FIRST + 8 else new)[fn]), fn
    ctx.pool_upload(A)


def test_resize_and_back(ctx):
    pc._setup(ctx, "terrain", "K1")
    big = pc._reference(ctx, "terrain", "K1", W, H)
    pc._frames(ctx, 8, 4, slots=1)
    assert ctx.dense_shade_info()["bytes"] > 0
    ctx.resize(W, 8)
    assert ctx.dense_shade_info()["bytes"] == 0      # the ray records go with the frame's buffers
    small = pc._reference(ctx, "terrain", "K1", W, 8)
    before = ctx.dense_shade_info()
    _equal(pc._frames(ctx, 12, 4, slots=1), {fn: small[fn] for fn in range(FIRST, FIRST + 12)}, "76x8")
    assert ctx.dense_shade_info()["launches"] - before["launches"] == 2
    ctx.resize(W, H)
    before = ctx.dense_shade_info()
    _equal(pc._frames(ctx, 12, 4, slots=1), {fn: big[fn] for fn in range(FIRST, FIRST + 12)}, "76x44")
    assert ctx.dense_shade_info()["launches"] - before["launches"] == 2


def test_primary_hits_without_a_normal(ctx):
    """A voxel with normal code 0 gives scatter() a zero normal: a NaN direction, a cast that spins to the cap (quirk Q7) and NaN
    sums, so neither colour word of such a ray is black.  fuzzpool.random_pool(1) under K1: 1434 of 3344 primary hits are such
    (found with oracle.render(..., want_hits=True)), 37 primaries see sky."""
    import fuzzpool
    from oracle import oracle
    pool, cam = fuzzpool.random_pool(1), pc._cam("K1")
    ref = oracle.render(pool, W, H, cam, FIRST, 0, bounces=2, want_hits=True)
    hit = ref["hits"]["pointer"] != 0
    assert (hit & (ref["hits"]["raw_normal"] == 0)).sum() >= 1000 and (~hit).any()
    ctx.pool_upload(pool)
    ctx.resize(W, H)
    ctx.set_rows(0, H)
    ctx.set_camera(cam)
    try:
        off = pc._off(ctx, 12, 4, slots=1)
        pc._check_oracle(off, pool, W, H, cam, only=[FIRST, FIRST + 7])
        before = ctx.dense_shade_info()
        got = pc._frames(ctx, 12, 4, slots=1)
        assert ctx.dense_shade_info()["launches"] - before["launches"] == 2
        _equal(got, off, "fuzz pool 1")
    finally:
        ctx.pool_upload(pc._pool("terrain"))
