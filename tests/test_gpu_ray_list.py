"""The dense pass with its ray records as a compact list (svo_persistent.hip.h: ray_list_kernel appends, per band, an entry for every
(pixel, frame) that casts a ray; persist_runs_kernel draws runs of consecutive entries).  The list is what the product library runs
(PersistSettings::list_mode, on by default); the pass as it was before -- a record per (frame, pixel), a slot per pixel -- stays as
the comparator and is run here through the variants library with SVO_RAY_LIST=0.  Every byte must be what the same frames are
with the cache switched off (persist_span_kernel), which are checked against the CPU oracle (colour and depth bits).  Helpers, pools
and reference frames are tests/test_gpu_primary_cache.py's: 76x44 has partial tiles right and below; 76x8 is one tile row, so seven
bands are empty, every wave off the first XCD steals and the fill is far below kChunk.  A camera turned at the sky leaves every
band empty, one looking straight down fills the list to its room.  The metadata check at the end reads the built code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_primary_cache as pc
from test_gpu_primary_cache import FIRST, H, NFRAMES, W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
HEAD_SETS = 8      # counter sets of a context, each with ray records of its own (svo_persistent.hip.h: kHeadSets)


@pytest.fixture(scope="module")
def ctx():
    from svo_raytracer_amd import hiplib
    c = hiplib.HipContext(0)
    c.set_pipeline(1)
    pc._setup(c, "terrain", "K1")
    before = c.dense_shade_info()
    pc._frames(c, 8, 4, slots=1)
    after = c.dense_shade_info()
    # a fill, then one launch that reads; 24 bytes per record: the list is on (a record per (frame, pixel) has 20)
    assert after["launches"] - before["launches"] == 1 and after["bytes"] == 24 * W * 48 * 4 * HEAD_SETS, (before, after)
    yield c
    c.close()


def test_the_comparator_a_record_per_frame_and_pixel():
    """SVO_RAY_LIST=0 on the variants library: bounce_rays_kernel + persist_cast_kernel, 20 bytes per record, the same bytes"""
    from svo_raytracer_amd import hiplib
    assert os.path.exists(hiplib.VARIANTS_LIB_PATH), "the variants library is not built"
    old = os.environ.get("SVO_RAY_LIST")
    os.environ["SVO_RAY_LIST"] = "0"      # read once, at the context's first launch
    c = hiplib.HipContext(0, lib_path=hiplib.VARIANTS_LIB_PATH)
    try:
        c.set_pipeline(1)
        for cam_name in ("K1", "K0"):
            pc._setup(c, "terrain", cam_name)
            off = pc._reference(c, "terrain", cam_name, W, H)
            before = c.dense_shade_info()
            got = pc._frames(c, 12, 4, slots=1)
            after = c.dense_shade_info()
            assert after["launches"] - before["launches"] == 2 and after["bytes"] == 20 * W * 48 * 4 * HEAD_SETS, (before, after)
            _equal(got, {fn: off[fn] for fn in got}, cam_name)
    finally:
        c.close()
        if old is None:
            del os.environ["SVO_RAY_LIST"]
        else:
            os.environ["SVO_RAY_LIST"] = old


def _equal(got, off, what):
    assert sorted(got) == sorted(off), what
    for fn in off:
        assert pc._same(got[fn], off[fn]), (what, fn)


def _camera(ctx, cam, w=W, h=H):
    """the terrain under a camera of this module's own, and its 12 cache-off frames checked against the oracle"""
    ctx.pool_upload(pc._pool("terrain"))
    ctx.resize(w, h)
    ctx.set_rows(0, h)
    ctx.set_camera(cam)
    off = pc._off(ctx, 12, 4, slots=1)
    pc._check_oracle(off, pc._pool("terrain"), w, h, cam, only=[FIRST, FIRST + 6])
    return off


@pytest.mark.parametrize("batch", [2, 4, 7])
def test_76x44_partial_tiles_and_a_partial_last_submission(ctx, batch):
    pc._setup(ctx, "terrain", "K1")
    off = pc._reference(ctx, "terrain", "K1", W, H)
    before = ctx.dense_shade_info()
    got = pc._frames(ctx, NFRAMES, batch, slots=3, wait_first=True)      # 24 frames: the last submission of 7 is partial
    submissions = -(-NFRAMES // batch)
    rose = ctx.dense_shade_info()["launches"] - before["launches"]
    # (three slots in flight, as tests/test_gpu_dense_shade.py has it: a submission made before the fill is seen complete casts its own)
    assert rose >= submissions - 3 and rose >= 1, (batch, rose)
    _equal(got, off, batch)
    # one slot: every submission behind the fill reads the cache and takes the pass
    ctx.set_primary_cache(False); ctx.set_primary_cache(True)
    before = ctx.dense_shade_info()
    got = pc._frames(ctx, NFRAMES, batch, slots=1)
    assert ctx.dense_shade_info()["launches"] - before["launches"] == submissions - 1, batch
    _equal(got, off, (batch, "one slot"))


@pytest.mark.parametrize("cam_name", ["K1", "K0"])
def test_76x8_one_tile_row_seven_empty_bands(ctx, cam_name):
    pc._setup(ctx, "terrain", cam_name, W, 8)
    off = pc._reference(ctx, "terrain", cam_name, W, 8)
    for batch in (2, 4, 7):
        ctx.set_primary_cache(False); ctx.set_primary_cache(True)
        before = ctx.dense_shade_info()
        got = pc._frames(ctx, NFRAMES, batch, slots=1)
        assert ctx.dense_shade_info()["launches"] - before["launches"] == -(-NFRAMES // batch) - 1, batch
        _equal(got, off, batch)


def test_a_camera_turned_at_the_sky_leaves_every_band_empty(ctx):
    from oracle import oracle
    from svo_raytracer_amd.cameras import rot_cam
    cam = rot_cam((1.5, 1.9, 1.5), 1.4, 0.3)
    ref = oracle.render(pc._pool("terrain"), W, H, cam, FIRST, 0, bounces=2, want_hits=False)
    assert (ref["depth"] == 0).all(), "the camera must see nothing but sky"
    off = _camera(ctx, cam)
    before = ctx.dense_shade_info()
    got = pc._frames(ctx, 12, 4, slots=1)
    assert ctx.dense_shade_info()["launches"] - before["launches"] == 2      # a fill, then two that read: both cast kernels ended
    _equal(got, off, "sky")
    for fn in got:
        assert (got[fn]["depth"] == 0).all() and np.array_equal(got[fn]["rgba"], ref["rgba"]), fn      # the same sky in every frame


def test_a_camera_looking_straight_down_fills_the_list_to_its_room(ctx):
    from oracle import oracle
    from svo_raytracer_amd.cameras import rot_cam
    cam = rot_cam((1.5, 1.5, 1.5), -np.pi / 2, 0.0)
    ref = oracle.render(pc._pool("terrain"), W, 40, cam, FIRST, 0, bounces=2, want_hits=True)
    assert (ref["hits"]["pointer"] != 0).all(), "every primary ray must hit"
    off = _camera(ctx, cam, W, 40)      # whole tile rows: no record's room is left over
    for batch in (4, 7):
        ctx.set_primary_cache(False); ctx.set_primary_cache(True)
        before = ctx.dense_shade_info()
        got = pc._frames(ctx, 12, batch, slots=1)
        assert ctx.dense_shade_info()["launches"] - before["launches"] == -(-12 // batch) - 1
        _equal(got, off, batch)


def test_a_stripe_of_rows(ctx):
    """set_rows(8, 32): a record's cache index starts at the launch's first output row (kept_origin != 0)"""
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


def test_nan_directions_pass_through_the_list(ctx):
    """tests/test_gpu_dense_shade.py's fuzz pool: 1434 of 3344 primary hits have normal code 0, so their bounce direction is NaN"""
    import fuzzpool
    pool, cam = fuzzpool.random_pool(1), pc._cam("K1")
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


def test_counts(ctx):
    pc._setup(ctx, "terrain", "K1")
    ctx.resize(W, 8); ctx.resize(W, H)      # the ray records go with the frame's buffers
    assert ctx.dense_shade_info()["bytes"] == 0
    before = ctx.dense_shade_info()
    pc._frames(ctx, 12, 4, slots=1)
    after = ctx.dense_shade_info()
    assert after["launches"] - before["launches"] == 2      # a fill, then two that read
    records = W * 48 * 4                                    # whole tile rows x frames
    assert after["bytes"] == 24 * records * HEAD_SETS, after


def test_cast_kernels_keep_seven_waves_per_simd(tmp_path):
    """the built code object's metadata, read as tests/test_kernel_isa_kept.py reads it, for persist_cast_kernel and for the list's
    persist_runs_kernel: at most 72 VGPRs and no private segment = 7 waves per SIMD, and the stack as the kernel's only LDS"""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools not installed")
    so = shutil.copy(os.path.join(ROOT, "svo-raytracer_amd", "csrc", "libsvohip.so"), tmp_path)
    subprocess.check_call([OBJDUMP, "--offloading", so], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp_path)
    co = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert len(co) == 1, os.listdir(tmp_path)
    notes = subprocess.check_output([READELF, "--notes", os.path.join(tmp_path, co[0])], text=True)
    found, cur = {}, {}
    for line in notes.splitlines():
        if re.match(r"\s*- \.agpr_count:", line):
            cur = {}
        m = re.match(r"\s*(?:- )?\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        if m.group(2).isdigit():
            cur[m.group(1)] = int(m.group(2))
        elif m.group(1) == "name" and ("persist_cast_kernel" in m.group(2) or "persist_runs_kernel" in m.group(2)):
            found[m.group(2)] = cur
    assert len(found) == 2, sorted(found)
    for name, meta in found.items():
        assert meta["vgpr_count"] <= 72 and meta["agpr_count"] == 0, (name, meta)
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["group_segment_fixed_size"] == 6144, (name, meta)
