"""svo_cast_rays / svo_cast_rays_device / svo_cast_info (csrc/svo_rays.hip.h): caller-supplied rays through the octree.
Every comparison is byte equality of the 16-byte hit records, against two independent checkers (tests/rays_helpers.py):
(A) the oracle's cast of one ray, (B) the hit records of the frame whose pixel rays are cast -- for the golden cases the
reference shader's own."""
import ctypes

import numpy as np
import pytest

import svo_raytracer_amd.scene as scene
from svo_raytracer_amd import hiplib
from svo_raytracer_amd.cameras import CAMERAS
from oracle import oracle
from helpers import compare_with_golden, golden_case
import rays_helpers as R

pytestmark = pytest.mark.gpu

LIBS = {"asm": hiplib.LIB_PATH, "cxxloop": hiplib.CXXLOOP_LIB_PATH}
GOLDENS = [("s128_K1_m0", "s128"), ("s128_K2_m2", "s128"), ("s64_K0_m2_odd", "s64"), ("s128k6_K1_m0", "s128k6"),
           ("dust256_KDUST_m2", "dust256"), ("s64sdf_KEDIT_m0", "s64sdf")]


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(lib):
        if lib not in made:
            made[lib] = hiplib.HipContext(0, lib_path=LIBS[lib])
        return made[lib]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture()
def ctx():
    c = hiplib.HipContext()
    yield c
    c.close()


def _same(got, want, tag=None):
    bad = np.flatnonzero((R.words(got) != R.words(want)).any(axis=1))
    assert bad.size == 0, (tag, bad.size, bad[:6], got[bad[:6]], want[bad[:6]])


@pytest.mark.parametrize("derived", [1, 0], ids=["table", "records"])
@pytest.mark.parametrize("lib", list(LIBS))
@pytest.mark.parametrize("name,poolkey", GOLDENS)
def test_a_frames_pixel_rays_give_the_frames_hit_records(contexts, name, poolkey, lib, derived):
    """(B): the rays of every pixel of a golden frame: the reference shader's first_hit where compare_with_golden compares
    it, and the library's own frame's records everywhere"""
    g = golden_case(name, poolkey)
    c = contexts(lib)
    c.set_derived(derived)
    try:
        frame = c.render(g["pool"], g["w"], g["h"], g["cam"], g["frame"], g["mode"])
        got = c.cast_rays(R.pixel_rays(g["cam"], g["w"], g["h"]))
        info = c.cast_info()
        assert info["walk"] == (derived if c.derived_info()["walkable"] else 0), info
        assert 1 <= info["waves"] <= (got.size + 63) // 64, info
        bad = compare_with_golden({"rgba": g["rgba"], "depth": g["depth_bits"].view(np.float32),
                                   "hits": got.reshape(g["h"], g["w"])}, g)
        assert bad == {k: 0 for k in bad}, bad
        _same(got, frame["hits"].reshape(-1), name)
    finally:
        c.set_derived(1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129])
def test_wave_edges(contexts, n):
    """the first n of a fixed 129-ray set against (A); nothing is written behind ray n - 1"""
    c = contexts("asm")
    c.pool_upload(R.pool128())
    rays = np.ascontiguousarray(R.edge_rays()[:n])
    hits = np.full(n + 8, 0xA5, dtype=np.uint8).repeat(16).view(hiplib.HIT_DTYPE)     # the guard pattern
    c._chk(c._L.svo_cast_rays(c._h, rays.ctypes.data, n, hits.ctypes.data))
    _same(hits[:n], R.edge_ref()[:n], n)
    assert (hits[n:].view(np.uint8) == 0xA5).all()


def test_a_prefix_of_a_cast_is_the_cast_of_the_prefix(contexts):
    c = contexts("asm")
    c.pool_upload(R.pool128())
    a, b = c.cast_rays(R.edge_rays()), c.cast_rays(R.edge_rays()[:65])
    _same(a[:65], b)
    _same(a, R.edge_ref())


@pytest.mark.parametrize("thresh", [0, 16, 1], ids=["default", "every_stop", "nearly_all_stopped"])
def test_refill_and_drain(ctx, thresh):
    """one wave per CU and more rays than lanes: every lane refills, and the tail drains.  (The round threshold is in
    sixteenths: 16 = a round behind every trip, so at every stop; 1 = a round once nearly all lanes have stopped.)"""
    rays, ref = R.refill_set()
    ctx.pool_upload(R.pool128())
    ctx.set_tuning(1, thresh)
    got = ctx.cast_rays(rays)
    info = ctx.cast_info()
    assert info["waves"] * 64 < rays.shape[0], info
    _same(got, ref, thresh)
    assert (info["calls"], info["rays"]) == (1, rays.shape[0]), info


@pytest.mark.parametrize("derived", [1, 0], ids=["table", "records"])
@pytest.mark.parametrize("lib", list(LIBS))
@pytest.mark.parametrize("deep", [False, True], ids=["s128", "deep13"])
def test_hostile_rays(contexts, deep, lib, derived):
    """rays from outside, from faces and edges, from inside solid; axis directions, signed zeros, lengths 1e-20 and 1e20, zero
    and NaN: what (A) says, on the 128^3 scene and on a 13-level pool (the deepest stack slot)"""
    c = contexts(lib)
    c.set_derived(derived)
    try:
        c.pool_upload(R.pool_deep() if deep else R.pool128())
        rays = R.into_deep(R.HOSTILE) if deep else R.HOSTILE
        got = c.cast_rays(rays)
        want = R.hostile_ref(deep)
        assert want[R.ALL_NAN]["iter"] == 1501 and got[R.ALL_NAN]["iter"] == 1501
        _same(got, want, (deep, lib, derived))
        if deep:
            assert c.derived_info()["walkable"] and want["level"].max() == 13
            # ... and a frame's worth of ordinary rays into the corner the scene occupies, against a full-frame oracle render
            cam = np.array(CAMERAS["K1"], dtype=np.float32)
            cam[:3] = R.into_deep(cam[None, :6])[0, :3]
            _same(c.cast_rays(R.pixel_rays(cam, 64, 48)),
                  oracle.render(R.pool_deep(), 64, 48, cam, 2, 0, bounces=1)["hits"].reshape(-1), "deep frame")
        inf = c.cast_rays(R.into_deep(R.INFINITE) if deep else R.INFINITE)      # not representable by (A): they come back
        assert (inf["iter"] <= 1501).all(), inf
    finally:
        c.set_derived(1)


def test_device_variant_on_the_callers_stream(ctx):
    import torch
    g = golden_case("s128_K1_m0", "s128")
    ctx.pool_upload(g["pool"])
    rays, ref = R.refill_set()
    rays = rays[:4099]
    want = ctx.cast_rays(rays)
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_hits = [torch.full((rays.shape[0], 4), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for h in d_hits:                          # two calls back to back: the second waits its turn on the stream
            ctx.cast_rays_device(d_rays.data_ptr(), rays.shape[0], h.data_ptr())
        assert ctx.cast_info()["calls"] == 3
        stream.synchronize()
    for h in d_hits:
        assert (h.cpu().numpy().view(np.uint32) == R.words(want)).all()
    assert ctx.cast_info()["gpu_ms"] > 0.0
    ctx.set_stream(None)                          # back on the library's stream: a frame still matches its golden
    res = ctx.render(None, g["w"], g["h"], g["cam"], g["frame"], g["mode"])
    bad = compare_with_golden(res, g)
    assert bad == {k: 0 for k in bad}, bad


def test_a_cast_leaves_the_context_alone(ctx):
    g = golden_case("s128_K1_m0", "s128")
    rays = R.edge_rays()

    def state():
        return (ctx.read_color().tobytes(), ctx.read_depth().tobytes(), ctx.read_hits().tobytes(), ctx.pick_info(),
                ctx.primary_cache_info(), ctx.stats())
    ctx.render(g["pool"], g["w"], g["h"], g["cam"], g["frame"], g["mode"])
    before = state()
    _same(ctx.cast_rays(rays), R.restate(g["pool"], rays))
    assert state() == before
    bad = compare_with_golden(ctx.render(None, None, None, None, g["frame"], g["mode"]), g)
    assert bad == {k: 0 for k in bad}, bad
    # casts between a ring submission and its wait
    ctx.ring_create(2, 1, want_hits=True)
    try:
        slot = ctx.ring_submit(g["frame"], 1)
        a = ctx.cast_rays(rays)
        b = ctx.cast_rays(rays[:33])
        ctx.ring_wait(slot)
        bad = compare_with_golden(ctx.ring_read(slot, 0, want_hits=True), g)
        assert bad == {k: 0 for k in bad}, bad
        _same(a[:33], b)
    finally:
        ctx.ring_destroy()


def test_casts_follow_the_edits_of_the_pool(ctx):
    """upload, brush stroke, compaction: each cast is (A) on the pool as it is at that moment (the descriptor table and the
    pool's length follow)"""
    rays = np.concatenate([R.pixel_rays(CAMERAS["K1"], 32, 24), R.HOSTILE[:10]])
    first = scene.build_scene(64)[0]
    ctx.pool_upload(first)
    sizes = [first.size]
    for step in ("upload", "brush", "compact"):
        if step == "brush":
            sizes.append(ctx.brush_sphere((30, 30, 30), 10, 2, 64, 6)[3])
        if step == "compact":
            sizes.append(ctx.pool_compact()[1])
        pool = ctx.pool_download(sizes[-1])
        got = ctx.cast_rays(rays)
        _same(got, R.restate(pool, rays), step)
        assert ctx.cast_info()["walk"] == 1 and (got["pointer"] != 0).any()
    assert sizes[0] < sizes[2] < sizes[1], sizes                 # the stroke appends, compaction drops what it orphaned


def test_errors(ctx):
    L, h = ctx._L, ctx._h
    rays = np.ascontiguousarray(R.edge_rays()[:4])
    hits = np.zeros(4, dtype=hiplib.HIT_DTYPE)
    assert L.svo_cast_rays(h, rays.ctypes.data, 4, hits.ctypes.data) == -2             # SVO_E_NOPOOL
    assert L.svo_cast_rays_device(h, rays.ctypes.data, 4, hits.ctypes.data) == -2
    ctx.pool_upload(R.pool128())
    for f in (L.svo_cast_rays, L.svo_cast_rays_device):
        assert f(h, None, 4, hits.ctypes.data) == -1 and f(h, rays.ctypes.data, 4, None) == -1      # SVO_E_INVALID
        assert f(h, rays.ctypes.data, (1 << 26) + 1, hits.ctypes.data) == -5           # SVO_E_TOOLARGE, before any allocation
        assert f(h, None, 0, None) == 0                                                # nothing to do
    info = ctx.cast_info()
    assert (info["calls"], info["rays"], info["waves"], info["gpu_ms"]) == (0, 0, 0, 0.0), info      # n = 0 is not counted
    assert L.svo_cast_info(h, None, None, None, None, None) == 0
    ctx.cast_rays(rays)
    assert ctx.cast_info()["calls"] == 1 and ctx.cast_info()["rays"] == 4 and ctx.cast_info()["waves"] == 1
