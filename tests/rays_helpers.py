"""What the ray-query tests (svo_cast_rays) share: the two independent checkers of a cast, the fixed ray sets, and their
references, each computed once.

(A) the restatement: oracle.render(pool, 1, 1, [o, d, d, d, d], render_mode=0, bounces=1)["hits"][0, 0] is the cast of the
    ray (o, d) -- the four equal corners mix to d exactly, and main normalises it.
(B) the frame: a pixel's primary direction before normalising, a + p_x (b - a) with a = l1 + p_y (l2 - l1),
    b = r1 + p_y (r2 - r1), p = (pixel + 0.5) / size, in float32 with no fused operation, is bit for bit what the shader
    forms: cast_rays of a frame's pixel rays equals that frame's hit records."""
import functools

import numpy as np

import svo_raytracer_amd.scene as scene
from oracle import oracle
from svo_raytracer_amd.cameras import CAMERAS
from svo_raytracer_amd.hiplib import HIT_DTYPE

NAN = float("nan")
INF = float("inf")


def words(hits):
    """the 16-byte records as (n, 4) uint32, for byte comparisons"""
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4)


def pixel_rays(cam, w, h):
    """(B): the w * h primary rays of a frame, row by row, un-normalised as the shader forms them"""
    cam = np.asarray(cam, dtype=np.float32).reshape(5, 3)
    o, l1, l2, r1, r2 = cam
    f = np.float32
    px = ((np.arange(w, dtype=np.float32) + f(0.5)) / f(w))[None, :, None]
    py = ((np.arange(h, dtype=np.float32) + f(0.5)) / f(h))[:, None, None]
    a = l1[None, None, :] + py * (l2 - l1)[None, None, :]
    b = r1[None, None, :] + py * (r2 - r1)[None, None, :]
    d = (a + px * (b - a)).astype(np.float32)
    rays = np.empty((h, w, 6), dtype=np.float32)
    rays[..., :3] = o
    rays[..., 3:] = d
    return rays.reshape(-1, 6)


def restate(pool, rays):
    """(A) for every ray: n HIT_DTYPE records"""
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 6)
    out = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
    for k, r in enumerate(rays):
        cam = np.concatenate([r[:3], r[3:], r[3:], r[3:], r[3:]]).astype(np.float32)
        out[k] = oracle.render(pool, 1, 1, cam, 2, 0, bounces=1)["hits"][0, 0]
    return out


# Origins outside the cube pointing away, outside grazing a face and an edge, on a face, inside empty space, inside solid
# (128^3 terrain: the ground lies below y = 1.5, the sky above); directions along the six axes (the EPSILON clamp), with
# components of +-0.0, of un-normalised lengths 1e-20 and 1e20, all zero, and the all-NaN ray.  Finite or all-NaN only.
_AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
HOSTILE = np.array(
    [(2.5, 1.5, 1.5, 1.0, 0.2, 0.1),            # outside, pointing away
     (0.5, 2.0, 1.5, 1.0, 0.0, 0.0),            # outside, grazing the face y = 2
     (0.5, 2.0, 2.0, 1.0, 0.0, 0.0),            # outside, grazing the edge y = z = 2
     (0.5, 1.0, 1.0, 1.0, 0.0, 0.0),            # ... and the edge y = z = 1
     (1.0, 1.5, 1.5, 1.0, 0.1, 0.05),           # on the face x = 1, inwards
     (1.5, 2.0, 1.5, 0.1, -1.0, 0.2),           # on the face y = 2, inwards
     (1.5, 1.9, 1.5, 0.1, -1.0, 0.2),           # inside empty space, down to the ground
     (1.5, 1.9, 1.5, 0.1, 1.0, 0.2),            # inside empty space, up and out
     (1.5, 1.05, 1.5, 0.0, 1.0, 0.0),           # inside solid
     (1.3, 1.02, 1.7, 0.3, 0.9, -0.2)] +        # inside solid
    [(1.5, 1.9, 1.5) + a for a in _AXES] +      # the six axis directions from the sky
    [(1.25, 1.01, 1.75) + a for a in _AXES] +   # ... and from inside the ground
    [(1.5, 1.9, 1.5, 0.0, -1.0, -0.0),          # components of +-0.0
     (1.5, 1.9, 1.5, -0.0, -1.0, 0.0),
     (1.2, 1.8, 1.2, 0.5, -0.0, 0.5),
     (1.2, 1.8, 1.2, -0.0, -0.0, -1.0),
     (1.5, 1.9, 1.5, 0.3e-20, -0.8e-20, 0.2e-20),   # length 1e-20
     (1.5, 1.9, 1.5, 0.3e20, -0.8e20, 0.2e20),      # length 1e20
     (0.2, 2.7, 0.1, 0.5e20, -0.6e20, 0.6e20),
     (1.5, 1.9, 1.5, 0.0, 0.0, 0.0),            # an all-zero direction
     (1.5, 1.9, 1.5, -0.0, -0.0, -0.0),
     (NAN, NAN, NAN, NAN, NAN, NAN),            # the all-NaN ray
     (1.5, 1.9, 1.5, NAN, NAN, NAN),
     (NAN, NAN, NAN, 0.1, -1.0, 0.2)], dtype=np.float32)
ALL_NAN = int(np.flatnonzero(np.isnan(HOSTILE).all(axis=1))[0])
# a single infinite component is not representable by (A) (the mix turns it into NaN): such rays must only come back
INFINITE = np.array([(1.5, 1.9, 1.5, INF, -1.0, 0.2), (1.5, 1.9, 1.5, 0.1, -INF, 0.2), (INF, 1.9, 1.5, 0.1, -1.0, 0.2),
                     (1.5, -INF, 1.5, 0.0, 1.0, 0.0)], dtype=np.float32)
DEEP_K = 7   # levels chained above the 64^3 scene: 13 in all, the deepest the walk's stack holds


@functools.lru_cache(maxsize=None)
def pool128():
    p = scene.build_scene(128)[0]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def pool_deep():
    p = scene.embed_deep(scene.build_scene(64)[0], DEEP_K)
    p.setflags(write=False)
    return p


def into_deep(rays):
    """the rays with their origins taken into the corner [1, 1 + 2^-DEEP_K]^3 the deep pool's scene occupies"""
    r = np.array(rays, dtype=np.float32)
    r[:, :3] = np.float32(1.0) + (r[:, :3] - np.float32(1.0)) * np.float32(2.0 ** -DEEP_K)
    return r


@functools.lru_cache(maxsize=None)
def edge_rays():
    """the fixed 129-ray set of the wave-edge test: every 95th pixel ray of a 128 x 96 frame of K1 on the 128^3 scene (ground
    and sky), with a few hostile rays among them"""
    r = pixel_rays(CAMERAS["K1"], 128, 96)[::95][:129].copy()
    r[7::16] = HOSTILE[:8]
    assert r.shape == (129, 6)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def edge_ref():
    out = restate(pool128(), edge_rays())
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hostile_ref(deep):
    out = restate(pool_deep(), into_deep(HOSTILE)) if deep else restate(pool128(), HOSTILE)
    out.setflags(write=False)
    return out


REFILL_W, REFILL_H = 256, 192


@functools.lru_cache(maxsize=None)
def refill_set():
    """the rays of a 256 x 192 frame plus 17 hostile ones, shuffled by a fixed permutation, and their records: one full-frame
    oracle render plus (A) for the 17"""
    cam = CAMERAS["K1"]
    rays = np.concatenate([pixel_rays(cam, REFILL_W, REFILL_H), HOSTILE[:17]])
    ref = np.concatenate([oracle.render(pool128(), REFILL_W, REFILL_H, cam, 2, 0, bounces=1)["hits"].reshape(-1),
                          hostile_ref(False)[:17]])
    perm = np.random.default_rng(20240607).permutation(rays.shape[0])
    rays, ref = np.ascontiguousarray(rays[perm]), np.ascontiguousarray(ref[perm])
    rays.setflags(write=False)
    ref.setflags(write=False)
    return rays, ref
