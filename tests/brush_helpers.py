"""Helpers of the GPU brush tests (svo_brush_sphere / svo_brush_box): the checker is the restatement of Octree.useSDFBrush
(oracle/octree_restatement.cpp) run on a hostlib.Octree that adopted the same pool."""
import numpy as np

from svo_raytracer_amd import hostlib
from oracle import octree as restated

BOX_EDIT = ("box", (34, 30, 30), (3, 5, 4), 3)      # the box stroke of tests/test_sdf_edit.py


def edits64():
    """the three sphere EDITS of tests/test_sdf_edit.py and its box stroke, as (kind, origin, radius | (w, h, d), value)"""
    from test_sdf_edit import EDITS
    return list(EDITS) + [BOX_EDIT]


class Checker:
    """the restatement's side of a stroke sequence"""

    def __init__(self, pool, kb=1 << 16):
        self.o = hostlib.Octree(kb)
        self.o.adopt(pool)

    def stroke(self, kind, origin, size, value, world_size, max_lod):
        if kind == "sphere":
            cb = restated.useSDFBrushSphere(self.o, origin, size, value, worldSize=world_size, maxLOD=max_lod)
        else:
            cb = restated.useSDFBrushBox(self.o, origin, size[0], size[1], size[2], value, worldSize=world_size, maxLOD=max_lod)
        return cb, self.o.getByteBuffer()


def gpu_stroke(ctx, kind, origin, size, value, world_size, max_lod):
    if kind == "sphere":
        return ctx.brush_sphere(origin, size, value, world_size, max_lod)
    return ctx.brush_box(origin, size[0], size[1], size[2], value, world_size, max_lod)


def assert_stroke_equal(ctx, cb, want_cb, want_pool, before=None, tag=None):
    """cb, the pool's length and every byte equal the restatement's; with `before`, every byte that changed lies in
    [lo, hi) or [start1, end1)"""
    assert cb == want_cb, (tag, cb, want_cb)
    assert cb[3] == want_pool.size, (tag, cb, want_pool.size)
    got = ctx.pool_download(want_pool.size)             # (cb[3] is the pool's length)
    bad = np.nonzero(got != want_pool)[0]
    assert bad.size == 0, (tag, bad.size, bad[:8], got[bad[:8]], want_pool[bad[:8]])
    if before is not None:
        info = ctx.brush_info()
        n = before.size
        diff = np.nonzero(before != got[:n])[0]
        inside = (diff >= info["lo"]) & (diff < info["hi"])
        assert inside.all(), (tag, info, diff[~inside][:8])
        assert cb[2] == n
    return got


def stroke_args(n=128, strokes=14, seed=11):
    """the arguments of derived_edits.brush_strokes' strokes (the generator yields only what they left): the same draws
    from the same generator, as (kind, origin, radius | (w, h, d), value)"""
    rng = np.random.default_rng(seed)
    out = []
    for stroke in range(strokes):
        org = tuple(int(v) for v in rng.integers(n // 4, 3 * n // 4, 3))
        r = int(rng.integers(3, 14))
        val = int(rng.choice([0, 0, 1, 2, 3]))
        if stroke % 5 == 4:
            out.append(("box", org, (r, max(2, r // 2), r), val))
        else:
            out.append(("sphere", org, r, val))
    return out
