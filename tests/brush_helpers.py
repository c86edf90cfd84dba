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


def restatement_safe(world_size, max_lod, depth):
    """THE RULE of every generator below: the restatement (like the Java) never sees a (world_size, max_lod) under which a
    node of size > 1 can be a 3-byte or 1-byte record.  Short records sit at level min(max_lod, depth) -- `depth` the level
    of the tree's own short records, max_lod the level at which a stroke creates them -- and the size halves (rounding down)
    once per level.  Where this does not hold the reference subdivides a short record, writes a child pointer over its
    neighbour and corrupts its own pool (the next stroke may crash the process): such a stroke goes to the GPU alone, which
    must refuse it (test_gpu_brush_edges.py::test_max_lod_below_the_depth_is_refused)."""
    return (int(world_size) >> min(int(max_lod), int(depth))) <= 1


class Checker:
    """the restatement's side of a stroke sequence; with `depth` (the level of the tree's short records) every stroke is
    held to restatement_safe"""

    def __init__(self, pool, kb=1 << 16, depth=None):
        self.o = hostlib.Octree(kb)
        self.o.adopt(pool)
        self.depth = depth

    def stroke(self, kind, origin, size, value, world_size, max_lod):
        assert self.depth is None or restatement_safe(world_size, max_lod, self.depth), (world_size, max_lod, self.depth)
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


# ------------------------------------------------------------------------------------------------------------------------
# The edges (test_gpu_brush_edges.py on the GPU; test_brush_edges_cases.py shows on the CPU that they reach what they claim)

FAMILIES = ("terrain", "caves", "dust")
FUZZ_SEEDS = {"terrain": 1, "caves": 2, "dust": 3}


def family_pool64(family):
    """the 64^3 pool of a scene family: world_size 64, max_lod 6 = its depth"""
    import svo_raytracer_amd.scene as scene
    return scene.build(family, 64)[0]


# one sequence per pool, in this order: later strokes land on records that earlier ones subdivided, filled or marked 127
EDGE_STROKES = [
    ("sphere", (32, 32, 32), 120, 2),            # the root filled: write_kernel's i == 0 branch, 8 children -> 127
    ("sphere", (32, 32, 32), 120, 0),            # the root filled again over dirty children
    ("sphere", (0, 0, 0), 20, 3),                # bounding box with negative mn, clipped at three faces
    ("sphere", (63, 63, 63), 9, 0),              # the far corner (on dust: nothing to do)
    ("sphere", (-3, 30, 70), 8, 1),              # origin outside the world on two axes
    ("sphere", (20, 20, 20), 0, 2),              # radius 0: only dist == 0 at one voxel
    ("sphere", (20, 20, 20), 1, 2),              # even origin: a size-2 node whose corner is the origin (normal of length 0)
    ("sphere", (21, 21, 21), 1, 0),              # odd origin, carve
    ("box", (32, 32, 32), (0, 0, 0), 2),         # zero extents
    ("box", (32, 32, 32), (200, 1, 200), 0),     # a slab through the whole world
    ("sphere", (30, 30, 30), 10, 127),           # the brush value equals DELETE_VALUE
    ("sphere", (30, 30, 30), 12, 255),           # top byte value, over the previous stroke
    ("sphere", (30, 30, 30), 4, 255),            # inside it: subdivideNode's value == currentValue, the pool stays untouched
]
EDGE_ROOT_FILLS, EDGE_GROWS, EDGE_GROWTH = (0, 1), 2, 12152     # what the restatement reports on all three pools
EDGE_DUST_IDLE = 3                               # on dust the restatement returns cb = [len, 0, len, len] here


def diff_facts(before, now):
    """what a stroke did, from the two pools alone"""
    n = before.size
    changed = np.nonzero(before != now[:n])[0]
    return {"root": bool((changed < 7).any()), "more127": int((now == 127).sum()) - int((before == 127).sum()),
            "appended": int(now.size - n), "untouched": now.size == n and changed.size == 0}

# 256^3 terrain, world_size 256, max_lod 8: the root (16 row chunks) and the level-1 nodes (4) are marched by several waves;
# the second stroke's work list outgrows 2^18 items and is planned again; the third reuses the enlarged list
WAVE_STROKES = [("sphere", (128, 100, 128), 110, 0), ("sphere", (128, 100, 128), 100, 2), ("sphere", (60, 90, 70), 5, 3)]
FIRST_CAP = 1 << 18                              # brush::kFirstCap

# (pool edge, world_size, max_lod, strokes): max_lod and world_size away from the tree's depth, all restatement_safe
LOD_CASES = {
    "lod7_on_64": (64, 64, 7, [("sphere", (22, 25, 41), 7, 2), ("sphere", (22, 25, 41), 7, 0)]),
    "world132_on_128": (128, 132, 7, [("sphere", (40, 50, 60), 9, 2), ("box", (70, 44, 66), (12, 6, 10), 0),
                                      ("sphere", (129, 40, 131), 7, 3)]),
}
REFUSED = (64, 4, ("sphere", (30, 30, 30), 9, 2))   # world_size, max_lod < depth: NOT restatement_safe, never given to it

TWO_VOXEL_STROKE = ("sphere", (1, 1, 1), 5, 4)      # world_size 2, max_lod 1: the root is filled


def two_voxel_pool(short_first):
    """a hand-made two-voxel world: the root [1, child pointer 7, mask] and its eight children, all 7-byte tag-2 leaves, or
    (short_first) child 0 a 3-byte tag-1 leaf: 59 bytes, on which the root fill's re-tag of child 0 moves the other seven"""
    mask = 0xaaaa if not short_first else 0xaaa9
    out = [1, 0, 0, 0, 7, mask >> 8, mask & 255]
    for c in range(8):
        out += [10 + c, 43, 2] if (short_first and c == 0) else [10 + c, 0, 0, 0, 0, 0, 0]
    return np.array(out, np.uint8)


def fuzz_strokes(n, count, seed):
    """`count` strokes on a world of edge n, every third one a box, as (kind, origin, radius | (w, h, d), value): origins up
    to n/8 outside the world, radii and extents from nothing to more than the world, DELETE_VALUE and 255 among the values"""
    rng = np.random.default_rng(seed)
    radii = [0, 1, 2, 3, 5, 8, 13, n // 4, n // 2, 2 * n]
    extents = [0, 1, 2, n // 8, n, 4 * n]
    out = []
    for stroke in range(count):
        org = tuple(int(v) for v in rng.integers(-(n // 8), n + n // 8, 3))
        val = int(rng.choice([0, 0, 1, 2, 3, 127, 255]))
        if stroke % 3 == 2:
            out.append(("box", org, tuple(int(v) for v in rng.choice(extents, 3)), val))
        else:
            out.append(("sphere", org, int(rng.choice(radii)), val))
    return out
