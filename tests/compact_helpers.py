"""Inputs shared by tests/test_compact_cases.py (CPU) and tests/test_gpu_compact.py: edited pools through the restatement of
Octree.useSDFBrush, computed once per session and never written to, and a few hand-made pools."""
import functools

import numpy as np

import brush_helpers as B
import compact_ref

HIT_FIELDS = ("value", "raw_normal", "level", "iter", "t")     # every field of a hit record but `pointer`


@functools.lru_cache(maxsize=None)
def edited64(family, first=0):
    """the 64^3 pool of a family after EDGE_STROKES[first:] through the restatement, and what compact_ref makes of it"""
    chk = B.Checker(B.family_pool64(family), depth=6)
    for kind, org, size, val in B.EDGE_STROKES[first:]:
        now = chk.stroke(kind, org, size, val, 64, 6)[1]
    now = now.copy()
    want = compact_ref.compact(now)
    now.setflags(write=False)
    want.setflags(write=False)
    return now, want


def same_frame_but_pointers(a, b, tag=None):
    """rgba, depth bits and every hit field but `pointer` equal; `pointer` non-zero on the same pixels.  Returns the hit mask."""
    assert (a["rgba"] == b["rgba"]).all(), tag
    assert (a["depth"].view(np.uint32) == b["depth"].view(np.uint32)).all(), tag
    for key in HIT_FIELDS:
        x, y = a["hits"][key], b["hits"][key]
        if key == "t":
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert (x == y).all(), (tag, key)
    hit = a["hits"]["pointer"] != 0
    assert ((b["hits"]["pointer"] != 0) == hit).all(), tag
    return hit


def leaf_block(first_value):
    """eight 7-byte tag-2 leaves"""
    out = []
    for c in range(8):
        out += [first_value + c, 0, 0, 0, 0, 0, 0]
    return out


def rec(value, rel, mask):
    return [value] + list(int(rel).to_bytes(4, "big", signed=True)) + [mask >> 8, mask & 255]


def fan_pool(blocks):
    """a chain of `blocks` blocks behind the root: the eight records of each are interior and all point at the next block, the
    last block holds leaves.  56 blocks' worth of bytes in the pool; as a tree, level k has 8^k nodes."""
    out = rec(1, 7, 0 if blocks > 1 else 0xaaaa)
    for b in range(1, blocks + 1):
        at = 7 + 56 * (b - 1)
        if b == blocks:
            out += leaf_block(50)
        else:
            for c in range(8):
                out += rec(1, at + 56 - (at + 7 * c), 0 if b + 1 < blocks else 0xaaaa)
    return np.array(out, np.uint8)


def cyclic_pool():
    """the root's child 0 is interior and its pointer leads back to the root's own block, which holds it: 63 bytes"""
    mask = 0xaaa8                                              # child 0 tag 0, the others tag-2 leaves
    block = leaf_block(20)
    block[0:7] = rec(1, 0, mask)                               # at offset 7, its block at 7 + 0
    return np.array(rec(1, 7, mask) + block, np.uint8)


def shared_pool():
    """the root's children 0 and 3 are interior and point at ONE block of leaves (119 bytes); a tree needs it twice (175)"""
    mask = 0xaaaa & ~(3 << 0) & ~(3 << 6)
    block = leaf_block(30)
    block[0:7] = rec(2, 56, 0xaaaa)                            # child 0 at 7: the shared block at 63
    block[21:28] = rec(3, 63 - 28, 0xaaaa)                     # child 3 at 28
    return np.array(rec(1, 7, mask) + block + leaf_block(40), np.uint8)
