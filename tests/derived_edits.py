"""Pools and edit sequences for the tests of the interior-descriptor table: the edit generators the rendering tests
(test_sdf_edit.py, test_gpu_derived.py) and the whole-table test (test_derived_table.py) share, hand-made pools at the
limits of what the table can state, and small edits aimed at the corners of the refresh."""
import numpy as np

import derived_ref as R


# ------------------------------------------------------------------------------------------- shared edit sequences

def brush_strokes(pool, n=128, lod=7, strokes=14, seed=11):
    """SDF brush strokes on the n^3 terrain `pool` (spheres, every fifth a box; fills, carves, strokes over strokes):
    yields (stroke, host pool after it, the stroke's two byte ranges (s0, e0, s1, e1), whether the root record changed)"""
    from svo_raytracer_amd import hostlib
    from oracle import octree as restated
    o = hostlib.Octree(1 << 16)
    o.adopt(pool)
    rng = np.random.default_rng(seed)
    prev_host = pool
    for stroke in range(strokes):
        org = tuple(int(v) for v in rng.integers(n // 4, 3 * n // 4, 3))
        r = int(rng.integers(3, 14))
        val = int(rng.choice([0, 0, 1, 2, 3]))
        if stroke % 5 == 4:
            cb = restated.useSDFBrushBox(o, org, r, max(2, r // 2), r, val, worldSize=n, maxLOD=lod)
        else:
            cb = restated.useSDFBrushSphere(o, org, r, val, worldSize=n, maxLOD=lod)
        host = o.getByteBuffer()
        # (a stroke that rewrites the root record -- its mask changes when one of the eight top-level children is
        # re-tagged, common in a 128^3 world, out of reach of a brush at 8192^3 -- is the one case left to a rebuild)
        root_changed = bool((host[1:7] != prev_host[1:7]).any())
        prev_host = host
        yield stroke, host, cb, root_changed


def reachable_records(pool):
    """(offset, tag) of every record a proper walk from the root reaches"""
    out, stack = [], [0]
    while stack:
        p = stack.pop()
        cp = int.from_bytes(bytes(pool[p + 1:p + 5]), "big", signed=True)
        if cp == 0:
            continue
        mask = (int(pool[p + 5]) << 8) | int(pool[p + 6])
        c = p + cp
        for k in range(8):
            tag = (mask >> (2 * k)) & 3
            out.append((c, tag))
            if tag == 0:
                stack.append(c)
            c += {0: 7, 1: 3, 2: 7, 3: 1}[tag]
    return out


def record_edits(host, edits=40, seed=23):
    """Small edits of a kind no brush makes, applied to `host` in place: value bytes zeroed and set, child pointers cut and
    re-pointed at other blocks (shared and cyclic subtrees), tag masks rewritten, records copied over one another.  Yields
    (edit number, kind, lo, hi) after each; an edit that touches the root record is made but not yielded."""
    recs = reachable_records(host)
    inner = [o for o, t in recs if t == 0 and int.from_bytes(bytes(host[o + 1:o + 5]), "big") != 0]
    rng = np.random.default_rng(seed)
    for edit in range(edits):
        kind = edit % 5
        o, tag = recs[int(rng.integers(len(recs)))]
        if kind == 0:      # a value byte flips between empty and solid
            lo, hi = o, o + 1
            host[o] = 0 if host[o] else 3
        elif kind == 1:    # an interior node loses its children
            o = inner[int(rng.integers(len(inner)))]
            lo, hi = o + 1, o + 5
            host[lo:hi] = 0
        elif kind == 2:    # ... or gets another node's: a shared (possibly cyclic) subtree
            o, src = inner[int(rng.integers(len(inner)))], inner[int(rng.integers(len(inner)))]
            tgt = src + int.from_bytes(bytes(host[src + 1:src + 5]), "big", signed=True)
            lo, hi = o + 1, o + 7
            host[o + 1:o + 5] = np.frombuffer(int(tgt - o).to_bytes(4, "big", signed=True), np.uint8)
            host[o + 5:o + 7] = host[src + 5:src + 7]
        elif kind == 3:    # a tag mask is rewritten: the children's records are re-read at other sizes
            o = inner[int(rng.integers(len(inner)))]
            lo, hi = o + 5, o + 7
            host[lo:hi] = rng.integers(0, 256, 2, dtype=np.uint8)
        else:              # seven bytes of one record land on another
            src = recs[int(rng.integers(len(recs)))][0]
            lo, hi = o, min(o + 7, host.size)
            host[lo:hi] = host[src:src + (hi - lo)].copy()
        if lo < 7:
            continue       # (the root record: a rebuild by design, covered elsewhere)
        yield edit, kind, lo, hi


def replace_ranges(a, b):
    """the tree `a` replaced by the tree `b` in three ranges (and what is left of a longer `a` zeroed): yields (the pool as
    it stands after the range, lo, hi)"""
    third = b.size // 3
    ranges = [(0, third), (third, 2 * third), (2 * third, b.size)]
    if a.size > b.size:
        ranges.append((b.size, a.size))
    big = np.zeros(max(a.size, b.size), np.uint8)
    big[:b.size] = b
    cur = a.copy()
    for lo, hi in ranges:
        if hi > cur.size:
            cur = np.concatenate([cur, np.zeros(hi - cur.size, np.uint8)])
        cur[lo:hi] = big[lo:hi]
        yield cur.copy(), lo, hi


# ------------------------------------------------------------------------------------------- hand-made pools

def _rec(value, cp=0, mask=0):
    return [value & 0xff] + list(int(cp & 0xffffffff).to_bytes(4, "big")) + [(mask >> 8) & 0xff, mask & 0xff]


def _chain_block(level):
    """a child block of one interior record (slot level % 8) and seven one- and three-byte records, some of them empty:
    (bytes, offset of the interior record inside them, tag mask)"""
    slot = level % 8
    out, mask, at = [], 0, 0
    for c in range(8):
        if c == slot:
            at = len(out)
            out += _rec(1 + level % 3)
        elif (c + level) % 2:
            mask |= 3 << (2 * c)
            out += [0 if (c + level) % 3 == 0 else 2]
        else:
            mask |= 1 << (2 * c)
            out += [0 if c % 4 == 0 else 1, (455 + c) & 0xff, (455 + c) >> 8]
    return out, at, mask


def chain_pool(depth):
    """`depth` child blocks one below the other: parent states at depth 0 .. depth - 1; the interior record of the last block
    has no child block"""
    out = _rec(1)
    rec = 0
    for level in range(depth):
        block, at, mask = _chain_block(level)
        out[rec + 1:rec + 7] = _rec(0, len(out) - rec, mask)[1:]
        rec = len(out) + at
        out += block
    return np.array(out, np.uint8)


def chain_append(host):
    """one more block under the chain's last interior record: (new host, (lo of the record's pointer and mask, lo of the new
    block), (hi, hi)) -- two ranges, like a brush stroke's"""
    pool = bytes(host)
    state, rec, level = R.root_state(pool), 0, 0
    while True:
        kids = R.children(pool, *state)[2]
        if not kids:
            break
        (c, state, rec), = kids
        level += 1
    # `state` is the deepest block; its interior record (cp 0) is the child with tag 0
    B, M = state
    slot = [c for c in range(8) if (M >> (2 * c)) & 3 == 0][0]
    rec = B + R.child_offset(M, slot)
    block, at, mask = _chain_block(level + 1)
    out = list(pool)
    out[rec + 1:rec + 7] = _rec(0, len(out) - rec, mask)[1:]
    out += block
    return np.array(out, np.uint8), (rec + 1, len(pool)), (rec + 7, len(out))


def _loop_back():
    """a block whose one interior record points back at the block it lies in (cp = -1, the offsets wrap): a chain without end"""
    return np.array(_rec(1, 7, 0xfff3) + [2] + _rec(1, -1, 0xfff3) + [1, 0, 3, 1, 0, 2], np.uint8)


def _loop_wide():
    """a block of eight interior records, seven of which point back at it: the unrolling grows sevenfold per level"""
    out = _rec(1, 7, 0)
    for c in range(8):
        out += _rec(1 + c % 3, -7 * c, 0)
    return np.array(out, np.uint8)


def _short40():
    """40 bytes: a root with eight one-byte children, then bytes that are no records of the tree but that the pair (0, 0)
    reads as interior nodes at 14, 21, 28, 35 -- pointing past the end, backwards into the root's children, and (the last
    one) lying across the end of the pool itself"""
    out = _rec(1, 7, 0xffff) + [1, 0, 2, 3, 0, 1, 127, 0]
    out = out[:14] + _rec(2, 30, 0x1234) + _rec(1, 5, 0) + _rec(3, -16, 0x0003) + [1, 0, 0, 0, 2]
    assert len(out) == 40
    return np.array(out, np.uint8)


def _root_cp0():
    """the 64^3 terrain with the root's child pointer cut: the root pair is (0, mask), its first child the root record itself"""
    import svo_raytracer_amd.scene as scene
    p = scene.build_scene(64)[0].copy()
    p[1:5] = 0
    return p


HAND_MADE = {"chain12": lambda: chain_pool(12), "chain13": lambda: chain_pool(13), "chain14": lambda: chain_pool(14),
             "loop_back": _loop_back, "loop_wide": _loop_wide, "short40": _short40, "root_cp0": _root_cp0}


def family_pool(name):
    """one small pool of the "caves" / "dust" scene families"""
    import svo_raytracer_amd.scene as scene
    return scene.build(name, 64)[0]


# ------------------------------------------------------------------------------------------- aimed edits

def interior_nodes(pool):
    """every interior record with a child block that a walk from the root reaches (a proper tree is assumed):
    (record offset, depth of its state, B, M, world position of its low corner, edge) -- the root's cube is [1, 2]^3"""
    pool = bytes(pool)
    out, stack = [], [(0, R.root_state(pool), 0, (1.0, 1.0, 1.0), 1.0)]
    while stack:
        rec, (B, M), depth, pos, edge = stack.pop()
        out.append((rec, depth, B, M, pos, edge))
        h = edge / 2
        for c, st, p in R.children(pool, B, M)[2]:
            stack.append((p, st, depth + 1, (pos[0] + h * (c & 1), pos[1] + h * ((c >> 1) & 1), pos[2] + h * ((c >> 2) & 1)), h))
    return out


def block_size(M):
    return R.child_offset(M, 8)


def states_over(pool, lo, hi):
    """distinct parent states of the unrolled pool whose child block overlaps [lo, hi)"""
    u = R.unroll(pool)
    seen = {(s[0], s[1]) for lvl in u.levels + u.phantom_levels for s in lvl} | {(0, 0)}
    return sum(1 for B, M in seen if B < hi and B + block_size(M) > lo)


def _toggle(host, at):
    host[at] = 0 if host[at] else 3


def block_edge_edits(host):
    """Applied to `host` in place, yielding (what, lo, hi) after each: one- and two-byte updates on the first and the last
    byte of a child block, just before and just past it -- on a block deep in the tree whose first and last byte are value
    bytes, so that each edit changes what the block's state says -- then the same on a block that two states share."""
    nodes = interior_nodes(host)

    def usable(n):
        rec, depth, B, M, pos, edge = n
        last = (M >> 14) & 3
        return depth >= 3 and last == 3 and B - 2 > 64 and B + block_size(M) + 2 < host.size

    cands = [n for n in nodes if usable(n)]
    rec, depth, B, M, pos, edge = cands[len(cands) // 2]
    E = B + block_size(M)

    def edges(tag):
        for what, lo, hi in (("first byte", B, B + 1), ("last byte", E - 1, E), ("one before", B - 1, B), ("one past", E, E + 1),
                             ("two over the start", B - 1, B + 1), ("two over the end", E - 1, E + 1),
                             ("two inside at the start", B, B + 2), ("two inside at the end", E - 2, E)):
            for at in range(lo, hi):
                _toggle(host, at)
            yield tag + what, lo, hi

    yield from edges("")
    # a second record of the same depth (so the tree keeps its depth) is pointed at the block: two states (B, M), or one that
    # two parents share -- either way both must follow an edit of the block
    other = [n for n in nodes if n[1] == depth and n[0] != rec and n[2] != B][0]
    o = other[0]
    host[o + 1:o + 5] = np.frombuffer(int(B - o).to_bytes(4, "big", signed=True), np.uint8)
    host[o + 5:o + 7] = (M >> 8, M & 0xff)
    yield "re-point", o + 1, o + 7
    yield from edges("shared: ")


def record_behind_camera(host, cam_name):
    """the offset of a non-empty record at least four levels down whose cell lies well behind the camera's image plane"""
    from svo_raytracer_amd.cameras import CAMERAS
    cam = np.asarray(CAMERAS[cam_name], np.float64)
    fwd = cam[3:6] + cam[6:9] + cam[9:12] + cam[12:15]
    fwd /= np.linalg.norm(fwd)
    pool = bytes(host)
    best = None
    for rec, depth, B, M, pos, edge in interior_nodes(host):
        centre = np.array(pos) + edge / 2
        if depth < 3 or np.dot(centre - cam[:3], fwd) > -0.1 - edge:
            continue
        m_ne = R.children(pool, B, M)[0]
        if m_ne and (best is None or depth > best[0]):
            c = [k for k in range(8) if (m_ne >> k) & 1][0]
            best = (depth, B + R.child_offset(M, c))
    assert best is not None
    return best[1]


def phantom_block_edits(host):
    """edits inside bytes 7..55 -- the child block of the pair (0, 0), in a builder's pool also the root's -- that leave the
    root record alone: a value byte of one of the root's children cleared and set, and a pointer byte of a record the root
    takes for a leaf set together with its value byte (the root gets a solid leaf; the pair (0, 0), which reads every record
    there as an interior node, gets a child to descend into)"""
    host = host.copy()
    for _ in range(2):
        _toggle(host, 14)
        yield "value byte at 14", host.copy(), 14, 15
    B, M = R.root_state(bytes(host))
    leafs = [c for c in range(7) if (M >> (2 * c)) & 3 == 2]
    assert B == 7 and leafs and block_size(M) == 56          # (a builder's terrain: eight 7-byte records behind the root's)
    at = 7 + 7 * leafs[0]
    old = host[at:at + 3].copy()
    host[at:at + 3] = (3, 0, 0x40)
    yield "a leaf of the root's made solid, with a pointer only (0, 0) follows", host.copy(), at, at + 3
    host[at:at + 3] = old
    yield "and back", host.copy(), at, at + 3


def appending_edits(host):
    """a copy of one child block appended past the pool's end (the pointers of its records adjusted to mean the same blocks),
    then its parent pointed at the copy: the update that grows the pool, then the one that makes it count"""
    nodes = [n for n in interior_nodes(host) if n[1] == 3]
    rec, depth, B, M, pos, edge = nodes[len(nodes) // 3]
    size, end = block_size(M), host.size
    block = host[B:B + size].copy()
    for c in range(8):
        if (M >> (2 * c)) & 3 == 0:
            at = R.child_offset(M, c)
            cp = int.from_bytes(bytes(block[at + 1:at + 5]), "big", signed=True)
            if cp:
                block[at + 1:at + 5] = np.frombuffer(int(cp - (end - B)).to_bytes(4, "big", signed=True), np.uint8)
    host = np.concatenate([host, block])
    yield "block appended", host.copy(), end, end + size
    host[rec + 1:rec + 5] = np.frombuffer(int(end - rec).to_bytes(4, "big", signed=True), np.uint8)
    yield "parent pointed at it", host.copy(), rec + 1, rec + 5
