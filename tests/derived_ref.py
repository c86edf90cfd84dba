"""A plain restatement of the interior-descriptor table's contract (the header comment of
svo-raytracer_amd/csrc/svo_derive.hip.h), for checking the table the library builds and refreshes.  Python integers
and the pool's bytes only: nothing is imported from the library.

The pool is read the way the shader's getByte reads it: every byte at or past the pool's length is 0.  Offsets are
32-bit and wrap.  A parent state is the pair (B, M) = (child-block base, tag mask); child c of it lies at
p = B + child_offset(M, c); it is `ne` when its value byte is not 0 and `has` (the walk descends into it) when it is ne,
its tag is 0 and its big-endian child pointer cp is not 0; as a parent it is the state (p + cp, bytes 5..6 big-endian).

    unroll(pool)                               the states level by level from the root pair, and whether the table can state the pool
    check_table(pool, desc, aux, count, fresh) walks a table read out of the library in lockstep with the pool
"""
U32 = 0xffffffff
K_NEW = 0xffffffff       # desc.x of a state the refresh has appended but not unrolled yet
PHANTOM, ROOT = 0, 1     # table indices of the pair (0, 0) and of the root pair
LEVELS = 13              # parent states at depth 0..12
GROUP_BIAS = 64          # desc.x = 8 * (index of the first child descriptor) - 64
HEADROOM = 4096 + 65536
_SIZE = (7, 3, 7, 1)     # record sizes of tags 0..3


class TableError(AssertionError):
    pass


def budget(pool_len):
    """descriptors the library allows a pool's unrolling (its second, larger attempt)"""
    return pool_len // 8 + HEADROOM


def child_offset(mask, c):
    return sum(_SIZE[(mask >> (2 * k)) & 3] for k in range(c))


def desc_word(m_ne, m_has):
    """a nibble per child slot: 0 empty, 1 a hit, 8 | rank = descend into the rank-th child descriptor"""
    w = rank = 0
    for c in range(8):
        if (m_has >> c) & 1:
            w |= (8 | rank) << (4 * c)
            rank += 1
        elif (m_ne >> c) & 1:
            w |= 1 << (4 * c)
    return w


def desc_first(x):
    return ((x + GROUP_BIAS) & U32) >> 3


def desc_base(first):
    return (first * 8 - GROUP_BIAS) & U32


def _bytes(pool):
    return pool if isinstance(pool, bytes) else bytes(bytearray(pool))


def children(pool, B, M):
    """(m_ne, m_has, [(slot, (B', M'), offset of the child's record) for every child the walk descends into])"""
    n = len(pool)
    m_ne = m_has = 0
    kids = []
    off = 0
    for c in range(8):
        tag = (M >> (2 * c)) & 3
        p = (B + off) & U32
        off += _SIZE[tag]
        if p >= n or pool[p] == 0:
            continue
        m_ne |= 1 << c
        if tag != 0:
            continue
        r = pool[p + 1:p + 7]                      # (a slice past the end is short: the missing bytes are 0)
        if len(r) < 6:
            r = r + bytes(6 - len(r))
        cp = (r[0] << 24) | (r[1] << 16) | (r[2] << 8) | r[3]
        if cp == 0:
            continue
        m_has |= 1 << c
        kids.append((c, ((p + cp) & U32, (r[4] << 8) | r[5]), p))
    return m_ne, m_has, kids


def root_state(pool):
    r = pool[1:7] + bytes(6)
    return (((r[0] << 24) | (r[1] << 16) | (r[2] << 8) | r[3]), (r[4] << 8) | r[5])


class Unrolled:
    """levels[d]: the states at depth d reached from the root pair, in table order -- (B, M, m_ne, m_has, [child states]);
    the children of level d, concatenated, are level d + 1.
    phantom: (m_ne, m_has, [(slot, state, shared)]) of the pair (0, 0); shared = "root", ("rootchild", rank) or None.
    phantom_levels[0]: the phantom's children that are not shared (depth 1), [1]: their children (depth 2), ...
    count: the descriptors of a table built from scratch; walkable: whether the library can state the pool; why: if not."""

    def __init__(self):
        self.levels, self.phantom, self.phantom_levels = [], None, []
        self.count, self.walkable, self.why, self.budget = 0, False, "", 0

    @property
    def states(self):
        return sum(len(l) for l in self.levels) + 1 + sum(len(l) for l in self.phantom_levels)


def _expand(pool, states):
    out, nkids = [], 0
    for B, M in states:
        m_ne, m_has, kids = children(pool, B, M)
        out.append((B, M, m_ne, m_has, [k[1] for k in kids]))
        nkids += len(kids)
    return out, nkids


def unroll(pool):
    pool = _bytes(pool)
    u = Unrolled()
    u.budget = cap = budget(len(pool))
    stop = cap + cap // 50          # a cyclic pool grows without end: far enough past the budget to say so
    root = root_state(pool)
    end = 2

    def levels_from(first, depth, into):
        """level by level from the states `first` at `depth`; False when the pool is too deep or too large"""
        nonlocal end
        cur = first
        while cur:
            lvl, nkids = _expand(pool, cur)
            into.append(lvl)
            if depth == LEVELS - 1:
                if nkids:
                    u.why = "a child block below depth %d" % depth
                    return False
                return True
            end += nkids
            if end > stop:
                u.why = "more than %d states" % stop
                return False
            cur = [k for s in lvl for k in s[4]]
            depth += 1
        return True

    ok = levels_from([root], 0, u.levels)
    if ok and end > cap:
        ok, u.why = False, "%d states, budget %d" % (end, cap)
    if ok:
        m_ne, m_has, kids = children(pool, 0, 0)
        rootkids = u.levels[0][0][4]
        ph, unshared = [], []
        for c, st, _ in kids:
            shared = None
            if st == root:
                shared = "root"
            elif st in rootkids:
                shared = ("rootchild", rootkids.index(st))
            else:
                unshared.append(st)
            ph.append((c, st, shared))
        u.phantom = (m_ne, m_has, ph)
        end += len(ph)
        ok = levels_from(unshared, 1, u.phantom_levels)
        if ok and end > cap:
            ok, u.why = False, "%d states, budget %d" % (end, cap)
    u.count = end
    u.walkable = ok
    return u


def check_table(pool, desc, aux, count, fresh):
    """desc, aux: (>= count, 2) uint32 arrays read out of the library.  Walks the table from index 1 (the root pair) and from
    index 0 (the pair (0, 0)) in lockstep with the pool; raises TableError with the index, the path of child slots and the
    pool offset at the first entry that does not state what the pool's bytes say.  fresh: the table was built from scratch,
    so every one of its `count` entries must be reached; otherwise (a table that followed updates) garbage groups may lie
    between the reached ones.  Returns the number of (index, state, depth) triples checked."""
    pool = _bytes(pool)
    count = int(count)
    dx = [int(v) for v in desc[:count, 0]]
    dy = [int(v) for v in desc[:count, 1]]
    ax = [int(v) for v in aux[:count, 0]]
    ay = [int(v) for v in aux[:count, 1]]
    if count < 2 or len(dx) < count:
        raise TableError("a table of %d entries (%d read)" % (count, len(dx)))
    root = root_state(pool)
    seen = set()
    visited = bytearray(count)

    def fail(what, i, path, at):
        raise TableError("%s: index %d, path %s, pool offset %d" % (what, i, "/".join(str(c) for c in path) or "-", at))

    for start, state, from_root in ((ROOT, root, True), (PHANTOM, (0, 0), False)):
        stack = [(start, state, 0, (), 0)]
        while stack:
            i, (B, M), depth, path, at = stack.pop()
            key = (i, B, M, depth)
            if key in seen:
                continue
            seen.add(key)
            visited[i] = 1
            if ax[i] != B:
                fail("aux.x = %d, the child block is at %d" % (ax[i], B), i, path, at)
            if ay[i] & 0xffff != M:
                fail("aux.y mask = 0x%04x, the tag mask is 0x%04x" % (ay[i] & 0xffff, M), i, path, at)
            if from_root and (ay[i] >> 16) & 15 != depth:
                fail("aux.y depth = %d at depth %d" % ((ay[i] >> 16) & 15, depth), i, path, at)
            m_ne, m_has, kids = children(pool, B, M)
            if dy[i] != desc_word(m_ne, m_has):
                fail("desc.y = 0x%08x, the pool says 0x%08x" % (dy[i], desc_word(m_ne, m_has)), i, path, at)
            if dx[i] == K_NEW:
                fail("desc.x = kNew: never unrolled", i, path, at)
            if depth >= LEVELS - 1 and m_has:
                fail("children with a child block (0x%02x) at depth %d" % (m_has, depth), i, path, at)
            first = desc_first(dx[i])
            for rank, (c, st, p) in enumerate(kids):
                j = first + rank
                if not 2 <= j < count:
                    fail("child %d -> index %d outside [2, %d)" % (c, j, count), i, path, at)
                # (below the pair (0, 0) the root pair stands where it does under the root: 13 levels from there)
                d = 0 if (not from_root and i == PHANTOM and st == root) else depth + 1
                stack.append((j, st, d, path + (c,), p))
    if fresh:
        missing = [i for i in range(count) if not visited[i]]
        if missing:
            raise TableError("%d of %d entries are not reached from the root pair or the pair (0, 0), the first at index %d"
                             % (len(missing), count, missing[0]))
    return len(seen)
