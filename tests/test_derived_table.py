"""The whole interior-descriptor table (svo-raytracer_amd/csrc/svo_derive.hip.h) against a plain unrolling of the pool
(tests/derived_ref.py), entry by entry -- not only the entries the rays of a frame happen to visit.

CPU part: a table laid out in Python the way build_table lays it out is accepted by the checker, and every kind of
single-entry damage is rejected (so the checker can fail).  GPU part: the table the library builds for a range of pools
(svo_derived_read), and the table after every single svo_pool_update of several edit scenarios, which refresh_table has
followed without a rebuild -- or has given up on, in which case the rebuilt one is read."""
import os

import numpy as np
import pytest

import derived_ref as R
import derived_edits as E

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}


def _fuzz():
    if "z" not in _cache:
        _cache["z"] = np.load(os.path.join(HERE, "golden", "fuzz_golden.npz"))
    return _cache["z"]


def _fuzz_pools():
    return sorted(k[5:] for k in _fuzz().files if k.startswith("pool/"))


def _scene(n):
    import svo_raytracer_amd.scene as scene
    if ("scene", n) not in _cache:
        _cache["scene", n] = scene.build_scene(n)[0]
    return _cache["scene", n]


def _pool(name):
    if name.startswith("scene"):
        return _scene(int(name[5:]))
    if name in E.HAND_MADE:
        return E.HAND_MADE[name]()
    return _fuzz()["pool/" + name]


def reference_table(u):
    """(desc, aux) of the unrolling u, every entry where build_table puts it: index 0 the pair (0, 0), 1 the root pair, then
    the root's levels, then the children of (0, 0) -- shared ones as copies -- and the levels below the ones not shared"""
    assert u.walkable
    desc = np.zeros((u.count, 2), np.uint32)
    aux = np.zeros((u.count, 2), np.uint32)
    end = 2

    def place(where, lvl, depth):
        nonlocal end
        first = end
        for i, (B, M, m_ne, m_has, kids) in zip(where, lvl):
            aux[i] = (B, M | (depth << 16))
            desc[i] = (0 if depth == R.LEVELS - 1 else R.desc_base(end), R.desc_word(m_ne, m_has))
            end += len(kids)
        return list(range(first, end))

    where = [R.ROOT]
    for depth, lvl in enumerate(u.levels):
        where = place(where, lvl, depth)
    m_ne, m_has, ph = u.phantom
    desc[R.PHANTOM] = (R.desc_base(end), R.desc_word(m_ne, m_has))
    rootkid0 = R.desc_first(int(desc[R.ROOT, 0]))
    ph0, where = end, []
    end += len(ph)
    for k, (c, st, shared) in enumerate(ph):
        aux[ph0 + k] = (st[0], st[1] | (1 << 16))
        if shared == "root":
            desc[ph0 + k] = desc[R.ROOT]
        elif shared is not None:
            desc[ph0 + k] = desc[rootkid0 + shared[1]]
        else:
            where.append(ph0 + k)
    for depth, lvl in enumerate(u.phantom_levels, 1):
        where = place(where, lvl, depth)
    assert end == u.count, (end, u.count)
    return desc, aux


TABLE_POOLS = ["scene64", "t_root", "t_loop", "t_leaves", "t_surf", "m3", "chain13", "root_cp0"]


@pytest.fixture(scope="module")
def tables():
    out = {}
    for name in TABLE_POOLS:
        pool = _pool(name)
        u = R.unroll(pool)
        assert u.walkable, (name, u.why)
        out[name] = (pool, u) + reference_table(u)
    return out


def test_plain_unrolling_counts_the_states_of_the_terrains():
    assert R.unroll(_scene(64)).states - 1 == 3530       # (- 1: the pair (0, 0) is no state of the tree)
    assert R.unroll(_scene(128)).states - 1 == 14415
    u = R.unroll(_pool("t_surf"))
    assert [len(l) for l in u.levels] == [1] and u.count == 2 + 5 and u.phantom[1] == 0b00011111 & u.phantom[0]


@pytest.mark.parametrize("name", TABLE_POOLS)
def test_checker_accepts_a_table_laid_out_like_a_fresh_build(tables, name):
    pool, u, desc, aux = tables[name]
    n = R.check_table(pool, desc, aux, u.count, fresh=True)
    assert n >= u.states
    assert R.check_table(pool, desc, aux, u.count, fresh=False) == n


def _rejects(pool, desc, aux, count, fresh=False):
    with pytest.raises(R.TableError) as e:
        R.check_table(pool, desc, aux, count, fresh)
    assert "index" in str(e.value)
    return 1


def _nibbles(w):
    return [(w >> (4 * c)) & 15 for c in range(8)]


@pytest.mark.parametrize("name", TABLE_POOLS)
def test_checker_rejects_every_single_damaged_entry(tables, name):
    """One entry changed at a time, at up to 14 entries spread over the table (all of a tiny one): each change must raise."""
    pool, u, desc0, aux0 = tables[name]
    count = u.count
    rootlen = 2 + sum(len(l) for l in u.levels[1:])       # [1, rootlen): reached from the root pair, depth bits checked
    picks = sorted(set(int(v) for v in np.linspace(0, count - 1, 12)) | {0, 1})
    done = dict.fromkeys(("0->1", "1->0", "1->8", "rank", "x+8", "x-8", "knew", "knew_leaf", "auxx+1", "auxx-1", "mask", "depth"), 0)

    def damaged(i, col, value, table="desc"):
        desc, aux = desc0.copy(), aux0.copy()
        (desc if table == "desc" else aux)[i, col] = np.uint32(value & 0xffffffff)
        return pool, desc, aux, count

    for i in picks:
        w, x = int(desc0[i, 1]), int(desc0[i, 0])
        nib = _nibbles(w)
        for c, v in enumerate(nib):
            if v == 0:
                done["0->1"] += _rejects(*damaged(i, 1, w | (1 << (4 * c))))
            elif v == 1:
                done["1->0"] += _rejects(*damaged(i, 1, w & ~(15 << (4 * c))))
                done["1->8"] += _rejects(*damaged(i, 1, (w & ~(15 << (4 * c))) | (8 << (4 * c))))
            elif v >= 8:
                done["rank"] += _rejects(*damaged(i, 1, w ^ (1 << (4 * c))))
        if any(v >= 8 for v in nib):
            done["x+8"] += _rejects(*damaged(i, 0, x + 8))
            done["x-8"] += _rejects(*damaged(i, 0, x - 8))
        else:
            done["knew_leaf"] += 1
        done["knew"] += _rejects(*damaged(i, 0, R.K_NEW))
        done["auxx+1"] += _rejects(*damaged(i, 0, int(aux0[i, 0]) + 1, "aux"))
        done["auxx-1"] += _rejects(*damaged(i, 0, int(aux0[i, 0]) - 1, "aux"))
        done["mask"] += _rejects(*damaged(i, 1, int(aux0[i, 1]) ^ 0x0100, "aux"))
        if 1 <= i < rootlen:
            done["depth"] += _rejects(*damaged(i, 1, int(aux0[i, 1]) + (1 << 16), "aux"))
    # an entry more than the unrolling has: garbage in a table that claims to be fresh (fine in one that followed updates)
    desc1, aux1 = np.vstack([desc0, desc0[-1:]]), np.vstack([aux0, aux0[-1:]])
    _rejects(pool, desc1, aux1, count + 1, fresh=True)
    R.check_table(pool, desc1, aux1, count + 1, fresh=False)
    print(name, count, done)
    assert done["knew"] and done["auxx+1"] and done["auxx-1"] and done["mask"] and done["depth"] and done["0->1"] and done["1->0"]
    assert done["knew_leaf"]                               # kNew was also tried where desc.x is not otherwise looked at
    if name in ("scene64", "m3"):
        assert all(done.values()), done


def test_checker_rejects_a_table_one_level_deeper_than_the_walk_can_stand_on(monkeypatch):
    """a chain of 14 unrolled and laid out as if 14 levels were allowed: every entry states the pool, and the state at depth
    12 has a child block -- which is the one thing wrong with it"""
    pool = _pool("chain14")
    monkeypatch.setattr(R, "LEVELS", 14)
    u = R.unroll(pool)
    desc, aux = reference_table(u)
    assert R.check_table(pool, desc, aux, u.count, fresh=True) >= 15
    monkeypatch.undo()
    with pytest.raises(R.TableError, match="at depth 12"):
        R.check_table(pool, desc, aux, u.count, fresh=True)


def test_pools_the_table_cannot_state_are_reported():
    """a child block below depth 12 (a chain of 14, and the cycles of the mangled pool m0 and of a 21-byte loop) and an
    unrolling past the budget (a block whose eight children all point back at it)"""
    for name in ("chain14", "m0", "loop_back"):
        u = R.unroll(_pool(name))
        assert not u.walkable and "depth" in u.why, (name, u.why)
    u = R.unroll(_pool("loop_wide"))
    assert not u.walkable and "states" in u.why, u.why
    # t_loop (8 bytes, the root record and one zero byte) is no cycle for the walk: the root's cp is 0, so its first
    # child -- the root record read again -- has no child block.  Two states: the pair (0, 0) and the root pair, the same
    u = R.unroll(_pool("t_loop"))
    assert u.walkable and u.count == 2 and u.levels[0][0][:4] == (0, 0, 1, 0)


# ---------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def ctx():
    from svo_raytracer_amd import hiplib
    c = hiplib.HipContext(0)
    c.set_pipeline(1)
    c.set_derived(1)
    yield c
    c.close()


def _fresh_names():
    return _fuzz_pools() + ["caves", "dust", "scene128", "chain12", "chain13", "chain14", "root_cp0", "loop_back", "loop_wide", "short40"]


def _check_fresh(ctx, name, pool):
    u = R.unroll(pool)
    assert abs(u.count - u.budget) > u.budget // 100 or u.count > u.budget + u.budget // 100, \
        "%s: %d states within 1 %% of the budget %d: pick another pool" % (name, u.count, u.budget)
    ctx.pool_upload(pool)
    info = ctx.derived_info()
    assert info["walkable"] == u.walkable, (name, info, u.why)
    if not u.walkable:
        return u, 0
    assert info["descriptors"] == u.count, (name, info, u.count)
    desc, aux = ctx.derived_read()
    return u, R.check_table(pool, desc, aux, u.count, fresh=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _fresh_names())
def test_fresh_table_states_the_whole_pool(ctx, name):
    pool = _pool(name) if name not in ("caves", "dust") else E.family_pool(name)
    u, n = _check_fresh(ctx, name, pool)
    print(name, pool.size, "walkable" if u.walkable else "not walkable: " + u.why, u.count, "checked", n)
    if name == "chain13":
        desc, aux = ctx.derived_read()
        deepest = [i for i in range(u.count) if (int(aux[i, 1]) >> 16) & 15 == 12]
        assert deepest and all(int(desc[i, 0]) == 0 for i in deepest)
    assert u.walkable == (name not in ("chain14", "loop_back", "loop_wide", "m0", "m1"))


@pytest.mark.gpu
def test_read_refuses_a_range_past_the_table(ctx):
    from svo_raytracer_amd import hiplib
    pool = _pool("t_surf")
    ctx.pool_upload(pool)
    n = ctx.derived_info()["descriptors"]
    d, a = ctx.derived_read(n - 1, 1)
    full = ctx.derived_read()
    assert (d == full[0][-1:]).all() and (a == full[1][-1:]).all()
    assert ctx.derived_read(n, 0)[0].shape == (0, 2)
    # refused before anything is copied: the raw export, with buffers of one entry
    d1, a1 = np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.uint32)
    for first, count in ((n, 1), (0, n + 1), (n + 1, 0), (1 << 40, 1), (1, (1 << 64) - 1), ((1 << 64) - 1, 2)):
        rc = hiplib.lib().svo_derived_read(ctx._h, first, count, d1.ctypes.data, a1.ctypes.data)
        assert rc == -1 and not d1.any() and not a1.any(), (first, count, rc)     # SVO_E_INVALID
    with pytest.raises(hiplib.SvoError):
        ctx.derived_read(n, 1)


class _Followed:
    """one scenario: every update is sent through svo_pool_update and applied to a host mirror of the pool as the GPU holds
    it (an edit that is sent as two ranges is half applied after the first), and the table is checked against the mirror"""

    def __init__(self, ctx, name, pool):
        self.ctx, self.name = ctx, name
        ctx.pool_upload(pool)
        self.pool = np.array(pool, np.uint8)
        info = ctx.derived_info()
        assert info["walkable"], name
        self.refreshes = self.updates = self.checked = 0
        self.log = []

    def update(self, host, lo, hi, expect=None):
        """expect: True = the refresh must follow it, False = it must give up (a rebuild), None = either"""
        before = self.ctx.derived_refresh_info()["refreshes"]
        self.ctx.pool_update(host, lo, hi)
        if hi > self.pool.size:
            self.pool = np.concatenate([self.pool, np.zeros(hi - self.pool.size, np.uint8)])
        self.pool[lo:hi] = host[lo:hi]
        host = self.pool
        followed = self.ctx.derived_refresh_info()["refreshes"] - before
        info = self.ctx.derived_info()
        u = None
        if not followed or not info["walkable"]:
            u = R.unroll(host)                      # rebuilt: what a fresh build says
            assert info["walkable"] == u.walkable, (self.name, lo, hi, info, u.why)
        n = 0
        if info["walkable"]:
            desc, aux = self.ctx.derived_read()
            try:
                n = R.check_table(host, desc, aux, info["descriptors"], fresh=not followed)
            except R.TableError as e:
                raise R.TableError("%s, update [%d, %d) #%d (%s): %s" % (self.name, lo, hi, self.updates,
                                                                        "followed" if followed else "rebuilt", e)) from None
        self.log.append((lo, hi, followed, n))
        self.updates += 1
        self.refreshes += followed
        self.checked = n
        if expect is not None:
            assert bool(followed) == expect, (self.name, lo, hi, "followed" if followed else "rebuilt")
        return followed

    def finish(self, host):
        """the final pool uploaded whole: a fresh table, complete, and no larger than the grown one"""
        assert self.pool.size == host.size and (self.pool == host).all(), "the updates sent do not add up to the final pool"
        grown = self.ctx.derived_info()
        u, n = _check_fresh(self.ctx, self.name, host)
        if grown["walkable"] and u.walkable:
            assert u.count <= grown["descriptors"], (self.name, u.count, grown)
        print("%s: %d updates, %d followed, %d states checked after the last, %d in the fresh table"
              % (self.name, self.updates, self.refreshes, self.checked, n))
        return n


@pytest.mark.gpu
def test_table_after_every_brush_stroke(ctx):
    """the 14 strokes of test_sdf_edit.test_descriptor_table_follows_brush_strokes_without_a_rebuild (128^3)"""
    pool = _scene(128)
    s = _Followed(ctx, "brush strokes", pool)
    host = pool
    for stroke, host, cb, root_changed in E.brush_strokes(pool):
        for lo, hi in ((cb[0], cb[1]), (cb[2], cb[3])):
            if hi > lo:
                s.update(host, lo, hi, expect=None if root_changed else True)
    assert s.updates >= 15 and s.refreshes >= 10
    s.finish(host)


@pytest.mark.gpu
def test_table_after_every_random_record_edit(ctx):
    """the 40 edits of test_gpu_derived.test_refreshed_table_equals_a_rebuilt_one_under_random_record_edits (64^3)"""
    host = _scene(64).copy()
    s = _Followed(ctx, "record edits", host)
    for edit, kind, lo, hi in E.record_edits(host):
        s.update(host, lo, hi)
    assert s.updates >= 35 and s.refreshes >= 10
    s.finish(host)


@pytest.mark.gpu
def test_table_after_every_range_of_a_replaced_tree(ctx):
    """one tree replaced by another range by range (test_gpu_derived.test_table_follows_ranged_pool_updates): in between the
    pool is a mix of the two, whatever that unrolls to"""
    a, b = _scene(128), _scene(256)
    s = _Followed(ctx, "tree replaced", a)
    for host, lo, hi in E.replace_ranges(a, b):
        s.update(host, lo, hi)
    assert s.updates >= 3
    s.finish(host)


@pytest.mark.gpu
def test_table_after_updates_at_the_edges_of_a_child_block(ctx):
    """one- and two-byte ranges on the first and the last byte of a child block, one byte before and one byte past it, and on
    a block two states share; each must be followed (none touches the root record), and the table must state the pool after
    each, whether or not a state was listed"""
    host = _scene(64).copy()
    s = _Followed(ctx, "block edges", host)
    said, prev = [], host.copy()
    for what, lo, hi in E.block_edge_edits(host):
        s.update(host, lo, hi, expect=True)
        listed, least = ctx.derived_refresh_info()["states"], E.states_over(prev, lo, hi)
        said.append((what, lo, hi, "followed", listed, least))
        prev = host.copy()
    print(said)
    # every one of these ranges lies in some child block: at least the distinct states over it are listed (more when a
    # state has several descriptors, or garbage groups still state it)
    assert all(least >= 1 and listed >= least for *_, listed, least in said), said
    s.finish(host)


@pytest.mark.gpu
def test_table_after_edits_no_frame_of_the_fixed_camera_sees(ctx):
    """a value byte cleared and set again behind the camera K1, an edit inside the child block of the pair (0, 0) (bytes 7..55)
    that leaves the root record alone, and an update that appends past the old end of the pool"""
    host = _scene(64).copy()
    s = _Followed(ctx, "unseen edits", host)
    o = E.record_behind_camera(host, "K1")
    old = int(host[o])
    for v in (0, old, 0, old):
        host[o] = v
        s.update(host, o, o + 1, expect=True)
    for what, hst, lo, hi in E.phantom_block_edits(host):
        host = hst
        s.update(host, lo, hi, expect=True)
    for what, hst, lo, hi in E.appending_edits(host):
        host = hst
        s.update(host, lo, hi, expect=True)
    s.finish(host)


@pytest.mark.gpu
def test_table_follows_a_chain_to_its_thirteenth_level_and_gives_up_at_the_fourteenth(ctx):
    host = E.chain_pool(12)
    s = _Followed(ctx, "chain", host)
    host, lo, hi = E.chain_append(host)                 # 13 levels: the deepest state the table can hold
    s.update(host, lo[1], hi[1], expect=True)           # (the new block first, then the pointer to it: both followed)
    s.update(host, lo[0], hi[0], expect=True)
    assert ctx.derived_info()["walkable"]
    desc, aux = ctx.derived_read()
    deepest = [i for i in range(len(aux)) if (int(aux[i, 1]) >> 16) & 15 == 12 and int(desc[i, 0]) != R.K_NEW]
    assert deepest and R.unroll(host).walkable
    host, lo, hi = E.chain_append(host)                 # 14: the refresh must give up, the rebuilt table says not walkable
    s.update(host, lo[1], hi[1], expect=True)
    s.update(host, lo[0], hi[0], expect=False)
    assert not ctx.derived_info()["walkable"] and not R.unroll(host).walkable
    s.finish(host)
