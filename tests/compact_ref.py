"""The rule of svo_pool_compact restated in plain Python: the pool as exactly its reachable records, in the builder's order.
Reachable: the root record at offset 0 (always interior) and the eight children of every reachable record whose tag in its
parent's mask is 0 -- by tag, not by value.  Order: a node's children block, then the subtrees of its tag-0 children in child
order.  Records verbatim; only the big-endian relative child pointer of interior records is recomputed."""
import numpy as np

SIZE = (7, 3, 7, 1)           # bytes of a record by its tag
MAX_LEVELS = 13               # levels of nodes that own a children block: what the ray walk's stack stands on


class Refused(Exception):
    pass


def compact(pool):
    pool = np.ascontiguousarray(pool, np.uint8)
    out = bytearray(pool[:7].tobytes())

    def lay_out(old, new, level):
        """the record at `old` stands at out[new]: its children block and what hangs below go to the end of out"""
        if level >= MAX_LEVELS:
            raise Refused("more than %d levels (or a cycle)" % MAX_LEVELS)
        blk = old + int.from_bytes(pool[old + 1:old + 5].tobytes(), "big", signed=True)
        mask = (int(pool[old + 5]) << 8) | int(pool[old + 6])
        tags = [(mask >> (2 * c)) & 3 for c in range(8)]
        nbytes = sum(SIZE[t] for t in tags)
        if blk < 0 or blk + nbytes > pool.size:
            raise Refused("block [%d, %d) outside [0, %d)" % (blk, blk + nbytes, pool.size))
        start = len(out)
        out.extend(pool[blk:blk + nbytes].tobytes())
        out[new + 1:new + 5] = (start - new).to_bytes(4, "big")
        off = 0
        for t in tags:
            if t == 0:
                lay_out(blk + off, start + off, level + 1)
            off += SIZE[t]

    lay_out(0, 0, 0)
    return np.frombuffer(bytes(out), np.uint8).copy()
