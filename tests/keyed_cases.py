"""What the tests of keyed MiMC Merkle trees share (test_merkle_keyed_host.py, test_merkle_keyed_gpu.py): a model of the layout hashed by the oracle's
sponge, brute force over the full padded list, the catalogue of key sets, and the put scenarios (a base and one or two puts that reach one path of the
structure phase each: tiles_mixed, in_place, second_trip) with the integer-only model of what a put classifies, scans and merges.

The model is the layout as include/bpg.h states it: per height s (0 = the leaves) a dict {position: value} of the nodes that have a held key below them;
what is absent reads as E_s.  A put writes the leaves and recomputes the proper ancestors of the put keys, each once, bottom-up; it returns how many keys
were inserted and how often it evaluated the node function, height by height: |{k >> s : k put}| for s = 1..depth."""
import collections
import functools
import hashlib
import random
import oracle_lib as O
import pyref as R

le = lambda x: x.to_bytes(32, "little")
red = lambda b: le(int.from_bytes(b, "little") % R.L)
EMPTIES = [None, le(R.L - 1), le(2**256 - 1)]                  # NULL = zero, l - 1, and a value >= l: `empty` is taken mod l
TOP = 256                                                      # a height with more dirty parents than this is one launch of its own
_NODES = {}


def node(left, right):
    """the oracle's sponge over two children; a pair that was hashed before is not hashed again"""
    v = _NODES.get((left, right))
    if v is None:
        v = _NODES[(left, right)] = O.mimc_sponge(left + right)
    return v


def empty_chain(depth, empty=None):
    E = [red(empty or bytes(32))]
    for _ in range(depth):
        E.append(node(E[-1], E[-1]))
    return E


def rand_scalars(tag, n):
    out, i = [], 0
    while len(out) < n:
        d = hashlib.shake_256(b"%s-%d" % (tag, i)).digest(32 * 64)
        out += [le(int.from_bytes(d[32 * k:32 * k + 32], "little") % R.L) for k in range(64)]
        i += 1
    return out[:n]


def rand_keys(tag, n, depth):
    """n distinct seeded keys below 2^depth, in the order they were drawn (not sorted)"""
    out, seen, i = [], set(), 0
    while len(out) < n:
        d = hashlib.shake_256(b"keys-%s-%d" % (tag, i)).digest(8 * 64)
        for k in range(64):
            v = int.from_bytes(d[8 * k:8 * k + 8], "little") >> (64 - depth)
            if v not in seen and len(out) < n:
                seen.add(v); out.append(v)
        i += 1
    return out


def leaf_of(key):
    """the leaf every test puts at `key` first: any function of the key that is no constant"""
    return le((0x1000 + 7 * key * key + key) % R.L)


class KeyedModel:
    def __init__(self, depth, empty=None):
        self.depth, self.E = depth, empty_chain(depth, empty)
        self.h = [dict() for _ in range(depth + 1)]

    def value(self, s, p):
        return self.h[s].get(p, self.E[s])

    def put(self, keys, leaves):
        """-> (keys inserted, [node evaluations at height 1, ..., at height depth])"""
        assert len(set(keys)) == len(keys) == len(leaves) and all(0 <= k < 1 << self.depth for k in keys)
        inserted = sum(1 for k in keys if k not in self.h[0])
        for k, leaf in zip(keys, leaves):
            self.h[0][k] = red(leaf)
        dirty, evals = set(keys), []
        for s in range(1, self.depth + 1):
            dirty = {p >> 1 for p in dirty}
            for p in dirty:
                self.h[s][p] = node(self.value(s - 1, 2 * p), self.value(s - 1, 2 * p + 1))
            evals.append(len(dirty))
        return inserted, (evals if keys else [0] * self.depth)

    def root(self):
        return self.value(self.depth, 0)

    def siblings(self, i):
        return [self.value(s, (i >> s) ^ 1) for s in range(self.depth)]

    def on_path(self, i):
        return [self.value(s, i >> s) for s in range(1, self.depth + 1)]

    def keys(self):
        return sorted(self.h[0])

    def counts(self):
        return [len(x) for x in self.h]

    def get(self, keys):
        return [self.value(0, k) for k in keys], [k in self.h[0] for k in keys]

    def level(self, level, first=0, count=None):
        """nodes of `level` (0 = the root) as MerkleTree.nodes gives them"""
        s = self.depth - level
        count = (1 << level) - first if count is None else count
        return [self.value(s, p) for p in range(first, first + count)]

    def check_invariant(self):
        """height s holds exactly the distinct key >> s"""
        for s in range(self.depth + 1):
            assert set(self.h[s]) == {k >> s for k in self.h[0]}, s


def brute_levels(depth, held, empty=None):
    """levels[0] = [root] ... levels[depth] = the 2^depth leaves of the tree over the full list that is `empty` everywhere but at the keys of `held`"""
    e = red(empty or bytes(32))
    level = [red(held[k]) if k in held else e for k in range(1 << depth)]
    levels = [level]
    while len(level) > 1:
        level = [node(level[i], level[i + 1]) for i in range(0, len(level), 2)]
        levels.append(level)
    return levels[::-1]


def padded(depth, held, empty=None):
    """the full leaf list of brute_levels, for a dense tree of the same device to be built from"""
    e = empty or bytes(32)
    return [held[k] if k in held else e for k in range(1 << depth)]


def counts_of(held, depth):
    """the model's per-height node counts without its hashing: |{k >> s : k held}| for s = 0..depth"""
    return [len({k >> s for k in held}) for s in range(depth + 1)]


def evals_of(keys, depth):
    """the model's per-height evaluations of a put of `keys` without its hashing: |{k >> s}| for s = 1..depth"""
    return [len({k >> s for k in keys}) for s in range(1, depth + 1)]


def hashing_launches(evals):
    """what a put launches for these per-height evaluations: one launch per height above 256 parents, and the climb"""
    return sum(1 for m in evals if m > TOP) + (1 if any(evals) else 0)


def chosen_sets(depth):
    """the catalogue of key sets of test 3, by name; keys unsorted where the set has an order to lose"""
    n, half = 1 << depth, 1 << (depth - 1)
    sets = {
        "none": [], "first": [0], "last": [n - 1], "siblings": [1, 0], "adjacent non-siblings": [2, 1], "across the middle": [half, half - 1],
        "even": list(range(n - 2, -1, -2)), "odd": list(range(1, n, 2)), "all": list(range(n - 1, -1, -1)),
        "random 300": rand_keys(b"chosen%d" % depth, 300, depth),
    }
    if depth == 13:
        for k in (1023, 1024, 1025, 4095, 4096, 4097):
            sets["random %d" % k] = rand_keys(b"tile%d" % k, k, depth)
    return sets


DEEP_KEYS = [0, 1, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1]


# ---------------------------------------------------------------------------------------------------------------- put scenarios, and what of a put is integers only
TILE = 1024                                                    # MERKLE_KEYED_SCAN_TILE: the flags one block of the scan kernels covers
TOP_TILES = 256                                                # tile sums k_mkx_scan_top scans per trip
MIN_CAPACITY = 64                                              # MERKLE_KEYED_MIN_CAPACITY
Scenario = collections.namedtuple("Scenario", "name depth base puts")      # base: the keys the tree is built over; puts: [(keys, "held" | "new" | "mixed")]


def put_flags(held, keys):
    """flags.x of k_mkx_classify at height 0, in the order the device sees the put: per SORTED key 1 when it is brand-new (not held)"""
    return [0 if k in held else 1 for k in sorted(keys)]


def tile_counts(flags):
    """per scan tile (the flags it covers, how many of them are set)"""
    return [(len(flags[i:i + TILE]), sum(flags[i:i + TILE])) for i in range(0, len(flags), TILE)]


def put_lists(held, keys, depth):
    """per height s = 0..depth of a put of `keys` into a tree that holds `held`: (the dirty positions |{k >> s}|, how many of them are brand-new), by sets"""
    out = []
    for s in range(depth + 1):
        stored, dirty = {k >> s for k in held}, {k >> s for k in keys}
        out.append((len(dirty), len(dirty - stored)))
    return out


def put_lists_np(held, keys, depth):
    """put_lists by numpy.unique and numpy.isin on integer arrays (nothing is hashed): what depth 19 needs to stay quick"""
    import numpy as np
    h, k, out = np.unique(np.asarray(held, dtype=np.int64)), np.unique(np.asarray(keys, dtype=np.int64)), []
    for s in range(depth + 1):
        out.append((len(k), int(len(k) - np.isin(k, h, assume_unique=True).sum())))
        h, k = np.unique(h >> 1), np.unique(k >> 1)
    return out


def counts_np(held, depth):
    """counts_of by numpy.unique"""
    import numpy as np
    h, out = np.unique(np.asarray(held, dtype=np.int64)), []
    for s in range(depth + 1):
        out.append(len(h))
        h = np.unique(h >> 1)
    return out


def classified(lists):
    """the heights Engine::merkle_put runs k_mkx_classify at with classify == 1: height 0, and every height up to and including the first that finds no
    brand-new position.  Above it flags.x is written as zeros without a lookup (classify == 0); the root (height depth) has no launch."""
    out = []
    for s, (_, fresh) in enumerate(lists[:-1]):
        out.append(s)
        if not fresh:
            break
    return out


def capacity(cap, need, limit):
    """merkle_keyed_capacity of csrc/host/merkle_keyed_plan.hpp"""
    return cap if need <= cap else max(need, min(limit, max(MIN_CAPACITY, 2 * cap, need)))


def capacities(caps, counts, depth):
    """the room per height after a put that leaves `counts` nodes stored in arrays that had room for `caps`"""
    return [capacity(c, n, min(1 << (depth - s), 1 << 24)) for s, (c, n) in enumerate(zip(caps, counts))]


def merge_kinds(caps, before, after, depth):
    """per height of a put that takes the stored counts from `before` to `after`: None (no brand-new position: no merge), "grows" (new arrays, the old
    ones retired) or "in place" (merged into the context's scratch and copied back) -> (the kinds, the room afterwards)"""
    new_caps = capacities(caps, after, depth)
    return [None if a == b else ("grows" if nc != c else "in place") for c, nc, b, a in zip(caps, new_caps, before, after)], new_caps


# the pairs of "tiles mixed": what the two keys 2q, 2q + 1 of a pair are.  '.' not held, not put; 'h' held, not put; 'H' held and put; 'N' not held and put
# (brand-new).  A pair with an 'N' has an 'h' or 'H' beside it, so EVERY dirty position of height 1 is held: height 1 is the first height without a
# brand-new position and everything above runs with classify == 0.  The weights keep the base near 3,000 keys.
_PAIRS = (("HH", 1.0), ("HN", 5.0), ("NH", 5.0), ("H.", 0.75), (".H", 0.75), ("Hh", 0.1), ("hH", 0.1), ("Nh", 0.5), ("hN", 0.5), ("..", 0.5), ("h.", 0.05), (".h", 0.05))
_TILES_SEED = 13


def _tiles_rule(i, flag, flags):
    """may sorted put key i carry this brand-new flag?  tile 0 all held, tile 1 all brand-new, a change at 2,047 | 2,048 and at 3,071 | 3,072"""
    if i < TILE:
        return flag == 0
    if i < 2 * TILE:
        return flag == 1
    if i == 2 * TILE:
        return flag == 0
    if i == 3 * TILE:
        return flag != flags[i - 1]
    return i < 4 * TILE


@functools.lru_cache(maxsize=None)
def tiles_mixed(last):
    """Depth 13: a base of about 3,000 keys and ONE put of 4,097 keys whose brand-new flags, in sorted order, are by scan tile: none, all, irregular,
    irregular, and a tile of one flag - `last` = "new" or "held" says which.  Both variants share the base and the first 4,096 keys.  The pairs of keys
    are drawn left to right from a seeded generator, each kind of pair (_PAIRS) allowed where _tiles_rule allows its flags."""
    assert last in ("new", "held")
    depth, rnd = 13, random.Random(_TILES_SEED)
    base, put, flags, q = [], [], [], 0
    while len(put) < 4 * TILE:
        def fits(kind):
            f = list(flags)
            for c in kind:
                if c in "HN":
                    if not _tiles_rule(len(f), 1 if c == "N" else 0, f):
                        return False
                    f.append(1 if c == "N" else 0)
            return True
        allowed = [(kind, 8 * w if kind == "HH" and len(put) < TILE else w) for kind, w in _PAIRS if fits(kind)]      # (tile 0 has no "HN": mostly "HH" there)
        x = rnd.random() * sum(w for _, w in allowed)
        for kind, w in allowed:
            x -= w
            if x < 0:
                break
        for side, c in enumerate(kind):
            if c in "hH":
                base.append(2 * q + side)
            if c in "HN":
                put.append(2 * q + side); flags.append(1 if c == "N" else 0)
        q += 1
    base.append(2 * q)                                          # the pair of the last key: its left key is held, its right key is not
    put.append(2 * q + (1 if last == "new" else 0))
    assert 2 * q + 1 < 1 << depth
    rnd.shuffle(base)
    return Scenario("tiles mixed, the last key %s" % last, depth, tuple(base), ((tuple(put), "mixed"),))


@functools.lru_cache(maxsize=None)
def in_place():
    """Depth 13: 3,000 keys; 1,500 new ones, which make the low heights outgrow their arrays (height 0: 3,000 -> room for 6,000); then 1,000 keys of which
    500 are held, which fit the room there is: every height that gains a position merges in the context's scratch, each with another total"""
    keys = rand_keys(b"in place", 5000, 13)
    base, more, late = keys[:3000], keys[3000:4500], keys[4500:]
    mixed = base[100:400] + late[:250] + more[200:400] + late[250:]
    return Scenario("in place", 13, tuple(base), ((tuple(more), "new"), (tuple(mixed), "mixed")))


@functools.lru_cache(maxsize=None)
def second_trip(last):
    """Depth 19: a base of 2^17 keys; put A of exactly 262,144 keys = 256 scan tiles, ONE trip of k_mkx_scan_top; put B of exactly 262,145 keys = 257 tiles:
    the second trip holds one tile of one flag, the largest key of B, which is brand-new or held as `last` says.  100,000 keys of A and 130,000 of the
    other keys of B are held when they are put.  Keys as drawn, not sorted."""
    import numpy as np
    assert last in ("new", "held")
    depth, n = 19, 1 << 19
    rs = np.random.RandomState(19)
    perm = rs.permutation(n)
    base, rest = perm[:1 << 17], perm[1 << 17:]
    a = np.concatenate([base[:100000], rest[:162144]])
    rs.shuffle(a)
    held, free = np.concatenate([base, rest[:162144]]), rest[162144:]
    top = {"held": int(held.max()), "new": int(free.max())}
    below = min(top.values())                                    # every other key of B is below both candidates for its last key
    held_part, new_part = rs.permutation(held), free
    b = np.concatenate([held_part[held_part < below][:130000], new_part[new_part < below][:132144], [top[last]]])
    rs.shuffle(b)
    assert len(a) == 262144 and len(b) == 262145
    return Scenario("second trip, the last key %s" % last, depth, tuple(base.tolist()), ((tuple(a.tolist()), "mixed"), (tuple(b.tolist()), "mixed")))


def scenario_states(sc):
    """the keys held before every put of a scenario, and after the last one: [set, ...]"""
    held, out = set(sc.base), []
    for keys, _ in sc.puts:
        out.append(set(held))
        held |= set(keys)
    return out + [held]


def kind_of(held, keys):
    fresh = sum(1 for k in keys if k not in held)
    return "held" if not fresh else ("new" if fresh == len(keys) else "mixed")
