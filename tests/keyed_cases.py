"""What the tests of keyed MiMC Merkle trees share (test_merkle_keyed_host.py, test_merkle_keyed_gpu.py): a model of the layout hashed by the oracle's
sponge, brute force over the full padded list, and the catalogue of key sets.

The model is the layout as include/bpg.h states it: per height s (0 = the leaves) a dict {position: value} of the nodes that have a held key below them;
what is absent reads as E_s.  A put writes the leaves and recomputes the proper ancestors of the put keys, each once, bottom-up; it returns how many keys
were inserted and how often it evaluated the node function, height by height: |{k >> s : k put}| for s = 1..depth."""
import hashlib
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
