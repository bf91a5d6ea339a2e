"""CPU tests of keyed Merkle trees (no GPU needed): the model of tests/keyed_cases.py against brute force with the oracle's sponge, csrc/host/
merkle_keyed_plan.hpp - the index rules the kernels of csrc/hip/k_merkle_keyed.cuh run, and the hashing plan - replayed on host arrays against brute
force, that every put scenario of keyed_cases reaches the device path it is for (by integers alone), and what the five new C calls declare, export and
refuse before they touch a device."""
import ctypes as C
import itertools
import re
import subprocess
import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import keyed_cases as K

CALLS = ("bpg_merkle_build_keyed", "bpg_merkle_put", "bpg_merkle_get", "bpg_merkle_keys", "bpg_merkle_node_counts")
PLAN = O.ROOT / "bulletproofs_gadgets_amd" / "csrc" / "host" / "merkle_keyed_plan.hpp"


# ---------------------------------------------------------------------------------------------------------------- the model against brute force
def same_as_brute(m, held, empty):
    depth = m.depth
    want = K.brute_levels(depth, held, empty)
    for level in range(depth + 1):
        assert m.level(level) == want[level], (depth, sorted(held), level)
    m.check_invariant()
    assert m.keys() == sorted(held) and m.counts() == K.counts_of(held, depth)
    for i in range(1 << depth):
        assert m.siblings(i) == [want[depth - s][(i >> s) ^ 1] for s in range(depth)]
        assert m.on_path(i) == [want[depth - s][i >> s] for s in range(1, depth + 1)]


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_model_equals_brute_force_for_every_subset(depth):
    """every subset of the 2^depth keys, built in one put with the keys in descending order; `empty` rotates over NULL, l - 1 and a value >= l"""
    n = 1 << depth
    for mask in range(1 << n):
        empty = K.EMPTIES[mask % 3]
        keys = [k for k in range(n - 1, -1, -1) if mask >> k & 1]
        m = K.KeyedModel(depth, empty)
        inserted, evals = m.put(keys, [K.leaf_of(k) for k in keys])
        assert inserted == len(keys) and evals == (K.evals_of(keys, depth) if keys else [0] * depth)
        if depth == 4 and mask % 7:                        # at depth 4 every subset is compared node by node, and every seventh path by path as well
            want = K.brute_levels(depth, {k: K.leaf_of(k) for k in keys}, empty)
            assert all(m.level(level) == want[level] for level in range(depth + 1)), mask
            continue
        same_as_brute(m, {k: K.leaf_of(k) for k in keys}, empty)


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_model_put_sequences(depth):
    """held keys only, new keys before, after and between the held ones, mixed, a leaf equal to `empty`: after every step the model is the brute-force tree"""
    n, empty = 1 << depth, K.le(5)
    m, held = K.KeyedModel(depth, empty), {}
    steps = [[n // 2], [n // 2], [0], [n - 1], [n // 2 - 1, n // 2], list(range(n)), [1 % n], list(range(n - 1, -1, -2))]
    for r, keys in enumerate(steps):
        keys = list(dict.fromkeys(keys))
        leaves = [K.le(100 * r + k + 1) for k in keys]
        want_inserted = sum(1 for k in keys if k not in held)
        inserted, evals = m.put(keys, leaves)
        held.update(zip(keys, leaves))
        assert inserted == want_inserted and evals == K.evals_of(keys, depth)
        same_as_brute(m, held, empty)
    before = m.root()
    m2 = K.KeyedModel(depth, empty)                         # a key held with the empty value: the nodes of the absent key, and the key is held
    m2.put([0], [empty])
    assert m2.root() == K.empty_chain(depth, empty)[depth] and m2.keys() == [0] and m2.get([0, n - 1]) == ([K.red(empty), K.red(empty)], [True, False])
    assert m.root() == before


def test_launch_rule_of_the_model():
    assert K.hashing_launches([0] * 5) == 0 and K.hashing_launches([256, 128, 1]) == 1 and K.hashing_launches([257, 129, 1]) == 2 and K.hashing_launches([600, 300, 150]) == 3


# ---------------------------------------------------------------------------------------------------------------- the put scenarios reach what they are for
# Conditions of the GPU tests (test_merkle_keyed_gpu.py), by integers alone: the seeds are chosen so that they hold.
def test_integer_models_agree():
    """put_lists (sets), put_lists_np and counts_np (numpy.unique) against counts_of and evals_of"""
    held, keys = K.rand_keys(b"models held", 900, 13), K.rand_keys(b"models put", 700, 13)
    lists = K.put_lists(held, keys, 13)
    assert lists == K.put_lists_np(held, keys, 13) and [m for m, _ in lists[1:]] == K.evals_of(keys, 13)
    after = K.counts_of(set(held) | set(keys), 13)
    assert K.counts_np(held + keys, 13) == after and [b + f for b, (_, f) in zip(K.counts_of(held, 13), lists)] == after
    assert K.classified([(5, 2), (4, 1), (3, 0), (2, 0), (1, 0)]) == [0, 1, 2] and K.classified([(5, 0), (3, 0), (1, 0)]) == [0] and K.classified([(2, 2), (1, 1)]) == [0]
    assert [K.capacity(0, 3, 8192), K.capacity(64, 65, 8192), K.capacity(3000, 4500, 8192), K.capacity(2462, 3295, 4096), K.capacity(6000, 5000, 8192), K.capacity(0, 3, 2)] == [64, 128, 6000, 4096, 6000, 3]


@pytest.mark.parametrize("last", ["new", "held"])
def test_scenario_tiles_mixed(last):
    sc = K.tiles_mixed(last)
    held, (keys, kind) = set(sc.base), sc.puts[0]
    assert sc.depth == 13 and len(held) == len(sc.base) == 3416 and len(keys) == 4097 == len(set(keys)) and list(keys) == sorted(keys) and max(keys) < 1 << 13
    assert K.kind_of(held, keys) == kind == "mixed"
    flags = K.put_flags(held, keys)
    # by scan tile: none, all, irregular, irregular, a tile of one flag
    assert K.tile_counts(flags) == [(1024, 0), (1024, 1024), (1024, 442), (1024, 461), (1, 1 if last == "new" else 0)]
    assert (flags[2047], flags[2048]) == (1, 0) and flags[3071] != flags[3072]
    for tile in (2, 3):                                                     # irregular: the flag changes hundreds of times inside the tile, and no run is long
        f = flags[tile * K.TILE:(tile + 1) * K.TILE]
        assert sum(a != b for a, b in zip(f, f[1:])) > 512 and "1" * 10 not in "".join(map(str, f)) and "0" * 10 not in "".join(map(str, f))
    assert K.tiles_mixed("new").base == K.tiles_mixed("held").base and K.tiles_mixed("new").puts[0][0][:4096] == K.tiles_mixed("held").puts[0][0][:4096]
    lists = K.put_lists(held, keys, 13)
    # height 0 has both kinds of flag; height 1 is the first without a brand-new position (every dirty pair holds a key), so from height 2 on classify == 0,
    # and the dirty list of height 2 is still longer than a tile
    assert 0 < lists[0][1] < lists[0][0] and K.classified(lists) == [0, 1]
    assert lists[1] == (2718, 0) and lists[2] == (1594, 0) and lists[2][0] > K.TILE
    assert [s for s, (m, _) in enumerate(lists) if m > K.TILE] == [0, 1, 2]


def test_scenario_in_place():
    sc = K.in_place()
    states = K.scenario_states(sc)
    assert sc.depth == 13 and [len(s) for s in states] == [3000, 4500, 5000] and [len(k) for k, _ in sc.puts] == [1500, 1000]
    assert [K.kind_of(states[r], keys) for r, (keys, _) in enumerate(sc.puts)] == [kind for _, kind in sc.puts] == ["new", "mixed"]
    assert sum(1 for k in sc.puts[1][0] if k in states[1]) == 500
    caps = K.capacities([0] * 14, K.counts_of(states[0], 13), 13)
    assert caps[:4] == [3000, 2462, 1729, 1003] and caps[4:] == [512 >> s for s in range(10)]
    # the 1,500 new keys: heights 0..3 outgrow their arrays (height 0 takes twice its room, the others all their height can hold), nothing above gains a node
    kinds, caps = K.merge_kinds(caps, K.counts_of(states[0], 13), K.counts_of(states[1], 13), 13)
    assert kinds == ["grows"] * 4 + [None] * 10 and caps[:4] == [6000, 4096, 2048, 1024]
    # the 1,000 mixed keys: heights 0, 1 and 2 gain positions and keep their arrays
    after = K.counts_of(states[2], 13)
    kinds, caps2 = K.merge_kinds(caps, K.counts_of(states[1], 13), after, 13)
    assert kinds == ["in place"] * 3 + [None] * 11 and caps2 == caps
    totals = [after[s] for s, kind in enumerate(kinds) if kind == "in place"]
    assert totals == [5000, 3511, 2014] and len(set(totals)) == len(totals) >= 3 and min(totals) > 256
    lists = K.put_lists(states[1], sc.puts[1][0], 13)                       # and the flags of that put are mixed at every one of them
    assert all(0 < lists[s][1] < lists[s][0] for s in range(3))


@pytest.mark.parametrize("last", ["new", "held"])
def test_scenario_second_trip(last):
    sc = K.second_trip(last)
    states = K.scenario_states(sc)
    (a, _), (b, _) = sc.puts
    assert sc.depth == 19 and len(states[0]) == 1 << 17 and len(a) == len(set(a)) == 262144 and len(b) == len(set(b)) == 262145 and max(a + b) < 1 << 19
    assert K.second_trip("new").base == K.second_trip("held").base and K.second_trip("new").puts[0] == K.second_trip("held").puts[0]
    cdiv = lambda x, y: -(-x // y)
    trips = lambda m: cdiv(cdiv(m, K.TILE), K.TOP_TILES)                    # trips of k_mkx_scan_top over the tile sums of a list of m flags
    for r, keys in enumerate((a, b)):
        held = sum(1 for k in keys if k in states[r])
        assert len(keys) // 4 < held < 3 * len(keys) // 4, (r, held)
        lists = K.put_lists_np(sorted(states[r]), keys, 19)
        if r == 0:
            assert [m for m, _ in lists[1:]] == K.evals_of(keys, 19)
        assert cdiv(lists[0][0], K.TILE) == (256, 257)[r]
        # a second trip needs a dirty list above 262,144: none of A's heights has one, and of B's height 0 alone (height 1 has 2^18 positions in all)
        assert [s for s, (m, _) in enumerate(lists) if m > K.TILE * K.TOP_TILES] == ([], [0])[r]
        assert [trips(m) for m, _ in lists[:2]] == ([1, 1], [2, 1])[r]
        assert all(0 < f < m for m, f in lists[:4]) and len(K.classified(lists)) >= 4         # mixed flags over many tiles at the lowest heights
        assert K.counts_np(sorted(states[r + 1]), 19) == [c + f for c, (_, f) in zip(K.counts_np(sorted(states[r]), 19), lists)]
    order = sorted(b)
    assert [k in states[1] for k in order[-2:]] == [False, last == "held"]   # the one flag of tile 256, and its neighbour at dirty index 262,143
    assert order[-1] >> 1 != order[-2] >> 1                                  # (the last key starts a parent of its own: head flag 1 in that tile)


# ---------------------------------------------------------------------------------------------------------------- the plan header on host arrays
@pytest.fixture(scope="module")
def plan_run(tmp_path_factory):
    """tests/hostcheck/merkle_keyed_plan.cpp through the host compiler under ASan and UBSan (a stand-alone program: no preload), run once"""
    exe = tmp_path_factory.mktemp("merkle_keyed_plan") / "merkle_keyed_plan"
    src = O.ROOT / "tests" / "hostcheck" / "merkle_keyed_plan.cpp"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=1800)


def test_index_rules_and_plan_against_brute_force(plan_run):
    """Depths 1..4: every subset of the keys with every split into "held before" and "put now" (3^(2^depth) splits), and at depths 1..3 every pair of
    subsets that overlap (the overlap is replaced).  Depths 12, 31 and 32: the keys 0, 1, 2^(depth-1) - 1, 2^(depth-1), 2^depth - 2, 2^depth - 1 key by
    key and at once, then seeded random batches of 1 to 1,500 keys.  The program exits 0 only when positions stay sorted and distinct, every old value
    survives a merge at its new place, every destination is written once, the dirty lists are exactly the proper ancestors, the plan has wide steps only
    above 256 parents with one climb, and every node reads as brute force says."""
    assert plan_run.returncode == 0 and plan_run.stderr == "", plan_run.stderr
    head = plan_run.stdout.split()
    assert head[0] == "keyed"
    assert int(head[1]) == sum(3 ** (1 << d) for d in range(1, 5))
    assert int(head[2]) == sum(4 ** (1 << d) - 3 ** (1 << d) for d in range(1, 4))
    assert int(head[3]) == 3 * (3 * 13 + 1)
    assert int(head[4]) > 0 and int(head[5]) > 0


def test_plan_header_has_no_hip():
    text = PLAN.read_text()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text
    for name in ("MERKLE_KEYED_MIN_CAPACITY", "merkle_keyed_capacity", "merkle_keyed_lower_bound", "merkle_keyed_find", "merkle_keyed_children", "merkle_keyed_old_dest",
                 "merkle_keyed_new_dest", "merkle_keyed_head", "plan_merkle_keyed_hash"):
        assert name in text, name
    kernels = (O.ROOT / "bulletproofs_gadgets_amd" / "csrc" / "hip" / "k_merkle_keyed.cuh").read_text()
    assert '#include "../host/merkle_keyed_plan.hpp"' in kernels
    assert '#include "k_merkle_keyed.cuh"' in (O.ROOT / "bulletproofs_gadgets_amd" / "csrc" / "hip" / "kernels.cuh").read_text()


# ---------------------------------------------------------------------------------------------------------------- the C calls
def test_header_declares_and_library_exports():
    text = (O.ROOT / "include" / "bpg.h").read_text()
    assert re.search(r"^#define BPG_ABI_VERSION 7u\b", text, re.M)
    lib = bpg.lib()
    for name in CALLS:
        assert re.search(r"^bpg_status %s\(bpg_ctx \*ctx, " % name, text, re.M), name
        assert getattr(lib, name) is not None
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout      # the library that is loaded
    for name in CALLS:
        assert re.search(r" T %s$" % name, out, re.M), name
    assert "keyed (non-prefix) sparse trees" not in text
    for phrase in ("removing keys", "keys wider than", "sorting incoming keys on the device", "hashing records into keys"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", text), phrase


def u64s(*v):
    return (C.c_uint64 * len(v))(*v)


def test_refusals_that_need_no_device():
    """The C calls check their arguments before they look at the context or the tree, so each bad argument is sent with handles that are not NULL and are
    never dereferenced (0x5a): the call returns 4 because of THAT argument, *out is cleared, and no output is written."""
    lib = bpg.lib()
    dummy, tree = C.c_void_p(0x5a), C.c_void_p(0x5a)
    two = bytes(64)
    bad_builds = [                                                          # (ctx, depth, count, keys, leaves, what)
        (None, 3, 1, u64s(1), bytes(32), "a NULL context"),
        (dummy, 0, 0, None, None, "depth 0"),
        (dummy, 33, 0, None, None, "depth 33"),
        (dummy, 3, 1, None, bytes(32), "NULL keys"),
        (dummy, 3, 1, u64s(1), None, "NULL leaves"),
        (dummy, 3, 2, u64s(1, 8), two, "a key of 2^depth"),
        (dummy, 32, 2, u64s(1, 1 << 32), two, "a key of 2^32"),
        (dummy, 3, 2, u64s(5, 5), two, "a key given twice"),
        (dummy, 32, 3, u64s(2**32 - 1, 0, 2**32 - 1), bytes(96), "the last key given twice"),
        (dummy, 32, (1 << 24) + 1, u64s(1), bytes(32), "more than 2^24 keys"),
        (dummy, 1, 3, u64s(0, 1, 0), bytes(96), "more keys than 2^depth"),
    ]
    for ctx, depth, count, keys, leaves, what in bad_builds:
        tree.value = 0x5a
        assert lib.bpg_merkle_build_keyed(ctx, C.c_uint32(depth), C.c_uint64(count), keys, leaves, None, C.byref(tree)) == 4, what
        assert not tree.value, what                                         # a refused call sets *out to NULL
    assert lib.bpg_merkle_build_keyed(dummy, C.c_uint32(3), C.c_uint64(1), u64s(1), bytes(32), None, None) == 4         # NULL out
    # the calls on a tree: nothing is read through the context or the tree, and nothing is written
    ins, root = C.c_uint64(0x5a5a), (C.c_char * 32)(*([0x5a] * 32))
    bad_puts = [(1, None, bytes(32), "NULL keys"), (1, u64s(1), None, "NULL leaves"), (2, u64s(7, 7), two, "a key given twice"), (2, u64s(0, 1 << 32), two, "a key of 2^32"),
                ((1 << 24) + 1, u64s(1), bytes(32), "more than 2^24 keys")]
    for count, keys, leaves, what in bad_puts:
        assert lib.bpg_merkle_put(dummy, dummy, C.c_uint64(count), keys, leaves, C.byref(ins), root) == 4, what
    assert lib.bpg_merkle_put(None, dummy, C.c_uint64(1), u64s(1), bytes(32), C.byref(ins), root) == 4                  # a NULL context, a NULL tree
    assert lib.bpg_merkle_put(dummy, None, C.c_uint64(1), u64s(1), bytes(32), C.byref(ins), root) == 4
    assert ins.value == 0x5a5a and root.raw == b"\x5a" * 32
    leaves_out, held_out, keys_out, counts, nbytes = (C.c_char * 32)(*([0x5a] * 32)), (C.c_char * 1)(0x5a), u64s(0x5a5a), u64s(*([0x5a5a] * 33)), C.c_uint64(0x5a5a)
    assert lib.bpg_merkle_get(dummy, dummy, C.c_uint64(1), None, leaves_out, held_out) == 4                            # NULL keys, NULL output
    assert lib.bpg_merkle_get(dummy, dummy, C.c_uint64(1), u64s(1), None, held_out) == 4
    assert lib.bpg_merkle_get(None, dummy, C.c_uint64(1), u64s(1), leaves_out, held_out) == 4
    assert lib.bpg_merkle_get(dummy, None, C.c_uint64(1), u64s(1), leaves_out, held_out) == 4
    assert lib.bpg_merkle_keys(dummy, dummy, C.c_uint64(0), C.c_uint64(1), None) == 4
    assert lib.bpg_merkle_keys(dummy, dummy, C.c_uint64(0), C.c_uint64((1 << 24) + 1), keys_out) == 4
    assert lib.bpg_merkle_keys(None, dummy, C.c_uint64(0), C.c_uint64(1), keys_out) == 4
    assert lib.bpg_merkle_keys(dummy, None, C.c_uint64(0), C.c_uint64(1), keys_out) == 4
    assert lib.bpg_merkle_node_counts(dummy, dummy, None, None) == 4                                                   # both outputs NULL
    assert lib.bpg_merkle_node_counts(None, dummy, counts, C.byref(nbytes)) == 4
    assert lib.bpg_merkle_node_counts(dummy, None, counts, C.byref(nbytes)) == 4
    assert leaves_out.raw == b"\x5a" * 32 and held_out.raw == b"\x5a" and keys_out[0] == 0x5a5a and list(counts) == [0x5a5a] * 33 and nbytes.value == 0x5a5a


def test_python_argument_rules():
    """the ValueErrors of Context.merkle_tree(keys=) are raised before any call into the library (no context is needed to see them)"""
    class NoContext:
        _h = None
    for kwargs in (dict(keys=[1]), dict(keys=[1], depth=3, reserve=2), dict(keys=[1, 2], depth=3), dict(keys=[], depth=3, reserve=1)):
        with pytest.raises(ValueError):
            bpg.MerkleTree(NoContext(), [bytes(32)] if kwargs["keys"] else [], **kwargs)
