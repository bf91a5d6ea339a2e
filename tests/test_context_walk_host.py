"""The walk harness of tests/context_walk.py without a GPU: that the walks cover what they claim to cover, that every expectation stands on the CPU
references alone, and that the harness can fail - it passes on a model context whose operations return the expectations, and catches three broken models
at the step where each first lies."""
import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import context_walk as W
from test_context_walk_gpu import WALK_SEEDS

L = bpg.L
ALL_OPS = [o for f in W.FAMILIES for o in W.CATALOGUE[f]]


@pytest.fixture(scope="module")
def walks():
    return {seed: W.build_walk(seed) for seed in WALK_SEEDS}


def model_factory(world, cls=W.ModelContext):
    return lambda: cls(world)


# ------------------------------------------------------------------------------------------------ coverage and lifetimes
def test_the_catalogue_has_seventeen_families_of_two_to_four_variants():
    assert len(W.FAMILIES) == 17 and len(set(W.FAMILIES)) == 17
    assert W.FAMILIES[13:] == ["merkle_grow", "gates", "verify_wave", "merkle_keyed"] and [o.variant for o in W.CATALOGUE["merkle_keyed"]] == ["rebuild", "refuse", "read"]
    assert [o.variant for o in W.CATALOGUE["repeat_join_check"]][-1] == "repeat_inputs"
    for f in W.FAMILIES:
        assert 2 <= len(W.CATALOGUE[f]) <= 4, f
    assert len({o.name for o in ALL_OPS}) == len(ALL_OPS)


@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_every_ordered_pair_of_families_is_adjacent(walks, seed):
    steps = walks[seed]
    assert len(steps) == 17 * 17 + 1 == 290 and steps[0][0] == steps[-1][0]
    pairs = {(a[0], b[0]) for a, b in zip(steps, steps[1:])}
    assert pairs == {(f, g) for f in W.FAMILIES for g in W.FAMILIES}            # 289 pairs on 289 edges: each exactly once, a family after itself included
    assert {"%s/%s" % s for s in steps} == set(W.OPS), "every variant of every family occurs"
    assert sum(s == ("lifecycle", "grow") for s in steps) <= W.MAX_GROWS
    assert steps == W.build_walk(seed), "a walk is a function of its seed"


def test_the_walks_differ():
    assert len({tuple(W.build_walk(s)) for s in WALK_SEEDS}) == len(WALK_SEEDS) == 3


def test_pinned_orders_name_operations_and_say_why():
    assert len(W.PINNED) >= 19 and len(W.PINNED_TWO) >= 1
    for reason, names in W.PINNED + W.PINNED_TWO:
        assert reason and all(n in W.OPS for n in names), (reason, names)
    assert ["prove_tabled", "prove_folded", "prove_tabled", "prove_folded"] in [[n.split("/")[0] for n in names] for _, names in W.PINNED]


def pinned(word):
    found = [names for reason, names in W.PINNED if word in reason]
    assert len(found) == 1, word
    return found[0]


def test_pinned_orders_do_what_their_reasons_say():
    """read off the operations' own declarations (uses, uploads), not off their names"""
    # the circuit is uploaded by step 0, the generators grow in step 1, and nothing touches the new handle before step 2 proves on it
    assert ("mimc", 0, 1, 2) in W.first_used_after_a_grow(pinned("between an upload and its first proof"))
    late = W.first_used_after_a_grow(pinned("first use of anything in the resident set"))
    assert {(name, up, grew) for name, up, grew, _ in late} == {(n, -1, 0) for n in ("mimc", "rp40", "t_b64", "tree")}
    # the same small circuit on both sides of a folded proof: its tables of the original generators are there to be found again
    names = pinned("tables of the original generators")
    assert names[0] == names[2] == "prove_tabled/rp40" and W.OPS[names[1]].family == "prove_folded"
    # check() on the circuit that the proofs on both sides of it are of
    names = pinned("row view")
    assert names[0] == names[2] and set(W.OPS[names[0]].uses) <= set(W.OPS[names[1]].uses) and W.OPS[names[1]].variant == "check"
    names = pinned("freed and uploaded again")
    up, after = W.OPS[names[0]], W.OPS[names[1]]
    assert up.uploads and not set(up.uploads) & set(after.uses) and list(W.RESIDENT).index(after.uses[0]) < list(W.RESIDENT).index(up.uploads[0])
    # the growing tree and the gated template are first touched after the grow of step 0, neither by a step that uploads it
    late = W.first_used_after_a_grow(pinned("tables swapped under a growing tree"))
    assert late == [("gtree", -1, 0, 1), ("t_hand", -1, 0, 2)]
    # the tree that the relayout gave a new buffer is read again, not rebuilt, behind the folded proof
    names = pinned("relayout")
    assert W.OPS[names[0]].uploads == ("gtree",) and W.OPS[names[1]].family == "prove_folded" and W.OPS[names[2]].uses == ("gtree",) and not W.OPS[names[2]].uploads
    # two different trees, neither uploaded again, in alternation
    names = pinned("staging buffers")
    assert [W.OPS[n].uses for n in names] == [("tree",), ("gtree",), ("tree",)] and not any(W.OPS[n].uploads for n in names)
    # the same template on all three steps, the proving wave in the middle
    names = pinned("standing slots")
    assert names[0] == names[2] and {W.OPS[n].uses for n in names} == {("t_lt",)} and W.OPS[names[1]].family == "template_ck_inputs"
    names = pinned("lv / rv")
    assert [W.OPS[n].family for n in names] == ["prove_folded", "verify_wave", "prove_folded"] and names[0] != names[2]
    names = pinned("coefficient class 3")
    assert [W.OPS[n].uses for n in names] == [("t_hand",), (), ("t_hand",)] and W.OPS[names[1]].family == "lockstep"
    # the keyed rebuild directly after the prefix rebuild, and directly before it; both trees are then read, not rebuilt
    names = pinned("behind a prefix rebuild")
    assert names[:2] == ["merkle_grow/prefix", "merkle_keyed/rebuild"] and [W.OPS[n].uploads for n in names[2:]] == [(), ()] and {W.OPS[n].uses for n in names[2:]} == {("gtree",), ("ktree",)}
    names = pinned("ahead of a prefix rebuild")
    assert names[:2] == ["merkle_keyed/rebuild", "merkle_grow/prefix"] and [W.OPS[n].uploads for n in names[2:]] == [(), ()] and {W.OPS[n].uses for n in names[2:]} == {("gtree",), ("ktree",)}
    # the refusals, the tree read behind them, then a proving family
    names = pinned("a refused update")
    assert names[:2] == ["merkle_keyed/refuse", "merkle_keyed/read"] and W.OPS[names[2]].family == "prove_folded" and not W.OPS[names[0]].uploads
    names = pinned("sized by a rebuild")
    assert [W.OPS[n].uses for n in names] == [("ktree",), ("tree",), ("ktree",), ("ktree",)]
    # two contexts: the rebuild (an odd step) is the second context's, and the first context reads its own tree before and after it
    (reason, names), = W.PINNED_TWO
    first, second = names[0::2], names[1::2]
    assert second[0] == "merkle_keyed/rebuild" and first[0] == first[1] == "merkle_keyed/read" and "merkle_keyed/rebuild" not in first[:3]
    assert "merkle_keyed/read" in second[1:] and W.OPS[second[0]].uploads == ("ktree",)


def test_the_keyed_tree_model_is_the_padded_tree():
    """the final state of the keyed tree against brute force over the 2^11 padded leaves (the oracle's sponge); what the steps of a rebuild are for, by
    integers: the second step makes the leaves outgrow the minimum capacity, the third fits the room that made and has both kinds of key"""
    K, D = W.KC, W.KEYED_DEPTH
    steps = W.keyed_steps()
    held = {}
    for step in steps:
        held.update(step)
    m = W.keyed_model()
    want = K.brute_levels(D, held, W.KEYED_EMPTY)
    assert all(m.level(level) == want[level] for level in range(D + 1)) and m.keys() == sorted(held) and m.counts() == K.counts_of(held, D)
    m.check_invariant()
    sizes, kinds, now = [], [], set()
    for step in steps:
        keys = [k for k, _ in step]
        assert len(set(keys)) == len(keys)
        kinds.append(K.kind_of(now, keys))
        now |= set(keys)
        sizes.append(len(now))
    assert sizes == [7, 107, 122, 122] and kinds == ["new", "new", "mixed", "held"] and [k for k, _ in steps[0]] != sorted(k for k, _ in steps[0])
    assert sizes[0] < K.MIN_CAPACITY < sizes[1] and sizes[2] <= 2 * K.MIN_CAPACITY
    got = W.keyed_model_read()
    assert got[0] == 122 and got[1] == want[0][0] and got[3] == sorted(held)
    assert got[4] == ([want[D][i] for i in W.KEYED_PROBE], [i in held for i in W.KEYED_PROBE]) and {0, 2**D - 1} <= set(W.KEYED_PROBE)
    assert got[5] == [[want[D - s][(i >> s) ^ 1] for s in range(D)] for i in W.KEYED_PROBE]
    assert got[6] == [[want[D - s][i >> s] for s in range(1, D + 1)] for i in W.KEYED_PROBE]
    assert got[8] == [want[level] for level in W.KEYED_LEVELS]
    level7 = [p in {k >> 4 for k in held} for p in range(128)]
    assert any(level7) and not all(level7)                                   # a whole level with stored nodes and empty subtrees


def test_the_sparse_tree_model_is_the_padded_tree():
    """the model of the growing tree against brute force: the full tree over the leaves padded with the empty value to 2^11, every node by the oracle's
    sponge; the states the appends pass through and the final one; and the reserve formula on the example of csrc/host/merkle_prefix_plan.hpp"""
    D = W.GROW_DEPTH
    for size, updated in ((W.GROW_SIZES[1], False), (W.GROW_SIZES[2], False), (W.GROW_SIZES[2], True)):
        m = W.grow_model(size, updated)
        levels = [m.heights[0] + [W.GROW_EMPTY] * ((1 << D) - size)]
        while len(levels[-1]) > 1:
            lo = levels[-1]
            levels.append([O.mimc_sponge(lo[i] + lo[i + 1]) for i in range(0, len(lo), 2)])
        assert all(m.node(s, j) == levels[s][j] for s in range(D + 1) for j in range(1 << (D - s))), (size, updated)
        assert W.grow_empty_chain()[:D] == [levels[s][-1] for s in range(D)]         # the rightmost subtree of every height below the root holds no leaf
        got = m.read()
        assert got[0] == size and got[1] == levels[D][0]
        assert got[3] == [[levels[k][(i >> k) ^ 1] for k in range(D)] for i in W.GROW_PATHS]
        assert got[4] == [[levels[k + 1][i >> (k + 1)] for k in range(D)] for i in W.GROW_PATHS] and all(p[-1] == levels[D][0] for p in got[4])
        assert got[5] == [levels[D - level] for level in W.GROW_LEVELS]
    final, before = W.grow_model(606, True), W.grow_model(606, False)
    assert [final.heights[0][i] != before.heights[0][i] for i in W.GROW_UPDATE] == [True] * 4 and final.root() != before.root()
    assert len({W.grow_model(6, False).root(), before.root(), final.root(), W.grow_empty_chain()[D]}) == 4
    # W_s of reserve 7 at depth 11: 7, 4, 2, 1 and eight times 1 = 22 slots, + 12 constants; of 606: 606, 303 (odd: the edge), 152, 76, 38, 19, 10, 5, 3, 2, 1, 1
    assert W.prefix_bytes(7) == 32 * (22 + 12) and W.prefix_bytes(606) == 32 * (1216 + 12)
    assert W.GROW_RESERVE < W.GROW_SIZES[2] == max(2 * W.GROW_RESERVE, W.GROW_SIZES[2]) and W.GROW_SIZES[1] <= W.GROW_RESERVE


def test_no_expectation_reads_a_context():
    """prepare() of every operation names neither the walk's environment nor a context"""
    import inspect
    for o in ALL_OPS:
        src = inspect.getsource(o._prepare)
        assert "env." not in src and "ctx." not in src and "env)" not in src, o.name


@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_uploads_whose_first_use_follows_a_grow(walks, seed):
    """the committed walks hold that interaction too, by chance of their seeds, on one context and on one of two at least; the pinned orders hold it by design"""
    names = [W._name(s) for s in walks[seed]]
    assert W.first_used_after_a_grow(names), "no resident object of this walk is first used after a grow that followed its upload"
    assert W.first_used_after_a_grow(names[0::2]) + W.first_used_after_a_grow(names[1::2]), "nor on either of two contexts"


class Watching(W.ModelContext):
    """records every handle a step touched"""
    touched = None

    def model_execute(self, op, env):
        for name in op.uses:
            self.touched.append((op.name, env.res[name], env.res[name].freed))
        return super().model_execute(op, env)


@pytest.mark.parametrize("contexts", [1, 2])
@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_no_step_uses_a_freed_handle(walks, seed, contexts):
    world = W.ModelWorld()
    made = []

    def factory():
        c = Watching(world); c.touched = []
        made.append(c)
        return c
    W.run_walk(factory, walks[seed], contexts=contexts, census=world.census)
    assert len(made) == contexts and world.buffers == 0
    for c in made:
        assert c.touched and not any(freed for _, _, freed in c.touched)
        assert all(h.frees == 1 for h in c.handles), "every handle a walk makes is freed exactly once"
        assert len(c.handles) > len(W.RESIDENT), "free + upload happened"
        assert c.capacity <= W.START_CAPACITY << W.MAX_GROWS


# ------------------------------------------------------------------------------------------------ expectations stand on the reference alone
@pytest.mark.parametrize("o", ALL_OPS, ids=lambda o: o.name)
def test_expectations_stand_on_the_oracle(o):
    exp = o.prepare()
    assert o.prepare() is exp                                   # computed once
    for case, proof, status in exp.claims:
        got = case.verify(proof)                                # O.verify on the verifier-side circuit (the replayed assembly where one is known)
        assert got == status and (status == 0 or status in (O.ERR_FORMAT, O.ERR_VERIFY)), (o.name, status, got)
        # a second witness for the status, which for the mangled proofs was the oracle's own verdict: the product's host replay (no device) decides every
        # format error by itself and leaves the rest to the device, whose only other verdict is VERIFICATION_ERROR
        side = case.vinst or case.inst
        replayed, decided = bpg.test_verify_replay(side.n, side.m, case.N, case.vstate, proof, bytes(32))
        if status == 0:
            assert not decided, o.name
        else:
            assert (decided and replayed == status) or (not decided and status == O.ERR_VERIFY), (o.name, status, replayed, decided)
    for inst, v, report in exp.checks:
        assert report == direct_check(inst, v), o.name


def test_the_catalogue_holds_good_and_bad_proofs_and_reports():
    claims = [c for o in ALL_OPS for c in o.prepare().claims]
    checks = [c for o in ALL_OPS for c in o.prepare().checks]
    assert sum(s == 0 for _, _, s in claims) >= 133 and sum(s != 0 for _, _, s in claims) >= 32
    assert {s for _, _, s in claims} == {0, O.ERR_FORMAT, O.ERR_VERIFY}
    assert any(r.ok for _, _, r in checks) and any(not r.ok for _, _, r in checks)


def direct_check(inst, v, max_rows=16):
    """the definition of the R1CS check in Python integers: a_L * a_R = a_O per multiplier, every row's linear combination = 0"""
    sv = lambda b: [int.from_bytes(b[32 * i:32 * i + 32], "little") % L for i in range(len(b) // 32)]
    vals = [sv(inst.aL), sv(inst.aR), sv(inst.aO), sv(v), [1]]
    coef = sv(inst.coef)
    bad_mul = [i for i in range(inst.n) if vals[0][i] * vals[1][i] % L != vals[2][i]]
    bad_rows = []
    for r in range(inst.q):
        total = 0
        for t in range(int(inst.row_ptr[r]), int(inst.row_ptr[r + 1])):
            var = int(inst.term_var[t])
            kind, index = var >> 29, var & 0x1fffffff
            total += coef[int(inst.term_coef[t])] * vals[kind][index if kind < 4 else 0]
        if total % L:
            bad_rows.append(r)
    view = bpg.CheckReportView(len(bad_mul), bad_mul[0] if bad_mul else 2**64 - 1, len(bad_rows), bad_rows[0] if bad_rows else 2**64 - 1)
    return bpg.CheckReport(view, bad_rows[:max_rows])


# ------------------------------------------------------------------------------------------------ the harness can fail
def all_walks(walks):
    return [(("walk %d" % seed), steps) for seed, steps in walks.items()] + [(reason, names) for reason, names in W.PINNED + W.PINNED_TWO]


def test_the_model_context_passes_every_walk(walks):
    for _, steps in all_walks(walks):
        for contexts in (1, 2):
            world = W.ModelWorld()
            W.run_walk(model_factory(world), steps, contexts=contexts, census=world.census)
            assert world.buffers == 0


class Stale(W.ModelContext):
    """returns the previous result of the same family"""
    def __init__(self, world):
        super().__init__(world)
        self.last = {}

    def model_execute(self, op, env):
        true = self.truth(op, env)
        out = self.last.get(op.family, true)
        self.last[op.family] = true
        return out


class WrongAfterRefusal(W.ModelContext):
    """one byte of the result changed in the step after any refusal"""
    def __init__(self, world):
        super().__init__(world)
        self.refused = False

    def model_execute(self, op, env):
        true = self.truth(op, env)
        out = corrupt(true) if self.refused else true
        self.refused = op.family == "refusal"
        return out


class Leaky(W.ModelContext):
    """one buffer is still alive after close"""
    def close(self):
        super().close()
        self.world.buffers += 1


def corrupt(x):
    """x with the first byte string (or, failing that, the first number) in it changed by one bit"""
    done = [False]

    def walk(v, want_bytes):
        if done[0]:
            return v
        if isinstance(v, bytes) and v and want_bytes:
            done[0] = True
            return bytes([v[0] ^ 1]) + v[1:]
        if isinstance(v, int) and not isinstance(v, bool) and not want_bytes:
            done[0] = True
            return v ^ 1
        if isinstance(v, (list, tuple)):
            return type(v)(walk(y, want_bytes) for y in v)
        return v
    out = walk(x, True)
    return out if done[0] else walk(x, False)


def first_stale_lie(names):
    last = {}
    for i, n in enumerate(names):
        o = W.OPS[n]
        want = o.prepare().want
        if o.family in last and last[o.family] != want:
            return i
        last[o.family] = want
    return None


def first_step_after_a_refusal(names):
    for i in range(1, len(names)):
        if W.OPS[names[i - 1]].family == "refusal":
            return i
    return None


@pytest.mark.parametrize("broken,where", [(Stale, first_stale_lie), (WrongAfterRefusal, first_step_after_a_refusal), (Leaky, len)])
def test_broken_models_are_caught_where_they_first_lie(walks, broken, where):
    caught = 0
    for label, steps in all_walks(walks):
        names = [W._name(s) for s in steps]
        at = where(names)
        world = W.ModelWorld()
        if at is None:                                          # (a short pinned order in which this model never lies)
            W.run_walk(model_factory(world, broken), steps, census=world.census)
            continue
        with pytest.raises(W.WalkMismatch) as e:
            W.run_walk(model_factory(world, broken), steps, census=world.census)
        assert e.value.index == at, (label, broken.__name__, e.value.index, at)
        assert e.value.steps == names[:at + 1] and "replay(" in str(e.value)
        assert e.value.op == (names[at] if at < len(names) else "close")
        caught += 1
    assert caught >= len(WALK_SEEDS), "every Eulerian walk catches every broken model"


def test_corrupt_changes_what_it_is_given():
    for o in ALL_OPS:
        want = o.prepare().want
        assert corrupt(want) != want, o.name
