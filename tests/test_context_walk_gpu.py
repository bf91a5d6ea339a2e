"""One context walked through every family of entry points in many orders, byte-exact (tests/context_walk.py): three Eulerian walks of 290 steps - every
one of the seventeen families of operations after every family, itself included - and the nineteen pinned short orders, under four context profiles, and the
pinned order for two contexts.  Every step's result is compared with
an expectation computed on the CPU before the context existed; at the end the census of device buffers, pinned buffers, streams and events is what it was.

Profiles (environment knobs a context reads when it is created):
    default            none: N <= 2^14 is table-driven from round 0
    full_size_paths    BPG_TT_ORIG_LG=6, BPG_TT_LG=4: N <= 64 keeps tables of the original generators; N = 128 and N = 1024 take what 2^20 takes - bucket-method
                       A_I / A_O / S, equal-scalar merging, grouped folds, tables of folded generators in the arena
    merge_every_proof  full_size_paths and BPG_MERGE=2: equal scalars grouped afresh in every proof
    two_contexts       default knobs; the steps dealt alternately to two contexts of device 0, which share generator tables and the table budget"""
import pytest
import context_walk as W

pytestmark = pytest.mark.gpu

WALK_SEEDS = [20240611, 7, 31337]
FULL = {"BPG_TT_ORIG_LG": "6", "BPG_TT_LG": "4"}
PROFILES = {
    "default": ({}, 1),
    "full_size_paths": (FULL, 1),
    "merge_every_proof": (dict(FULL, BPG_MERGE="2"), 1),
    "two_contexts": ({}, 2),
}


def make_context():
    import bulletproofs_gadgets_amd as bpg
    return bpg.Context(0)


@pytest.fixture(scope="module")
def walks():
    return {seed: W.build_walk(seed) for seed in WALK_SEEDS}


def walk_under(monkeypatch, profile, steps):
    """-> what the contexts' schedules said after the steps: {knob: the values seen}"""
    env, contexts = PROFILES[profile]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seen = {}

    def observe(e, index, name):
        for k, v in e.ctx.schedule().items():
            seen.setdefault(k, set()).add(v)
    W.run_walk(make_context, steps, contexts=contexts, observe=observe)
    return seen


@pytest.mark.parametrize("profile", list(PROFILES))
@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_eulerian_walk(walks, monkeypatch, seed, profile):
    seen = walk_under(monkeypatch, profile, walks[seed])
    # the profile is what the contexts ran under, and the paths it is there for were taken
    if profile in ("default", "two_contexts"):
        assert seen["tt_orig_lg"] == {14} and max(seen["merged_skipped_last"]) == 0, seen
    else:
        assert seen["tt_orig_lg"] == {6} and seen["tt_lg"] == {4} and seen["merge_equal"] == {2 if profile == "merge_every_proof" else 1}, seen
        assert max(seen["merged_skipped_last"]) > 0, "no proof of the walk took the bucket-method path with equal scalars merged"


@pytest.mark.parametrize("profile", ["default", "full_size_paths"])
def test_pinned_orders(monkeypatch, profile):
    for reason, names in W.PINNED:
        try:
            seen = walk_under(monkeypatch, profile, names)
        except W.WalkMismatch as e:
            raise AssertionError("pinned order (%s): %s" % (reason, e)) from e
        if profile == "default":
            assert seen["tt_orig_lg"] == {14} and seen["merge_equal"] == {1}, (reason, seen)
        else:
            assert seen["tt_orig_lg"] == {6} and seen["tt_lg"] == {4} and seen["merge_equal"] == {1}, (reason, seen)


def test_pinned_orders_on_two_contexts():
    for reason, names in W.PINNED_TWO:
        try:
            W.run_walk(make_context, names, contexts=2)
        except W.WalkMismatch as e:
            raise AssertionError("pinned order for two contexts (%s): %s" % (reason, e)) from e


def test_original_tables_are_found_again_after_a_folded_proof(monkeypatch):
    """The first pinned order under full_size_paths, with the launches of k_tt_multiples (the kernel that fills window tables) counted after every step:
    the N = 64 proof builds the tables of its original generators, the N = 1024 proof builds tables of folded generators in the arena, and the second
    N = 64 proof builds nothing - it finds its tables where they were."""
    for k, v in FULL.items():
        monkeypatch.setenv(k, v)
    names = W.PINNED[0][1]
    assert [n.split("/")[0] for n in names] == ["prove_tabled", "prove_folded", "prove_tabled", "prove_folded"] and names[0] == names[2]
    built = []

    def observe(e, index, name):
        if index < 0:
            e.ctx.profile_set(2)
        else:
            built.append(e.ctx.profile_report().get("k_tt_multiples", {"count": 0})["count"])
    W.run_walk(make_context, names, observe=observe)
    assert built[0] >= 1 and built[1] > built[0] and built[2] == built[1] and built[3] > built[2], built
