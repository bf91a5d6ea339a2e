"""CPU tests of the growing Merkle tree (no GPU needed): the launch plan of csrc/host/merkle_plan.hpp replayed against brute force, the empty-subtree
constants from the host half of csrc/hip/k_mimc.cuh against the reference's tree of equal leaves, and what the four new C calls declare, export and
refuse before they touch a device."""
import ctypes as C
import re
import subprocess
import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O

CALLS = ("bpg_merkle_build_partial", "bpg_merkle_append", "bpg_merkle_size", "bpg_merkle_empty_nodes")


@pytest.fixture(scope="module")
def plan_run(golden, tmp_path_factory):
    """tests/hostcheck/merkle_plan.cpp through the host compiler under ASan and UBSan (a stand-alone program: no preload), run once"""
    m = golden["mimc"]
    exe = tmp_path_factory.mktemp("merkle_plan") / "merkle_plan"
    src = O.ROOT / "tests" / "hostcheck" / "merkle_plan.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    return subprocess.run([str(exe), m["leaf512_be"], str(len(m["levels512_be"]))], capture_output=True, text=True, timeout=300)


def test_plan_against_brute_force(plan_run):
    """every depth 1..7 with every 0 <= old <= new <= 2^depth, and depths 20 and 24 around every power of two: the program exits 0 only when every plan
    recomputes exactly the proper ancestors of the new leaves, each once, bottom-up, wide steps above 256 parents and climb levels at most 256"""
    assert plan_run.returncode == 0 and plan_run.stderr == "", plan_run.stderr
    head = plan_run.stdout.splitlines()[0].split()
    assert head[0] == "plan"
    small = sum(((1 << d) + 1) * ((1 << d) + 2) // 2 for d in range(1, 8))           # pairs old <= new of 2^d + 1 sizes
    big = 0
    for d in (20, 24):
        sizes = [0] + [v for k in range(d + 1) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= v <= 1 << d]      # as the program lists them
        big += sum(1 for o in sizes for n in sizes if n >= o)
    assert int(head[1]) == small + big
    assert int(head[2]) > 0


def test_empty_chain_is_the_reference_tree_of_equal_leaves(plan_run, golden):
    """a tree of equal leaves IS its empty-subtree chain: E_0 the leaf, E_k the reference's level k above it (merkle_tree_gadget.rs:476-503)"""
    m = golden["mimc"]
    assert plan_run.returncode == 0, plan_run.stderr
    lines = [l.split()[1] for l in plan_run.stdout.splitlines() if l.startswith("E ")]
    assert len(m["levels512_be"]) == 9
    assert lines == [m["leaf512_be"]] + m["levels512_be"]                                  # E_0 .. E_9


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


def test_refusals_that_need_no_device():
    """The C calls check their arguments before they look at the context, so each bad argument is sent with a context pointer that is not NULL and is
    never dereferenced (0x5a): the call returns 4 because of THAT argument.  Only the NULL-context case relies on the context check."""
    lib = bpg.lib()
    dummy = C.c_void_p(0x5a)                                                 # stands for a context (or a tree); a call that read through it would crash
    tree = C.c_void_p(0x5a)
    # build_partial: a refused call sets *out to NULL, as bpg_merkle_build does (and writes nothing through a NULL out)
    bad_builds = [
        (None, 1, 2, bytes(64), "a NULL context"),
        (dummy, 0, 0, None, "depth 0"),
        (dummy, 25, 1, bytes(32), "depth 25"),
        (dummy, 1, 3, bytes(96), "size > 2^depth"),
        (dummy, 24, (1 << 24) + 1, bytes(32), "size > 2^24"),
        (dummy, 1, 1, None, "NULL leaves with size 1"),
    ]
    for ctx, depth, size, leaves, what in bad_builds:
        tree.value = 0x5a
        assert lib.bpg_merkle_build_partial(ctx, C.c_uint32(depth), C.c_uint64(size), leaves, None, C.byref(tree)) == 4, what
        assert not tree.value, what
    assert lib.bpg_merkle_build_partial(dummy, C.c_uint32(1), C.c_uint64(2), bytes(64), bytes(32), None) == 4         # NULL out
    # the calls on a tree: nothing is read through the context or the tree, and nothing is written
    first, size, depth = C.c_uint64(0x5a5a), C.c_uint64(0x5a5a), C.c_uint32(0x5a5a)
    out = C.create_string_buffer(b"\x5a" * 64, 64)
    assert lib.bpg_merkle_append(dummy, dummy, C.c_uint64(1), None, C.byref(first), out) == 4      # NULL leaves with a count
    assert lib.bpg_merkle_size(dummy, dummy, None, None) == 4                                      # both outputs NULL
    assert lib.bpg_merkle_empty_nodes(dummy, dummy, None) == 4                                     # NULL out
    assert lib.bpg_merkle_append(None, dummy, C.c_uint64(1), bytes(32), C.byref(first), out) == 4  # a NULL context, a NULL tree
    assert lib.bpg_merkle_append(dummy, None, C.c_uint64(0), None, C.byref(first), out) == 4
    assert lib.bpg_merkle_size(None, dummy, C.byref(size), C.byref(depth)) == 4
    assert lib.bpg_merkle_size(dummy, None, C.byref(size), C.byref(depth)) == 4
    assert lib.bpg_merkle_empty_nodes(None, dummy, out) == 4
    assert lib.bpg_merkle_empty_nodes(dummy, None, out) == 4
    assert first.value == size.value == depth.value == 0x5a5a and out.raw == b"\x5a" * 64
