"""CPU tests of the prefix layout of the Merkle tree (no GPU needed): csrc/host/merkle_prefix_plan.hpp - the dimensions, the index rules the kernels of
csrc/hip/k_merkle_prefix.cuh run, and the launch plan - replayed on a host model against brute force, and what the three new C calls declare, export
and refuse before they touch a device."""
import ctypes as C
import re
import subprocess
import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O

CALLS = ("bpg_merkle_build_prefix", "bpg_merkle_reserve", "bpg_merkle_reserved")


@pytest.fixture(scope="module")
def plan_run(tmp_path_factory):
    """tests/hostcheck/merkle_prefix_plan.cpp through the host compiler under ASan and UBSan (a stand-alone program: no preload), run once"""
    exe = tmp_path_factory.mktemp("merkle_prefix_plan") / "merkle_prefix_plan"
    src = O.ROOT / "tests" / "hostcheck" / "merkle_prefix_plan.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)


def test_layout_and_plan_against_brute_force(plan_run):
    """Every depth 1..6 with every reserve and every 0 <= old <= new <= reserve on a model of the layout with values; depth 12 with wide steps; depths 25,
    31 and 32 at reserves 1, 5, 2^20, 2^20 + 1, 2^24 - 1 and 2^24 with intervals that start off zero.  The program exits 0 only when the offsets tile the
    buffer, every read hits a stored slot or is a fallback, every plan computes exactly the proper ancestors of the new leaves once each (wide steps above
    256 parents, climb levels at most 256, `evals` the size of the set), every node reads as brute force says, and relayout preserves every stored value."""
    assert plan_run.returncode == 0 and plan_run.stderr == "", plan_run.stderr
    head = plan_run.stdout.split()
    assert head[0] == "prefix"
    # (reserve, new, old) with max(new, 1) <= reserve <= 2^d and old <= new, as the program walks them; three more at depth 12
    small = sum(((1 << d) - max(n, 1) + 1) * (n + 1) for d in range(1, 7) for n in range((1 << d) + 1))
    assert int(head[1]) == small + 3
    assert int(head[2]) > 0 and int(head[3]) > 0
    big = 0
    for d in (25, 31, 32):
        for r in (1, 5, 1 << 20, (1 << 20) + 1, (1 << 24) - 1, 1 << 24):
            sizes = [0] + [v for k in range(25) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= v <= r] + [r, r - r // 3, r // 2]
            big += sum(1 for o in sizes for n in sizes if n >= o)
    assert int(head[4]) == big


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
    never dereferenced (0x5a): the call returns 4 because of THAT argument.  Only the NULL-context and NULL-tree cases rely on the handle checks."""
    lib = bpg.lib()
    dummy = C.c_void_p(0x5a)                                                 # stands for a context (or a tree); a call that read through it would crash
    tree = C.c_void_p(0x5a)
    bad_builds = [                                                           # (ctx, depth, reserve, size, leaves, what)
        (None, 3, 2, 1, bytes(32), "a NULL context"),
        (dummy, 0, 1, 0, None, "depth 0"),
        (dummy, 33, 1, 0, None, "depth 33"),
        (dummy, 3, 0, 0, None, "reserve 0"),
        (dummy, 3, 9, 1, bytes(32), "reserve > 2^depth"),
        (dummy, 32, (1 << 24) + 1, 1, bytes(32), "reserve > 2^24"),
        (dummy, 25, (1 << 24) + 1, 1, bytes(32), "reserve > 2^24 at depth 25"),
        (dummy, 3, 2, 3, bytes(96), "size > reserve"),
        (dummy, 3, 2, 1, None, "NULL leaves with size 1"),
    ]
    for ctx, depth, reserve, size, leaves, what in bad_builds:
        tree.value = 0x5a
        assert lib.bpg_merkle_build_prefix(ctx, C.c_uint32(depth), C.c_uint64(reserve), C.c_uint64(size), leaves, None, C.byref(tree)) == 4, what
        assert not tree.value, what                                          # a refused call sets *out to NULL
    assert lib.bpg_merkle_build_prefix(dummy, C.c_uint32(3), C.c_uint64(2), C.c_uint64(1), bytes(32), bytes(32), None) == 4     # NULL out
    # the calls on a tree: nothing is read through the context or the tree, and nothing is written
    r, b = C.c_uint64(0x5a5a), C.c_uint64(0x5a5a)
    assert lib.bpg_merkle_reserve(dummy, dummy, C.c_uint64((1 << 24) + 1)) == 4                    # beyond 2^24 whatever the tree
    assert lib.bpg_merkle_reserved(dummy, dummy, None, None) == 4                                  # both outputs NULL
    assert lib.bpg_merkle_reserve(None, dummy, C.c_uint64(1)) == 4                                 # a NULL context, a NULL tree
    assert lib.bpg_merkle_reserve(dummy, None, C.c_uint64(1)) == 4
    assert lib.bpg_merkle_reserved(None, dummy, C.byref(r), C.byref(b)) == 4
    assert lib.bpg_merkle_reserved(dummy, None, C.byref(r), C.byref(b)) == 4
    assert r.value == b.value == 0x5a5a
