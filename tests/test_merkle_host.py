"""CPU tests of the MiMC sponge behind the Merkle-tree calls (no GPU needed): bpg_mimc_sponge against the oracle, the Python reference and the
reference's own known answers, and the device's permutation and node function (csrc/hip/k_mimc.cuh) compiled for the host."""
import ctypes as C
import pathlib
import subprocess
import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import pyref as R

H = bytes.fromhex
le = lambda x: x.to_bytes(32, "little")
be = lambda b: bytes(reversed(b)).hex()
EDGES = [0, 1, R.L - 1, 2**256 - 1]          # the last one is unreduced: the sponge takes a block mod l


@pytest.fixture(scope="module")
def consts():
    return [int.from_bytes(H(l), "little") for l in (O.ROOT / "tests/golden/mimc_rc769.hex").read_text().split()]


def test_sponge_matches_oracle_and_pyref(consts):
    import hashlib
    rnd = [int.from_bytes(hashlib.sha256(b"merkle-host-%d" % i).digest(), "little") for i in range(6)]
    cases = [[e] for e in EDGES]                                                          # one block
    cases += [[a, b] for a in EDGES for b in (0, R.L - 1, 2**256 - 1)]                    # two blocks: a node
    cases += [[rnd[0], rnd[1]], [rnd[2] % R.L, rnd[3] % R.L]]
    cases += [[EDGES[i], rnd[i], EDGES[(i + 1) % 4]] for i in range(4)] + [rnd[3:6]]      # three blocks
    for blocks in cases:
        data = b"".join(le(b) for b in blocks)
        got = bpg.mimc_sponge(data)
        assert got == O.mimc_sponge(data), blocks
        assert got == le(R.mimc_sponge([b % R.L for b in blocks], consts)), blocks
        assert got == bpg.mimc_sponge([le(b) for b in blocks])                            # a list of blocks is the same call
        assert int.from_bytes(got, "little") < R.L


def test_sponge_reference_known_answers(golden):
    m = golden["mimc"]
    john, doe = bytes(reversed(H(m["john_be"]))), bytes(reversed(H(m["doe_be"])))
    n1, n2 = bpg.mimc_sponge(john + john), bpg.mimc_sponge(doe + doe)
    assert be(n1) == m["node_john"] and be(n2) == m["node_doe"]                           # reference tests/resources/merkle_tree.inst:1,3
    assert be(bpg.mimc_sponge(n1 + n2)) == "0b33a0e69996bf60542d94951136e4246b15591e3e47d7aeb1a7822ee96101c8"     # :5
    # the three KATs: pad on the host (mimc.rs:77-97), then the sponge - what bpg_mimc_hash does in one call
    for k in ("kat1", "kat2", "kat3"):
        pre = H(m[k + "_in"])
        blocks = [int.from_bytes(s, "little") for s in bpg.be_to_scalars(pre)]
        padded = b"".join(le(b) for b in R.mimc_pad(blocks))
        assert be(bpg.mimc_sponge(padded)) == m[k + "_be"]
        assert bpg.mimc_sponge(padded) == bpg.mimc_hash(pre)
    h = bytes(reversed(H(m["leaf512_be"])))
    for want in m["levels512_be"]:
        h = bpg.mimc_sponge(h + h)
        assert be(h) == want


def test_device_node_function_compiles_for_the_host(golden, tmp_path):
    """tests/hostcheck/merkle_chain.cpp: mimc_permute and mimc_node of k_mimc.cuh through the host compiler, under ASan and UBSan (a stand-alone
    program: no preload), on the reference's tree of 512 equal leaves."""
    m = golden["mimc"]
    exe = tmp_path / "merkle_chain"
    src = O.ROOT / "tests" / "hostcheck" / "merkle_chain.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe), m["leaf512_be"], str(len(m["levels512_be"]))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.split() == m["levels512_be"]


def test_sponge_argument_checks():
    lib = bpg.lib()
    out = C.create_string_buffer(b"\x5a" * 32, 32)
    assert lib.bpg_mimc_sponge(bytes(32), C.c_uint64(0), out) == 4            # no blocks
    assert lib.bpg_mimc_sponge(None, C.c_uint64(1), out) == 4
    assert lib.bpg_mimc_sponge(bytes(32), C.c_uint64(1), None) == 4
    assert out.raw == b"\x5a" * 32
    with pytest.raises(bpg.BpgError) as e:
        bpg.mimc_sponge(b"")
    assert e.value.status == 4
    with pytest.raises(ValueError):
        bpg.mimc_sponge(bytes(33))
    # the device calls check what needs no device first: without a context they are INVALID_ARGUMENT, and nothing is written
    tree = C.c_void_p(0x5a)
    assert lib.bpg_mimc_sponge_many(None, C.c_uint64(0), C.c_uint64(2), bytes(64), out) == 4
    assert lib.bpg_mimc_sponge_many(None, C.c_uint64(1), C.c_uint64(0), bytes(64), out) == 4
    assert lib.bpg_mimc_sponge_many(None, C.c_uint64(1), C.c_uint64((1 << 22) + 1), bytes(64), out) == 4      # an item of more than 2^22 blocks
    for depth in (0, 25):
        assert lib.bpg_merkle_build(None, C.c_uint32(depth), bytes(64), C.byref(tree)) == 4
    assert lib.bpg_merkle_build(None, C.c_uint32(1), None, C.byref(tree)) == 4
    assert lib.bpg_merkle_build(None, C.c_uint32(1), bytes(64), None) == 4
    assert lib.bpg_merkle_root(None, None, out) == 4
    lib.bpg_merkle_free(None, None)
    assert out.raw == b"\x5a" * 32
