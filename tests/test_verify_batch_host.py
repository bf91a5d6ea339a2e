"""bpg_r1cs_verify_batch without a GPU: the frozen bpg_verify_item as a C compiler lays it out == the ctypes mirror, the ABI version, refusal of a call
without a context (nothing written back), and the usage errors of `bpg_verifier --batch FILE --combine`."""
import ctypes as C
import subprocess
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import build as bpg_build
import oracle_lib as O
import gen_proof_fixtures as G

FIELDS = ("inst", "circuit", "transcript_state", "m", "V", "proof", "proof_len", "seed", "flags")


def test_verify_item_layout_matches_the_header_and_abi_version_is_7(tmp_path):
    src = tmp_path / "layout.c"
    offs = ", ".join("offsetof(bpg_verify_item, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bpg.h"\nint main(void) { printf("%u %zu' + " %zu" * len(FIELDS) +
                   '\\n", BPG_ABI_VERSION, sizeof(bpg_verify_item), ' + offs + '); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Werror", "-I", str(O.ROOT / "include"), "-o", str(exe), str(src)])
    want = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert want[0] == 7
    bpg.lib().bpg_abi_version.restype = C.c_uint32
    assert bpg.lib().bpg_abi_version() == 7
    assert [f for f, _ in bpg.VerifyItem._fields_] == list(FIELDS)
    got = [C.sizeof(bpg.VerifyItem)] + [getattr(bpg.VerifyItem, f).offset for f in FIELDS]
    assert got == want[1:], (got, want)


def test_a_call_without_context_is_refused_and_writes_nothing():
    inst, state, _ = G.build("range8")
    proof = bytes(O.proof_size(inst.n))
    arr, states, keep = bpg._verify_items([(inst, state, b"", proof, bytes(32), 0), (inst, state, b"", proof, bytes(32), 0)])
    status = (C.c_int32 * 2)(77, 77)
    lib = bpg.lib()
    assert lib.bpg_r1cs_verify_batch(None, C.c_uint64(2), arr, bytes(32), status) == 4               # as bpg_r1cs_verify(NULL, ...)
    assert list(status) == [77, 77] and all(ts.raw[:203] == state for ts in states)
    assert lib.bpg_r1cs_verify_batch(None, C.c_uint64(0), None, None, None) == 4
    cs = inst.cstruct()
    assert lib.bpg_r1cs_verify(None, C.byref(cs), C.create_string_buffer(state, 203), C.c_uint64(0), b"", proof, C.c_uint64(len(proof)), bytes(32), 0) == 4


def test_combine_needs_batch_and_the_verifier(tmp_path):
    prover_bin, verifier_bin = bpg_build.build_cli()
    f = tmp_path / "b.txt"
    f.write_text("a\n")
    r = subprocess.run([str(verifier_bin), "--combine"], capture_output=True, text=True)
    assert r.returncode == 2 and "--combine" in r.stderr
    r = subprocess.run([str(verifier_bin), "a", "--combine"], capture_output=True, text=True)
    assert r.returncode == 2 and "--combine" in r.stderr
    r = subprocess.run([str(prover_bin), "--batch", str(f), "--combine"], capture_output=True, text=True)
    assert r.returncode == 2 and "--combine" in r.stderr
