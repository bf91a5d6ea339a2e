"""bpg_r1cs_prove_batch without a GPU: the whole-call refusals and count == 0, the header prototype against the Python binding, and the
BPG_BATCH_WAVE_MB knob refused out of range before any device is touched."""
import ctypes as C
import os
import re
import subprocess
import sys
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import gen_proof_fixtures as G


def _items(n):
    inst, state, _ = G.build("range8")
    return bpg._batch_items([(inst, state, b"", bytes(32), 0)] * n)


def test_refused_calls_write_nothing():
    lib = bpg.lib()
    arr, keep = _items(2)
    status = (C.c_int32 * 2)(77, 77)
    assert lib.bpg_r1cs_prove_batch(None, C.c_uint64(2), arr, status) == 4                 # no context
    assert list(status) == [77, 77] and all(k[1].raw[:203] == keep[0][1].raw[:203] for k in keep)
    assert all(k[3].value == O.proof_size(k[0].n) for k in keep)                            # capacities untouched
    fake = C.c_void_p(1)                                                                    # never dereferenced: the call is refused first
    assert lib.bpg_r1cs_prove_batch(fake, C.c_uint64(2), None, status) == 4                 # NULL items
    assert lib.bpg_r1cs_prove_batch(fake, C.c_uint64(2), arr, None) == 4                    # NULL status_out
    assert list(status) == [77, 77]
    assert lib.bpg_r1cs_prove_batch(None, C.c_uint64(0), None, None) == 4                   # no context, even for an empty batch
    assert lib.bpg_r1cs_prove_batch(fake, C.c_uint64(0), None, None) == 0                   # count == 0: nothing to do
    assert b"item" not in (lib.bpg_last_error() or b"")


def test_header_prototype_matches_the_binding():
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    m = re.search(r"bpg_status bpg_r1cs_prove_batch\(([^)]*)\);", hdr)
    assert m, "prototype missing"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["bpg_ctx *ctx", "uint64_t count", "const bpg_batch_item *items", "bpg_status *status_out"]
    pool = re.search(r"bpg_status bpg_pool_prove\(([^)]*)\);", hdr).group(1)
    assert "const bpg_batch_item *items" in pool                                             # the same frozen item type as the pool
    assert [f for f, _ in bpg._BatchItem._fields_] == ["inst", "transcript_state", "m", "v_blinding", "rng_seed", "flags", "proof_out", "proof_len"]
    assert hasattr(bpg.lib(), "bpg_r1cs_prove_batch") and callable(bpg.Context.prove_batch)
    bpg.lib().bpg_abi_version.restype = C.c_uint32
    assert bpg.lib().bpg_abi_version() >= 7


def test_wave_knob_is_checked_at_context_creation():
    code = ("import ctypes as C, bulletproofs_gadgets_amd as bpg\n"
            "h = C.c_void_p()\n"
            "print(bpg.lib().bpg_ctx_create(0, C.byref(h)), bpg.lib().bpg_last_error().decode())\n")
    for bad in ("-1", "1048577", "x", "1.5"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BPG_BATCH_WAVE_MB=bad), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout.startswith("4 ") and "BPG_BATCH_WAVE_MB" in r.stdout, (bad, r.stdout)
