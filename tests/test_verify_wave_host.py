"""Lockstep verification without a device: the launch plan under the sanitizers (csrc/host/verify_wave_plan.hpp, as a stand-alone program - no preload), the
frozen item struct of include/bpg.h against its ctypes binding, the refusals of bpg_r1cs_verify_resident_batch that need no device, and the integer model of
tests/verify_wave_cases.py against itself."""
import ctypes as C
import re
import subprocess

import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import shape_cases as SC
import verify_cases as VC
import verify_wave_cases as W

CSRC = O.ROOT / "bulletproofs_gadgets_amd" / "csrc"
FAKE = C.c_void_p(0x1000)          # a context pointer no refused call may follow
L = W.L


def _err():
    return bpg.lib().bpg_last_error().decode()


def test_wave_plan_under_the_sanitizers(tmp_path):
    """tests/hostcheck/verify_wave_plan.cpp: plan_verify_wave over N = 1 .. 2^14, K around the wave size, wave_mb 0 / 1 / 512, 1 and 256 compute units, with and
    without tails - regions, waves, chunks, and the refusals by type"""
    exe = tmp_path / "verify_wave_plan"
    src = O.ROOT / "tests" / "hostcheck" / "verify_wave_plan.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr
    assert r.stdout.split()[-1] == "ok"
    assert int(re.search(r"^plans (\d+)$", r.stdout, re.M).group(1)) >= 7 * 3 * 2 * 3 * 5
    # one item per wave at wave_mb = 0; at the default the 1024 bounds checks are one wave, split so that a 256-CU device sees 1024 blocks
    assert "wave_mb 0: N 64 K 1024: 1024 waves of 1, 1 chunks of 1" in r.stdout
    assert "wave_mb 512: N 64 K 1024: 1 waves of 1024, 1024 chunks of 1 | N 1024: 1 waves of 1024, 256 chunks of 4" in r.stdout
    text = (CSRC / "host" / "verify_wave_plan.hpp").read_text()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text


def test_item_struct_of_the_header_is_the_binding(tmp_path):
    """a C11 -pedantic program over include/bpg.h prints sizeof and every offsetof of bpg_verify_resident_item: the ctypes structure agrees, the symbols are
    exported, and the ABI version did not move"""
    fields = [name for name, _ in bpg.VerifyResidentItem._fields_]
    assert fields == ["transcript_state", "V", "proof", "proof_len", "seed", "flags", "param_values", "input_values"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bpg.h"\nint main(void) {\n    printf("sizeof %zu\\n", sizeof(bpg_verify_resident_item));\n'
                   + "".join('    printf("%s %%zu\\n", offsetof(bpg_verify_resident_item, %s));\n' % (f, f) for f in fields)
                   + '    printf("abi %u\\n", (unsigned)BPG_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", str(O.ROOT / "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(bpg.VerifyResidentItem)
    for f in fields:
        assert int(out[f]) == getattr(bpg.VerifyResidentItem, f).offset, f
    assert int(out["abi"]) == 7
    lib = bpg.lib()
    lib.bpg_abi_version.restype = C.c_uint32
    assert lib.bpg_abi_version() == 7
    assert lib.bpg_r1cs_verify_resident_batch and lib.bpg_test_verify_wave_scalars             # AttributeError: not exported


def _item(state, V, proof, seed):
    it = bpg.VerifyResidentItem()
    it.transcript_state = C.cast(state, C.c_void_p); it.V = V; it.proof = proof; it.proof_len = len(proof); it.seed = seed
    return it


def test_refusals_need_no_device():
    """a NULL circuit, NULL items, status_out or batch_seed with count > 0, a NULL field of an item, a handle without device state, count = 0 on such a handle: the call is
    refused as documented before the context is looked at, status_out keeps its sentinel and the transcript state its bytes"""
    lib = bpg.lib()
    circ = VC.circuits()[2]                                      # small5: n = 5, m = 2
    cs = circ.inst.cstruct()
    h = C.c_void_p()
    assert lib.bpg_test_circuit_handle(C.byref(cs), None, C.byref(h)) == 0, _err()
    try:
        proof, seed = bytes(O.proof_size(circ.n, 0)), bytes(32)
        state = C.create_string_buffer(bytes(circ.state), 203)
        arr = (bpg.VerifyResidentItem * 2)(_item(state, circ.V, proof, seed), _item(state, circ.V, proof, seed))
        status = (C.c_int32 * 2)(77, 77)

        def refused(word, ctx, handle, count, items, st, batch_seed=bytes(32)):
            rc = lib.bpg_r1cs_verify_resident_batch(ctx, handle, C.c_uint64(count), items, batch_seed, st)
            assert rc == 4 and word in _err(), (rc, _err())
            assert list(status) == [77, 77] and state.raw[:203] == bytes(circ.state), "a refused call wrote its outputs"

        refused("no device state", FAKE, h, 2, arr, status)
        refused("no device state", None, h, 2, arr, status)
        refused("no device state", FAKE, h, 0, arr, status)                  # the circuit is checked before the count
        refused("null circuit", FAKE, None, 2, arr, status)
        refused("null circuit", FAKE, None, 0, None, None)
        refused("null items", FAKE, h, 2, None, status)
        refused("null items", FAKE, h, 2, arr, None)
        refused("null items", FAKE, h, 2, arr, status, batch_seed=None)
        for field, word in (("transcript_state", "transcript_state"), ("proof", "proof"), ("seed", "seed"), ("V", "V")):
            bad = (bpg.VerifyResidentItem * 2)(_item(state, circ.V, proof, seed), _item(state, circ.V, proof, seed))
            setattr(bad[1], field, None)
            refused("item 1: null " + word, FAKE, h, 2, bad, status)
        # (what follows the circuit's checks cannot be reached without a circuit on a device: test_verify_wave_gpu.py::test_refused_calls_touch_nothing)
        ev = C.create_string_buffer(1024)
        out = C.create_string_buffer(32 * 64)
        assert lib.bpg_test_verify_wave_scalars(None, h, C.c_uint64(1), bytes(32 * 13), None, None, out, out, out, ev, C.c_uint64(1024)) == 7      # BPG_ERR_DEVICE
        assert lib.bpg_test_verify_wave_scalars(FAKE, h, C.c_uint64(1), bytes(32 * 13), None, None, out, out, out, ev, C.c_uint64(1024)) == 4 and "no device state" in _err()
        assert out.raw == bytes(32 * 64)
    finally:
        lib.bpg_r1cs_free(None, h)


def test_the_model_is_self_consistent():
    """on every lockstep case of shape_cases and the six circuits of verify_cases: one item of weight 1 gives the item's own g, h; the sums over three items are
    linear in the weights; the padding lanes carry the factor u and no weight; s_i s_{N-1-i} = 1"""
    circuits = W.model_circuits(with_n0=True)
    assert len(circuits) == len(SC.lockstep_cases()) + 6 == 25 + 6
    for name, circ in circuits:
        lgN = circ.lgN
        for set_name in W.SET_NAMES:
            recs = W.challenge_set(set_name, lgN, W.K_MODEL, name.encode())
            assert all(len(W.record_bytes(r)) == 7 + 2 * lgN for r in recs)
            assert all(u * v % L == 1 for r in recs for u, v in zip(r["uk"], r["ukinv"]))
            per_item = [W.item(circ, r) for r in recs]
            # K = 1 with rho = 1 is the item itself
            for r, (g, h, slot) in zip(recs, per_item):
                g1, h1, s1 = W.wave([circ], [dict(r, rho=1)])
                assert (g1, h1, s1) == (g, h, [slot]), name
                assert len(slot) == circ.m + 2
                s = W.s_vector(r, circ.N)
                assert all(s[i] * s[circ.N - 1 - i] % L == 1 for i in range(circ.N))
                # a padding lane: no weight, the factor u
                for i in range(circ.n, circ.N):
                    assert g[i] == (-r["a"] * s[i]) * r["u"] % L, (name, i)
                    assert h[i] == (pow(r["yinv"], i, L) * (-r["b"] * s[circ.N - 1 - i]) - 1) * r["u"] % L, (name, i)
            # linear in rho: the sum at rho and at rho' differ by (rho' - rho) x the item
            g, h, slots = W.wave([circ] * W.K_MODEL, recs)
            assert slots == [p[2] for p in per_item]
            assert g == [sum(r["rho"] * p[0][i] for r, p in zip(recs, per_item)) % L for i in range(circ.N)]
            for k in range(W.K_MODEL):
                bumped = [dict(r, rho=(r["rho"] + 5) % L) if j == k else r for j, r in enumerate(recs)]
                g2, h2, slots2 = W.wave([circ] * W.K_MODEL, bumped)
                assert slots2 == slots
                assert all((g2[i] - g[i]) % L == 5 * per_item[k][0][i] % L and (h2[i] - h[i]) % L == 5 * per_item[k][1][i] % L for i in range(circ.N)), (name, k)
    # the edge set holds every edge the kernels are run on
    edges = W.challenge_set("edges", 3, 3)
    assert edges[0]["yinv"] == 1 and edges[0]["z"] == 1 and edges[1]["z"] == 0 and edges[0]["x"] == L - 1 and edges[0]["rho"] == 1 and edges[1]["rho"] == L - 1
    assert edges[0]["uk"][0] == L - 1 == edges[0]["ukinv"][0] and edges[1]["uk"] == [L - 1] * 3 and edges[2]["uk"][-1] == L - 1
    zero = W.challenge_set("zero", 3, 3)
    assert zero[0]["rho"] == 0 and (zero[1]["a"], zero[1]["b"]) == (0, 0) and (zero[2]["rho"], zero[2]["a"], zero[2]["b"]) == (0, 0, 0)


def test_lane_arithmetic_compiled_for_the_host(tmp_path):
    """tests/hostcheck/verify_wave_lanes.cpp: the BPG_HD half of csrc/hip/k_vwave.cuh under the sanitizers - the power walk of k_vw_exp, s_i and the weighted
    g_i, h_i of k_vw_scalars on both sides of `real`, and the four cases of a tail entry - against the integer model, on n = 5 padded to 8 under the three
    challenge sets"""
    exe = tmp_path / "verify_wave_lanes"
    src = O.ROOT / "tests" / "hostcheck" / "verify_wave_lanes.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    circ = VC.circuits()[2]
    assert (circ.n, circ.N) == (5, 8)
    hx = lambda x: W.le(x % (1 << 256)).hex()
    standing, param, coef, inp = 12345, L + 7, 2**255 + 19, 2**256 - 1            # the item's own values are reduced as assign reduces them
    runs = 0
    for set_name in W.SET_NAMES:
        for r in W.challenge_set(set_name, circ.lgN, 3, b"lanes"):
            wL, wR, wO, _, _ = SC.model(circ, r["z"])
            args = [str(circ.lgN), str(circ.n)] + [b.hex() for b in W.record_bytes(r)] + [hx(x) for x in wL + wR + wO] + [hx(standing), hx(param), hx(coef), hx(inp)]
            p = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=60)
            assert p.returncode == 0 and p.stderr == "" and p.stdout.split()[-1] == "ok", p.stdout[-1000:] + p.stderr
            got = {(a, int(i)): int.from_bytes(bytes.fromhex(h), "little") for a, i, h in (line.split() for line in p.stdout.splitlines()[:-1])}
            g, h, _ = W.wave([circ], [r])
            s = W.s_vector(r, circ.N)
            for i in range(circ.N):
                assert got["y", i] == pow(r["yinv"], i, L) and got["s", i] == s[i] and got["g", i] == g[i] and got["h", i] == h[i], (set_name, i)
            assert [got["tail", j] for j in range(4)] == [param % L, coef * inp % L, standing, standing]
            runs += 1
    assert runs == 9
