"""The R1CS check without a GPU: the device-less mirror (bpg_test_check_host, csrc/host/check.hpp) against the oracle's yes/no and against a restatement in
Python integers, the refusals of bpg_r1cs_check that need no device, the layout of bpg_check_report, and the host half of the row bookkeeping under the
sanitizers (tests/hostcheck/check_rows.cpp).

Circuits: every case of tests/golden/assembly_cases.py and the reference's thirteen .gadgets stems (tests/golden/resources), assembled by the product's own
host code with hashed stand-in commitments (StubProver).  Each is checked as it stands and with one committed value, one a_O and one coefficient bumped."""
import copy
import ctypes as C
import re
import shutil
import subprocess

import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import cli
import oracle_lib as O
import assembly_cases as AC
from test_template_host import StubProver, Api, FAKE, _err, _ints

L = bpg.L
RES = O.ROOT / "tests" / "golden" / "resources"
STEMS = ["bounds_check", "equality", "inequality", "less_than", "merkle_tree", "mimc_hash", "set_membership", "or", "or2", "or3", "or4", "or5", "example"]
NAMES = list(AC.CASES) + ["stem:" + s for s in STEMS]


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    """name -> FlatInstance with its witness and committed values, assembled once"""
    out = {name: AC.build(Api, name)[0].instance() for name in AC.CASES}
    d = tmp_path_factory.mktemp("stems")
    for s in STEMS:
        for ext in ("gadgets", "inst", "wtns"):
            shutil.copy(RES / ("%s.%s" % (s, ext)), d / ("%s.%s" % (s, ext)))
        p, _ = cli.prover(str(d / s), seed=b"check-host", rng_seed=bytes(32), quiet=True, prover_cls=StubProver, assemble_only=True)
        out["stem:" + s] = p.instance()
    return out


def restate(inst, v):
    """the definition over FlatInstance.row_ptr / term_var / term_coef / coef in Python integers -> (bad multipliers, bad rows), both ascending"""
    coef = [x % L for x in _ints(inst.coef)]
    vals = [[x % L for x in _ints(b)] for b in (inst.aL, inst.aR, inst.aO, v)] + [None]
    muls = [i for i in range(inst.n) if vals[0][i] * vals[1][i] % L != vals[2][i]]
    rp, tv, tc = [int(x) for x in inst.row_ptr], [int(x) for x in inst.term_var], [int(x) for x in inst.term_coef]
    rows = []
    for j in range(inst.q):
        acc = 0
        for k in range(rp[j], rp[j + 1]):
            kind, idx = tv[k] >> 29, tv[k] & 0x1fffffff
            acc += coef[tc[k]] * (1 if kind == 4 else vals[kind][idx])
        if acc % L:
            rows.append(j)
    return muls, rows


def oracle_says(inst, v):
    return O.satisfied(O.FlatCircuit(inst.n, inst.m, inst.aL, inst.aR, inst.aO, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef), v)


def bump(b, index):
    x = (int.from_bytes(b[32 * index:32 * index + 32], "little") + 1) % L
    return b[:32 * index] + x.to_bytes(32, "little") + b[32 * index + 32:]


def agrees(inst, v, cap=16):
    muls, rows = restate(inst, v)
    r = bpg.test_check_host(inst, v, cap)
    assert (r.bad_multipliers, r.first_bad_multiplier) == (len(muls), muls[0] if muls else None)
    assert (r.bad_rows, r.first_bad_row, r.rows) == (len(rows), rows[0] if rows else None, rows[:cap])
    assert r.ok == (not muls and not rows) == oracle_says(inst, v)
    return r


@pytest.mark.parametrize("name", NAMES)
def test_mirror_agrees_with_the_oracle_and_the_restatement(instances, name):
    inst = instances[name]
    r = agrees(inst, inst.v)
    assert r.ok, "every statement of the fixtures holds"
    if inst.m:                                              # one committed value
        agrees(inst, bump(inst.v, inst.m // 2))
    if inst.n:                                              # one a_O: its multiplier, and every row that reads it (equality has no multiplier)
        broken = copy.copy(inst)
        broken.aO = bump(inst.aO, inst.n // 2)
        assert inst.n // 2 in restate(broken, inst.v)[0] and not agrees(broken, inst.v).ok
    broken = copy.copy(inst)                                # one coefficient: every row that uses it with a non-zero value
    broken.coef = bump(inst.coef, int(inst.term_coef[inst.nnz // 2]))
    agrees(broken, inst.v)
    agrees(broken, inst.v, cap=1)
    assert bpg.test_check_host(broken, inst.v, 0).rows == []


def test_unreduced_values_are_taken_mod_l(instances):
    inst = instances["bounds_check_reference"]
    v = _ints(inst.v)
    big = b"".join((x + L).to_bytes(32, "little") for x in v)           # every value + l: below 2^254
    assert bpg.test_check_host(inst, big).ok and bpg.test_check_host(inst, inst.v).ok


def _handles(inst, prog):
    lib = bpg.lib()
    cs, cp = inst.cstruct(), prog.cstruct()
    tmpl, plain = C.c_void_p(), C.c_void_p()
    assert lib.bpg_test_circuit_handle(C.byref(cs), C.byref(cp), C.byref(tmpl)) == 0, _err()
    assert lib.bpg_test_circuit_handle(C.byref(cs), None, C.byref(plain)) == 0, _err()
    return tmpl, plain


def test_refusals_need_no_device(instances):
    lib = bpg.lib()
    p, _, _ = AC.build(Api, "mimc_1_block")
    inst, prog = p.instance(), p.witness_program()
    tmpl, plain = _handles(inst, prog)
    try:
        def refused(word, ctx, c, m, v, cap, rows, have=True, rep=True, status=4):
            n, r = C.c_uint64(77), bpg.CheckReportView(5, 5, 5, 5)
            rc = lib.bpg_r1cs_check(ctx, c, m, v, cap, rows, C.byref(n) if have else None, C.byref(r) if rep else None)
            assert rc == status and word in _err(), (rc, _err())
            assert n.value == 77 and (r.bad_multipliers, r.first_bad_multiplier, r.bad_rows, r.first_bad_row) == (5, 5, 5, 5), "a refused call wrote its outputs"
        rows = (C.c_uint64 * 4)()
        refused("m does not match", FAKE, plain, inst.m + 1, inst.v + bytes(32), 4, rows)         # wrong m
        refused("m does not match", FAKE, tmpl, inst.m - 1, inst.v[:-32], 4, rows)
        refused("pass v", FAKE, plain, inst.m, None, 4, rows)                                     # NULL v on a flat instance
        refused("rows_out", FAKE, plain, inst.m, inst.v, 4, None)                                 # cap > 0 with NULL rows_out
        refused("rows_out", FAKE, tmpl, inst.m, None, 1, None)
        refused("null", None, plain, inst.m, inst.v, 4, rows)
        refused("null", FAKE, None, inst.m, inst.v, 4, rows)
        refused("null", FAKE, plain, inst.m, inst.v, 4, rows, have=False)
        refused("null", FAKE, plain, inst.m, inst.v, 4, rows, rep=False)
        refused("no device state", FAKE, plain, inst.m, inst.v, 4, rows)                          # all arguments fine: the handle is what is missing
        refused("no device state", FAKE, tmpl, inst.m, None, 0, None)
    finally:
        lib.bpg_r1cs_free(None, tmpl); lib.bpg_r1cs_free(None, plain)
    # the mirror's own refusals
    cs = inst.cstruct()
    n, r, rows = C.c_uint64(), bpg.CheckReportView(), (C.c_uint64 * 4)()
    assert lib.bpg_test_check_host(C.byref(cs), None, 4, rows, C.byref(n), C.byref(r)) == 4 and "v is null" in _err()
    assert lib.bpg_test_check_host(C.byref(cs), inst.v, 4, None, C.byref(n), C.byref(r)) == 4 and "rows_out" in _err()
    assert lib.bpg_test_check_host(None, inst.v, 4, rows, C.byref(n), C.byref(r)) == 4
    assert lib.bpg_test_check_host(C.byref(cs), inst.v, 4, rows, None, C.byref(r)) == 4
    assert lib.bpg_test_check_host(C.byref(cs), inst.v, 4, rows, C.byref(n), None) == 4
    assert lib.bpg_test_check_host(C.byref(cs), inst.v, 0, None, C.byref(n), C.byref(r)) == 0 and (r.bad_rows, n.value) == (0, 0)
    cs.aL = cs.aR = cs.aO = None                            # a verifier's instance: no witness
    assert lib.bpg_test_check_host(C.byref(cs), inst.v, 4, rows, C.byref(n), C.byref(r)) == 5 and "no witness" in _err()


FIELDS = ("bad_multipliers", "first_bad_multiplier", "bad_rows", "first_bad_row")


def test_report_layout_matches_the_header_and_abi_version_stays_7(tmp_path):
    src = tmp_path / "layout.c"
    offs = ", ".join("offsetof(bpg_check_report, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bpg.h"\nint main(void) { printf("%u %zu' + " %zu" * len(FIELDS) +
                   '\\n", BPG_ABI_VERSION, sizeof(bpg_check_report), ' + offs + '); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Werror", "-I", str(O.ROOT / "include"), "-o", str(exe), str(src)])
    want = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert want == [7, 32, 0, 8, 16, 24]
    assert [f for f, _ in bpg.CheckReportView._fields_] == list(FIELDS)
    assert [C.sizeof(bpg.CheckReportView)] + [getattr(bpg.CheckReportView, f).offset for f in FIELDS] == want[1:]


CTYPE = {"bpg_ctx *": C.c_void_p, "bpg_circuit *": C.c_void_p, "uint64_t ": C.c_uint64, "const uint8_t *": C.c_char_p, "uint64_t *": C.POINTER(C.c_uint64),
         "bpg_check_report *": C.POINTER(bpg.CheckReportView), "const bpg_r1cs_instance *": C.POINTER(bpg.R1CSInstance)}


def test_header_prototypes_match_the_binding():
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    proto = lambda name: [a.strip() for a in re.search(r"bpg_status %s\(([^)]*)\);" % name, hdr).group(1).split(",")]
    head = ["uint64_t cap", "uint64_t *rows_out", "uint64_t *n_rows_out", "bpg_check_report *report"]
    assert proto("bpg_r1cs_check") == ["bpg_ctx *ctx", "bpg_circuit *c", "uint64_t m", "const uint8_t *v"] + head
    assert proto("bpg_test_check_host") == ["const bpg_r1cs_instance *inst", "const uint8_t *v"] + head
    for name in ("bpg_r1cs_check", "bpg_test_check_host"):
        types = [CTYPE[re.match(r"(.*?)\w+$", a).group(1)] for a in proto(name)]
        assert getattr(bpg.lib(), name).argtypes == types, name
    for attr in ("check", "check_batch"):
        assert hasattr(bpg.ResidentCircuit, attr)
    assert hasattr(bpg.Context, "check_flat") and hasattr(bpg.CheckReport, "items")
    r = bpg.CheckReport(bpg.CheckReportView(0, 2**64 - 1, 3, 131), [131, 260, 389])
    assert not r.ok and r.first_bad_multiplier is None and r.items(129) == [(1, 2), (2, 2), (3, 2)]


def test_row_bookkeeping_under_the_sanitizers(tmp_path):
    """tests/hostcheck/check_rows.cpp: the row-major view by the kernels' own per-entry steps, the bitmap-to-list extraction and the definition
    (csrc/host/check.hpp) through the host compiler under ASan and UBSan (a stand-alone program: no preload, no device)"""
    exe = tmp_path / "check_rows"
    src = O.ROOT / "tests" / "hostcheck" / "check_rows.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.split()[-1] == "ok"
