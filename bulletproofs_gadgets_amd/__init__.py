"""bulletproofs_gadgets_amd - MI355X-native Bulletproofs R1CS prove path behind the reference's Gadget/Prover surface.

Thin ctypes binding of libbpg_hip.so (include/bpg.h).  Names mirror the reference so that its tests translate
line by line:
    Transcript, PedersenGens, BulletproofGens, Prover, Verifier          (reference src/bin/prover.rs:47-100)
    commit, commit_single, commit_all_single, verifier_commit             (src/commitments.rs:8-47)
    BoundsCheck, MimcHash256, MerkleTree256, Pattern strings, range_proof (src/*/..._gadget.rs, src/utils.rs)
    be_to_scalar(s), scalar_to_be, mimc_hash                              (src/conversions.rs, src/mimc_hash/mimc.rs)
All arithmetic happens in the shared library; there is no Python or CPU fallback - importing works without a GPU,
creating a Context does not.
"""
import ctypes as C
import os
import pathlib

from . import build as _build

_PKG = pathlib.Path(__file__).resolve().parent
LIB_PATH = _PKG / "libbpg_hip.so"

FLAG_COMPACT_1PHASE = 1
FLAG_NO_1PHASE_DOMSEP = 2
FLAG_EXPANDED_BLINDING = 4      # prover-only opt-in: s_L, s_R expanded from one TranscriptRng draw (include/bpg.h); not upstream's derivation
VAR_MULTIPLIER_LEFT, VAR_MULTIPLIER_RIGHT, VAR_MULTIPLIER_OUTPUT, VAR_COMMITTED, VAR_ONE = 0, 1, 2, 3, 4
VAR_INPUT = 5                   # a public input of the proof (Prover.input / Verifier.input): in instances and programs of templates with inputs only
VAR_GATED = 6                   # input * variable (Prover.gate / Verifier.gate): in instances and programs of templates with gates only
L = 2**252 + 27742317777372353535851937790883648493

STATUS_NAMES = {0: "OK", 1: "INVALID_GENERATORS_LENGTH", 2: "FORMAT_ERROR", 3: "VERIFICATION_ERROR", 4: "INVALID_ARGUMENT",
                5: "MISSING_ASSIGNMENT", 6: "GADGET_ERROR", 7: "DEVICE_ERROR", 8: "INTERNAL", 9: "CHECKPOINT_MISMATCH"}
ERR_CHECKPOINT_MISMATCH = 9


class BpgError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), message))
        self.status = status
        self.first_mismatch = None      # CHECKPOINT_MISMATCH (ResidentCircuit.assign): the lowest flat index item * n_ck + k whose value was wrong
        self.item = None                # ResidentCircuit.prove_batch_checkpointed: the first failing item (first_mismatch is then that item's lowest bad checkpoint)


class R1CSInstance(C.Structure):
    _fields_ = [("n", C.c_uint64), ("q", C.c_uint64), ("m", C.c_uint64), ("nnz", C.c_uint64), ("ncoef", C.c_uint64),
                ("aL", C.c_void_p), ("aR", C.c_void_p), ("aO", C.c_void_p), ("row_ptr", C.c_void_p),
                ("term_var", C.c_void_p), ("term_coef", C.c_void_p), ("coef", C.c_void_p)]


class WitnessProgramView(C.Structure):
    """bpg_witness_program (frozen)."""
    _fields_ = [("lc_ptr", C.c_void_p), ("term_var", C.c_void_p), ("term_coef", C.c_void_p), ("n_params", C.c_uint64), ("param_rows", C.c_void_p)]


class WitnessHintsView(C.Structure):
    """bpg_witness_hints (frozen)."""
    _fields_ = [("n_hints", C.c_uint64), ("hint_mul", C.c_void_p), ("hint_kind", C.c_void_p), ("hint_arg", C.c_void_p)]


class WitnessCheckpointsView(C.Structure):
    """bpg_witness_checkpoints (frozen)."""
    _fields_ = [("n_checkpoints", C.c_uint64), ("vars", C.c_void_p)]


def _checkpoints_cstruct(checkpoints):
    import numpy as np
    arr = np.ascontiguousarray([int(x) for x in checkpoints], dtype=np.uint32)
    c = WitnessCheckpointsView()
    c.n_checkpoints, c.vars = len(arr), arr.ctypes.data if len(arr) else None
    c._owner = arr
    return c


HINT_BIT_PAIR = 1


class WitnessGatesView(C.Structure):
    """bpg_witness_gates: the gate table of a template - gate k is input gate_input[k] times the variable gate_var[k] (kind 0..3)."""
    _fields_ = [("n_gates", C.c_uint64), ("gate_var", C.POINTER(C.c_uint32)), ("gate_input", C.POINTER(C.c_uint32))]


def _gates_cstruct(gates):
    """[(Variable of kind 0..3, input index)] -> (bpg_witness_gates, keep-alive)"""
    n = len(gates)
    gv = (C.c_uint32 * max(n, 1))(*[int(g[0]) for g in gates])
    gi = (C.c_uint32 * max(n, 1))(*[int(g[1]) for g in gates])
    return WitnessGatesView(n, C.cast(gv, C.POINTER(C.c_uint32)), C.cast(gi, C.POINTER(C.c_uint32))), (gv, gi)


class CheckReportView(C.Structure):
    """bpg_check_report (frozen)."""
    _fields_ = [("bad_multipliers", C.c_uint64), ("first_bad_multiplier", C.c_uint64), ("bad_rows", C.c_uint64), ("first_bad_row", C.c_uint64)]


class CheckReport:
    """What bpg_r1cs_check found: the exact counts, the first bad multiplier and row (None when there is none) and `rows`, the lowest violated constraint rows
    in ascending order (at most the max_rows asked for).  Row j is the j-th constrain() call."""

    def __init__(self, view: CheckReportView, rows):
        none = lambda x: None if x == 2**64 - 1 else int(x)
        self.bad_multipliers, self.first_bad_multiplier = int(view.bad_multipliers), none(view.first_bad_multiplier)
        self.bad_rows, self.first_bad_row = int(view.bad_rows), none(view.first_bad_row)
        self.rows = [int(r) for r in rows]

    @property
    def ok(self):
        return self.bad_multipliers == 0 and self.bad_rows == 0

    def items(self, q_src):
        """on a repeat of a template of q_src constraints: `rows` as (copy, row of the source template) pairs"""
        return [(r // q_src, r % q_src) for r in self.rows]

    def parts(self, layout):
        """on a join (Context.join; layout = its .layout): `rows` as (part, item, row of the part's template) triples"""
        return [_join_place(layout, r, "q") for r in self.rows]

    def multiplier_part(self, layout):
        """on a join: the first bad multiplier as (part, item, multiplier of the part's template); None when there is none"""
        return None if self.first_bad_multiplier is None else _join_place(layout, self.first_bad_multiplier, "n")

    def __eq__(self, o):
        return isinstance(o, CheckReport) and self.__dict__ == o.__dict__

    def __repr__(self):
        return "CheckReport(bad_multipliers=%d, first_bad_multiplier=%r, bad_rows=%d, first_bad_row=%r, rows=%r)" % (
            self.bad_multipliers, self.first_bad_multiplier, self.bad_rows, self.first_bad_row, self.rows)


def _join_place(layout, index, what):
    """index of a joined circuit (what = "q": constraint row, "n": multiplier, "m": committed value, "n_params", "n_ck") -> (part, item, index in the part's template)"""
    for p, part in enumerate(layout):
        local = index - part["base_" + what]
        if 0 <= local < part["count"] * part[what]:
            return p, local // part[what], local % part[what]
    raise IndexError("%s index %d is outside the join" % (what, index))


class Timings(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("rng_host", "msm_aiao", "msm_s", "poly", "ipa", "total", "ipa_msm", "ipa_fold", "ipa_sync")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MsmSeg(C.Structure):
    """bpg_msm_seg: one segment of bpg_test_msm."""
    _fields_ = [("table", C.c_uint32), ("result", C.c_uint32), ("first", C.c_uint64), ("len", C.c_uint32), ("lgblk", C.c_uint32),
                ("skip", C.c_void_p)]


class Config(C.Structure):
    """bpg_config (include/bpg.h): zero / None fields fall back to the BPG_* environment variable, then to the profile's default."""
    _fields_ = [("struct_size", C.c_uint32), ("profile", C.c_uint32), ("table_budget_gb", C.c_double), ("chain_workers", C.c_uint32),
                ("chain_lanes", C.c_uint32), ("blocking_sync", C.c_int32), ("gens_cache_dir", C.c_char_p)]


PROFILE_DEFAULT, PROFILE_ONESHOT, PROFILE_SERVING = 0, 1, 2
_PROFILES = {None: 0, "default": 0, "oneshot": 1, "one-shot": 1, "serving": 2, 0: 0, 1: 1, 2: 2}


def make_config(profile=None, table_budget_gb=None, chain_workers=None, chain_lanes=None, blocking_sync=None, gens_cache_dir=None):
    cfg = Config()
    cfg.struct_size = C.sizeof(Config)
    cfg.profile = _PROFILES[profile]
    cfg.table_budget_gb = float(table_budget_gb or 0)
    cfg.chain_workers, cfg.chain_lanes = int(chain_workers or 0), int(chain_lanes or 0)
    cfg.blocking_sync = -1 if blocking_sync is None else (1 if blocking_sync else 0)      # -1 unset (environment, else spin), 1 blocking, 0 spin
    cfg.gens_cache_dir = os.fsencode(gens_cache_dir) if gens_cache_dir else None
    return cfg


class _Term(C.Structure):
    _pack_ = 1
    _fields_ = [("var", C.c_uint32), ("coeff", C.c_uint8 * 32)]


class _LC(C.Structure):
    _fields_ = [("terms", C.POINTER(_Term)), ("n", C.c_uint64)]


_lib = None


def lib():
    """Load (building first if the sources are newer) the shared library."""
    global _lib
    if _lib is None:
        # BPG_LIB_PATH: another build of the SAME sources - the sanitizer builds of tests/hostcheck (host side under ASan/UBSan or TSan) - for the
        # device-less tests; never a different implementation
        override = os.environ.get("BPG_LIB_PATH")
        if override:
            _lib = C.CDLL(override)
        else:
            if not LIB_PATH.exists() or (os.environ.get("BPG_REBUILD") and _build.needs_build()):
                _build.build()
            _lib = C.CDLL(str(LIB_PATH))
        _lib.bpg_strerror.restype = C.c_char_p
        _lib.bpg_last_error.restype = C.c_char_p
        for name in ("bpg_proof_size", "bpg_prover_num_constraints", "bpg_prover_num_multiplications", "bpg_prover_num_committed",
                     "bpg_verifier_num_vars"):
            getattr(_lib, name).restype = C.c_uint64
        _lib.bpg_proof_size.argtypes = [C.c_uint64, C.c_uint32]
        _lib.bpg_r1cs_check.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                        C.POINTER(CheckReportView)]
        _lib.bpg_test_check_host.argtypes = [C.POINTER(R1CSInstance), C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(CheckReportView)]
    return _lib


def _chk(status):
    if status != 0:
        raise BpgError(status, lib().bpg_last_error().decode())


def _buf(n):
    return C.create_string_buffer(max(n, 1))


def _seed32(seed):
    """The 32 bytes that stand in for upstream's thread_rng() draw: fresh OS randomness unless the caller pins them (tests, benchmarks).
    A constant seed makes every blinding factor a function of the public transcript and the commitment blindings alone."""
    if seed is None:
        return os.urandom(32)
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("rng seed must be exactly 32 bytes")
    return seed


def _exact(name, data, nbytes):
    data = bytes(data)
    if len(data) != nbytes:
        raise ValueError("%s must be exactly %d bytes, got %d" % (name, nbytes, len(data)))
    return data


# ------------------------------------------------------------------------------------------------ scalars / conversions
def scalar_from_int(x):
    return (x % L).to_bytes(32, "little")


def be_to_scalars(data: bytes):
    """conversions::be_to_scalars (src/conversions.rs:26-30): list of 32-byte little-endian Scalar encodings."""
    n = C.c_uint64(len(data) // 32 + 2)
    out = _buf(32 * n.value)
    _chk(lib().bpg_be_to_scalars(bytes(data), C.c_uint64(len(data)), out, C.byref(n)))
    return [out.raw[32 * i:32 * i + 32] for i in range(n.value)]


def be_to_scalar(data: bytes):
    """conversions::be_to_scalar (src/conversions.rs:49-53)."""
    if len(data) > 32:
        raise ValueError("the given vector is longer than 32 bytes")
    b = bytes(reversed(data)) + bytes(32 - len(data))
    return b[:31] + bytes([b[31] & 0x7f])


def scalar_to_be(s: bytes):
    return bytes(reversed(s))


def mimc_hash(preimage: bytes):
    """mimc::mimc_hash (src/mimc_hash/mimc.rs:61-75) -> Scalar bytes (little-endian)."""
    out = _buf(32)
    _chk(lib().bpg_mimc_hash(bytes(preimage), C.c_uint64(len(preimage)), out))
    return out.raw


def mimc_sponge(blocks):
    """mimc::mimc_sponge_1 (src/mimc_hash/mimc.rs:26-40) on the host: blocks is a list of 32-byte little-endian values (or their concatenation), each
    any 256-bit value (taken mod l) -> Scalar bytes.  A Merkle node is mimc_sponge([left, right])."""
    data = bytes(blocks) if isinstance(blocks, (bytes, bytearray)) else b"".join(_exact("block", b, 32) for b in blocks)
    if len(data) % 32:
        raise ValueError("blocks must be a whole number of 32-byte values")
    out = _buf(32)
    _chk(lib().bpg_mimc_sponge(data, C.c_uint64(len(data) // 32), out))
    return out.raw


def mimc_sponge_states(blocks):
    """bpg_mimc_sponge_states: mimc_sponge on the host, returning the state after EVERY absorbed block (the last one is the digest) - the checkpoint
    values of a preimage template (Prover.noted)."""
    data = bytes(blocks) if isinstance(blocks, (bytes, bytearray)) else b"".join(_exact("block", b, 32) for b in blocks)
    if len(data) % 32:
        raise ValueError("blocks must be a whole number of 32-byte values")
    out = _buf(len(data))
    _chk(lib().bpg_mimc_sponge_states(data, C.c_uint64(len(data) // 32), out))
    return [out.raw[32 * i:32 * i + 32] for i in range(len(data) // 32)]


def scalar_op(op, a, b=None):
    out = _buf(32)
    _chk(lib().bpg_scalar_op(C.c_int32({"add": 0, "sub": 1, "mul": 2, "invert": 3, "reduce": 4, "from_wide": 5}[op]), a, b, out))
    return out.raw


# ------------------------------------------------------------------------------------------------ variables / LCs
class Variable(int):
    """bulletproofs::r1cs::Variable packed as kind << 29 | index."""
    @property
    def kind(self): return int(self) >> 29
    @property
    def index(self): return int(self) & 0x1fffffff
    @staticmethod
    def One(): return Variable(VAR_ONE << 29)


class LinearCombination:
    """List of (Variable, Scalar bytes) terms; From<Variable>, From<Scalar>, +, -, * Scalar as upstream."""

    def __init__(self, terms=None):
        self.terms = list(terms or [])

    @staticmethod
    def of(x):
        if isinstance(x, LinearCombination):
            return x
        if isinstance(x, Variable):
            return LinearCombination([(x, scalar_from_int(1))])
        if isinstance(x, (bytes, bytearray)):
            return LinearCombination([(Variable.One(), bytes(x))])
        if isinstance(x, int):
            return LinearCombination([(Variable.One(), scalar_from_int(x))])
        raise TypeError(type(x))

    def __add__(self, o): return LinearCombination(self.terms + LinearCombination.of(o).terms)
    def __sub__(self, o): return LinearCombination(self.terms + [(v, scalar_op("sub", bytes(32), c)) for v, c in LinearCombination.of(o).terms])
    def __neg__(self): return LinearCombination([(v, scalar_op("sub", bytes(32), c)) for v, c in self.terms])
    def __mul__(self, s): return LinearCombination([(v, scalar_op("mul", c, s)) for v, c in self.terms])

    def _c(self):
        arr = (_Term * max(len(self.terms), 1))()
        for i, (v, c) in enumerate(self.terms):
            arr[i].var = int(v)
            arr[i].coeff[:] = c
        lc = _LC(C.cast(arr, C.POINTER(_Term)), len(self.terms))
        lc._keep = arr
        return lc


def vars_to_lc(variables):
    return [LinearCombination.of(v) for v in variables]


def _lc_array(lcs):
    cs = [LinearCombination.of(x)._c() for x in lcs]
    arr = (_LC * max(len(cs), 1))(*cs)
    arr._keep = cs
    return arr


# ------------------------------------------------------------------------------------------------ context / generators
LIVE_RESOURCE_KEYS = ("device_buffers", "device_bytes", "pinned_buffers", "pinned_bytes", "streams", "events")


def live_resources():
    """bpg_test_live_resources: what the process holds from the HIP runtime at this moment, every context together; all zero once everything is freed."""
    out = (C.c_uint64 * 6)()
    _chk(lib().bpg_test_live_resources(out))
    return dict(zip(LIVE_RESOURCE_KEYS, (int(x) for x in out)))


class Context:
    """One GPU: PedersenGens (fixed bases) + the BulletproofGens tables resident in HBM."""

    def __init__(self, device=0, profile=None, **config):
        """bpg_ctx_create(device) - the one-shot profile - or, with any of profile="serving" | "oneshot", table_budget_gb, chain_workers,
        chain_lanes, blocking_sync, gens_cache_dir given, bpg_ctx_create_ex with that bpg_config."""
        self._h = C.c_void_p()
        if profile is None and not config:
            _chk(lib().bpg_ctx_create(C.c_int32(device), C.byref(self._h)))
        else:
            cfg = make_config(profile, **config)
            _chk(lib().bpg_ctx_create_ex(C.c_int32(device), C.byref(cfg), C.byref(self._h)))

    def table_bytes(self):
        """bpg_table_bytes: precomputed generator multiples this process holds on the context's device."""
        lib().bpg_table_bytes.restype = C.c_uint64
        return int(lib().bpg_table_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().bpg_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pedersen_bases(self):
        a, b = _buf(32), _buf(32)
        _chk(lib().bpg_pedersen_bases(self._h, a, b))
        return a.raw, b.raw

    def gens_ensure(self, capacity):
        _chk(lib().bpg_gens_ensure(self._h, C.c_uint64(capacity)))

    def gens_export(self, first, count):
        g, h = _buf(32 * count), _buf(32 * count)
        _chk(lib().bpg_gens_export(self._h, C.c_uint64(first), C.c_uint64(count), g, h))
        return g.raw[:32 * count], h.raw[:32 * count]

    def pedersen_commit(self, values, blindings):
        k = len(values)
        out = _buf(32 * k)
        _chk(lib().bpg_pedersen_commit(self._h, C.c_uint64(k), b"".join(values), b"".join(blindings), out))
        return [out.raw[32 * i:32 * i + 32] for i in range(k)]

    def msm_gens(self, first, s, t):
        out = _buf(32)
        _chk(lib().bpg_msm_gens(self._h, C.c_uint64(first), C.c_uint64(len(s)), b"".join(s), b"".join(t), out))
        return out.raw

    def test_msm(self, nmsm, segments, scalars):
        """bpg_test_msm: the bucket-method MSM on a plan of nmsm results and up to 16 segments.  A segment is a dict: table ("G" or "H"),
        first, len, result, lgblk (31 = contiguous) and skip (None, or a list of (len + 31) // 32 uint32 words: bit e set = element e takes no
        part).  scalars: the canonical 32-byte scalars of all segments, in order (a list, or their concatenation).  Returns (nmsm compressed results, the evidence dict: the plan
        the call took and the starts[] / heavy / medium state its kernels left)."""
        import json
        segs = (MsmSeg * max(len(segments), 1))()
        keep = []
        for k, g in enumerate(segments):
            table = {"G": 0, "H": 1}.get(g["table"], g["table"])
            skip = g.get("skip")
            ptr = None
            if skip is not None:
                arr = (C.c_uint32 * max(len(skip), 1))(*skip)
                keep.append(arr)
                ptr = C.cast(arr, C.c_void_p)
            segs[k] = MsmSeg(table, g["result"], g.get("first", 0), g["len"], g.get("lgblk", 31), ptr)
        out = _buf(32 * max(nmsm, 1))
        cap = (1 << 16) + 11 * (max(min(nmsm, 4), 1) * (1 << 19) + 1)     # starts[]: at most 2^19 buckets per result (16 windows of 16 bits), 10 digits and a comma each
        ev = _buf(cap)
        _chk(lib().bpg_test_msm(self._h, C.c_uint32(nmsm), C.c_uint32(len(segments)), segs, scalars if isinstance(scalars, (bytes, bytearray)) else b"".join(scalars),
                                     out, ev, C.c_uint64(cap)))
        return [out.raw[32 * m:32 * m + 32] for m in range(nmsm)], json.loads(ev.value.decode())

    FOLD_KERNELS = ("k_fold_points_wnaf", "k_fold_points_quadw", "k_fold_points_quad", "k_fold_points_split", "k_fold_points_regw", "k_fold_points_reg",
                    "k_fold_points")          # the values of `kernel` in test_fold, in order (csrc/host/fold_plan.hpp FoldKernel)

    def test_fold(self, kernel, lgMr, rounds, first, n, sG, sH, u_ch):
        """bpg_test_fold: the generator fold of one group of `rounds` rounds on the context's own generator tables, through the prover's launch path.  kernel: -1
        (the chooser's), 0..6 or a name of FOLD_KERNELS; sG, sH: 2^rounds - 1 canonical 32-byte scalars each (lists, or their concatenations); u_ch: 32 bytes.
        Returns (the 2 * 2^lgMr compressed points, G side then H side; the evidence dict: what was launched)."""
        import json
        if isinstance(kernel, str):
            kernel = self.FOLD_KERNELS.index(kernel)
        count = 2 << lgMr if 0 <= lgMr <= 26 else 2             # a larger Mr is beyond any generator table: refused before anything is written
        out, ev = _buf(32 * count), _buf(1024)
        nbytes = 32 * ((1 << min(max(rounds, 1), 5)) - 1)          # what the library reads of sG, sH (None goes through as NULL: a refusal)
        join = lambda name, s: None if s is None else _exact(name, s if isinstance(s, (bytes, bytearray)) else b"".join(s), nbytes)
        _chk(lib().bpg_test_fold(self._h, C.c_int32(kernel), C.c_uint32(lgMr), C.c_uint32(rounds), C.c_uint32(first), C.c_uint64(n), join("sG", sG), join("sH", sH),
                                 None if u_ch is None else _exact("u_ch", u_ch, 32), out, ev, C.c_uint64(1024)))
        return [out.raw[32 * i:32 * i + 32] for i in range(count)], json.loads(ev.value.decode())

    def test_tail(self, lgM0, tables, first, n, a, b, yinv, u_ch, gamma0, eta0, w, u):
        """bpg_test_tail: the table-driven tail of the inner-product argument on the context's own generators G[0, M0), H[0, M0) and B, through the prover's freeze
        and per-round steps.  tables: 0 (4-bit tables of the original generators), 1 (4-bit tables in the arena, as for folded generators), 2 (8-bit tables);
        a, b: 2^lgM0 canonical 32-byte scalars each and u: one challenge per sub-round (lists, or their concatenations); the others: 32 bytes.  Returns ([(L_j, R_j)]
        per sub-round, the folded a, the folded b as lists of 32-byte scalars, the evidence dict: what was launched)."""
        import json
        M0 = 1 << lgM0 if 0 <= lgM0 <= 14 else 1                 # a larger M0 is refused before anything is read or written
        join = lambda name, s, count: None if s is None else _exact(name, s if isinstance(s, (bytes, bytearray)) else b"".join(s), 32 * count)
        ub = None if u is None else (u if isinstance(u, (bytes, bytearray)) else b"".join(u))
        rounds = 0 if ub is None else len(ub) // 32
        left = M0 >> min(rounds, lgM0) if 0 <= lgM0 <= 14 else 1
        lr, ab, ev = _buf(64 * max(rounds, 1)), _buf(64 * left), _buf(1024)
        one = lambda name, s: None if s is None else _exact(name, s, 32)
        _chk(lib().bpg_test_tail(self._h, C.c_uint32(lgM0), C.c_uint32(tables), C.c_uint32(first), C.c_uint64(n), join("a", a, M0), join("b", b, M0), one("yinv", yinv),
                                 one("u_ch", u_ch), one("gamma0", gamma0), one("eta0", eta0), one("w", w), C.c_uint32(rounds), ub, lr, ab, ev, C.c_uint64(1024)))
        cut = lambda raw, k: [raw[32 * i:32 * i + 32] for i in range(k)]
        return ([(lr.raw[64 * j:64 * j + 32], lr.raw[64 * j + 32:64 * j + 64]) for j in range(rounds)], cut(ab.raw, left), cut(ab.raw[32 * left:], left),
                json.loads(ev.value.decode()))

    def test_commit3(self, lgM0, n, aL, aR, aO, sL, sR, blind):
        """bpg_test_commit3: A_I, A_O, S from the window tables of the context's own generators G[0, M0), H[0, M0) (k_tt_commit3 and its finish).  aL .. sR: n
        canonical 32-byte scalars each, blind: three (lists, or their concatenations).  Returns ([A_I, A_O, S] encoded, the evidence dict)."""
        import json
        count = n if isinstance(n, int) and 0 <= n <= 1 << 14 else 0
        join = lambda name, s, k: None if s is None else _exact(name, s if isinstance(s, (bytes, bytearray)) else b"".join(s), 32 * k)
        out, ev = _buf(96), _buf(1024)
        _chk(lib().bpg_test_commit3(self._h, C.c_uint32(lgM0), C.c_uint64(n), join("aL", aL, count), join("aR", aR, count), join("aO", aO, count), join("sL", sL, count),
                                    join("sR", sR, count), join("blind", blind, 3), out, ev, C.c_uint64(1024)))
        return [out.raw[32 * k:32 * k + 32] for k in range(3)], json.loads(ev.value.decode())

    def test_fe_ops(self, op, a_list, b_list):
        n = len(a_list)
        out = _buf(32 * n)
        _chk(lib().bpg_test_fe_ops(self._h, C.c_int32(op), C.c_uint64(n), b"".join(a_list), b"".join(b_list), out))
        return [out.raw[32 * i:32 * i + 32] for i in range(n)]

    def test_decompress(self, encodings):
        """bpg_test_decompress: k_decompress on a list of 32-byte encodings -> (ok flags, [(x, y)] as integers - the affine coordinates the kernel
        wrote for every entry, meaningful where the flag is 1)."""
        n = len(encodings)
        ok, xy = (C.c_uint32 * max(n, 1))(), _buf(64 * n)
        _chk(lib().bpg_test_decompress(self._h, C.c_uint64(n), b"".join(_exact("encoding", e, 32) for e in encodings), ok, xy))
        return [int(ok[i]) for i in range(n)], [(int.from_bytes(xy.raw[64 * i:64 * i + 32], "little"), int.from_bytes(xy.raw[64 * i + 32:64 * i + 64], "little"))
                                                for i in range(n)]

    def mimc_sponge_many(self, items, blocks_per_item):
        """bpg_mimc_sponge_many: one mimc_sponge per item on the GPU.  items: a list of items (each blocks_per_item x 32 bytes, or a list of that many
        32-byte blocks), or the concatenation of all of them -> list of 32-byte digests."""
        if isinstance(items, (bytes, bytearray)):
            data = bytes(items)
        else:
            data = b"".join(bytes(it) if isinstance(it, (bytes, bytearray)) else b"".join(it) for it in items)
        size = 32 * blocks_per_item
        if size <= 0 or len(data) % size:
            raise ValueError("items must hold a whole number of items of blocks_per_item x 32 bytes")
        count = len(data) // size
        out = _buf(32 * count)
        _chk(lib().bpg_mimc_sponge_many(self._h, C.c_uint64(count), C.c_uint64(blocks_per_item), data, out))
        raw = out.raw                 # one copy of the buffer, not one per item
        return [raw[32 * i:32 * i + 32] for i in range(count)]

    def merkle_tree(self, leaves, depth=None, empty=None, reserve=None, keys=None) -> "MerkleTree":
        """Without `depth`, bpg_merkle_build: the full MiMC Merkle tree over 2^depth leaves (a list of 32-byte values, or their concatenation), resident on
        the GPU.  With `depth`, bpg_merkle_build_partial: a tree of capacity 2^depth over any len(leaves) <= 2^depth leaves, none included, whose other
        leaves hold `empty` (32 bytes, taken mod l; None = zero) - the tree MerkleTree.append grows.  With `depth` and `reserve`,
        bpg_merkle_build_prefix: the same tree in the prefix layout, depth up to 32, with room for `reserve` <= min(2^depth, 2^24) leaves and about 64
        bytes of device memory per reserved leaf; append grows the reserve as needed.  With `depth` and `keys` (distinct ints below 2^depth, any order, one
        per leaf; [] with no leaves: the empty keyed tree), bpg_merkle_build_keyed: leaves[i] sits at key keys[i] and every other leaf holds `empty`;
        MerkleTree.put inserts and replaces."""
        return MerkleTree(self, leaves, depth, empty, reserve, keys)

    def profile_set(self, mode):
        _chk(lib().bpg_profile_set(self._h, C.c_int32(mode)))

    def _report(self):
        import json
        out = _buf(1 << 16)
        _chk(lib().bpg_profile_report(self._h, out, C.c_uint64(1 << 16)))
        return json.loads(out.value.decode())

    def profile_report(self):
        """bpg_profile_report: {kernel: {count, total_ms, alg_bytes, device_bytes, field_mults}} since the last bpg_profile_set."""
        return {k: v for k, v in self._report().items() if not k.startswith("_")}

    def schedule(self):
        """The "_schedule" object of bpg_profile_report: what the knobs, the profile and the table budget of this context settled on (tail start,
        fold groups, window caps, NAF width and parts in use, epilogue segment, whether the last proof took the shared-device variants)."""
        return self._report()["_schedule"]

    def bench_fe_mul(self, iters=2000):
        r = C.c_double()
        _chk(lib().bpg_bench_fe_mul(self._h, C.c_uint32(iters), C.byref(r)))
        return r.value

    def verify_flat(self, inst: "FlatInstance", transcript_state, commitments, proof, seed=None, flags=0):
        """bpg_r1cs_verify: 0 = accepted, 3 = VERIFICATION_ERROR, 2 = FORMAT_ERROR, 1 = INVALID_GENERATORS_LENGTH."""
        return _verify_flat(self, inst, transcript_state, commitments, proof, seed, flags)

    # ---- PART 1 boundary on flattened instances
    def upload(self, inst: "FlatInstance"):
        h = C.c_void_p()
        cs = inst.cstruct()
        _chk(lib().bpg_r1cs_upload(self._h, C.byref(cs), C.byref(h)))
        return ResidentCircuit(self, h, inst.n, inst.m, q=inst.q)

    def check_flat(self, inst: "FlatInstance", max_rows=16) -> "CheckReport":
        """upload + ResidentCircuit.check(inst.v) + free: does the instance's own witness satisfy it, and which constraints does it break"""
        rc = self.upload(inst)
        try:
            return rc.check(inst.v if inst.m else None, max_rows)
        finally:
            rc.free()

    def upload_template(self, inst: "FlatInstance", program: "WitnessProgram", hints: "WitnessHints" = None, checkpoints=None, inputs=None, gates=None):
        """bpg_r1cs_upload_template: the instance (with or without a witness) plus its witness program; ResidentCircuit.assign gives it fresh witnesses.
        hints (a circuit with range proofs, Prover.witness_program(hints=True)): bpg_r1cs_upload_template_hinted.
        checkpoints (bpg_r1cs_upload_template_checkpointed): multiplier Variables whose values the caller hands to assign(..., checkpoints=values); the
        segments that read them stop waiting for the ones that compute them.
        inputs (bpg_r1cs_upload_template_inputs; an instance from Prover.template_instance): the values of the public inputs the instance and the program
        name (kind VAR_INPUT), as many as the template is to take with every assign(..., inputs=values); an int: that many, for an instance without a witness.
        gates (bpg_r1cs_upload_template_gated; Prover.gates()): [(gated Variable, input index)], the table the terms of kind VAR_GATED in the instance and
        the program name.  Such a template is served by assign, prove, verify, set_inputs, check, prove_batch_inputs and verify_batch; repeat and join refuse it."""
        h = C.c_void_p()
        cs, cp = inst.cstruct(), program.cstruct()
        n_in = 0 if inputs is None else inputs if isinstance(inputs, int) else (len(inputs) // 32 if isinstance(inputs, (bytes, bytearray)) else len(inputs))
        if n_in:
            iv = None if isinstance(inputs, int) else _scalars32("inputs", inputs, n_in)
            if iv is None:                                  # no values: the shape alone (a verifier's upload).  The struct must not claim a witness then
                cs.aL = cs.aR = cs.aO = None
            ch = hints.cstruct() if hints is not None and len(hints) else None
            ck = _checkpoints_cstruct(checkpoints or [])
            if gates:
                gs, _keep = _gates_cstruct(gates)
                _chk(lib().bpg_r1cs_upload_template_gated(self._h, C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.byref(ck),
                                                          C.c_uint64(n_in), iv, C.byref(gs), C.byref(h)))
            else:
                _chk(lib().bpg_r1cs_upload_template_inputs(self._h, C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.byref(ck),
                                                           C.c_uint64(n_in), iv, C.byref(h)))
            rc = ResidentCircuit(self, h, inst.n, inst.m, n_params=len(program.param_rows), q=inst.q, n_ck=len(checkpoints or []), n_inputs=n_in)
            rc.n_gates = len(gates or [])
            return rc
        if gates:
            raise BpgError(4, "upload_template: gates without public inputs (a gate is input * variable)")
        if checkpoints is not None and len(checkpoints):
            ch = hints.cstruct() if hints is not None and len(hints) else None
            ck = _checkpoints_cstruct(checkpoints)
            _chk(lib().bpg_r1cs_upload_template_checkpointed(self._h, C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.byref(ck), C.byref(h)))
            return ResidentCircuit(self, h, inst.n, inst.m, n_params=len(program.param_rows), q=inst.q, n_ck=len(checkpoints))
        if hints is not None and len(hints):
            ch = hints.cstruct()
            _chk(lib().bpg_r1cs_upload_template_hinted(self._h, C.byref(cs), C.byref(cp), C.byref(ch), C.byref(h)))
        else:
            _chk(lib().bpg_r1cs_upload_template(self._h, C.byref(cs), C.byref(cp), C.byref(h)))
        return ResidentCircuit(self, h, inst.n, inst.m, n_params=len(program.param_rows), q=inst.q)

    def blinding_begin(self, transcript_state, v_blinding, rng_seed, max_multipliers):
        """bpg_blinding_begin: start the blinding chain of the next prove on this context (state after every "V" append, m x 32 blinding bytes)."""
        ts = _buf(203); ts.raw = _exact("transcript_state", transcript_state, 203)
        v_blinding = bytes(v_blinding)
        if len(v_blinding) % 32:
            raise ValueError("v_blinding must be a multiple of 32 bytes")
        _chk(lib().bpg_blinding_begin(self._h, ts, C.c_uint64(len(v_blinding) // 32), v_blinding, _seed32(rng_seed), C.c_uint64(max_multipliers)))

    def attach_chain_pool(self, pool, max_streams=2):
        """bpg_ctx_attach_chain_pool: this context's blinding streams are drawn by the shared pool (None: back to its own chain worker)."""
        _chk(lib().bpg_ctx_attach_chain_pool(self._h, pool._h if pool is not None else None, C.c_uint32(max_streams)))
        self._pool = pool                                     # the pool must outlive the attachment

    def set_chain_lanes(self, lanes: int):
        """bpg_ctx_set_chain_lanes: queued blinding streams each chain thread draws in lockstep (1..8; workers * lanes + 1 streams may be alive)."""
        _chk(lib().bpg_ctx_set_chain_lanes(self._h, C.c_uint32(lanes)))

    def set_chain_workers(self, workers: int):
        """bpg_ctx_set_chain_workers: threads that draw queued blinding streams side by side (workers + 1 streams may be alive)."""
        _chk(lib().bpg_ctx_set_chain_workers(self._h, C.c_uint32(workers)))

    def chain_cpu(self):
        """Host core the chain worker of this context last drew a blinding stream on (-1: none yet)."""
        lib().bpg_chain_cpu.restype = C.c_int32
        return int(lib().bpg_chain_cpu(self._h))

    def prove_flat(self, inst: "FlatInstance", transcript_state, v_blinding, rng_seed=None, flags=0):
        ts = _buf(203); ts.raw = _exact("transcript_state", transcript_state, 203)
        v_blinding, rng_seed = _exact("v_blinding", v_blinding, 32 * inst.m), _seed32(rng_seed)
        cap = lib().bpg_proof_size(inst.n, flags)
        out = _buf(cap); ln = C.c_uint64(cap)
        cs = inst.cstruct()
        _chk(lib().bpg_r1cs_prove(self._h, C.byref(cs), ts, C.c_uint64(inst.m), v_blinding, rng_seed, C.c_uint32(flags), out, C.byref(ln)))
        return out.raw[:ln.value], ts.raw[:203]


class MerkleTree:
    """A binary MiMC Merkle tree of capacity 2^depth resident on the GPU of a context (bpg_merkle_*): node = mimc_sponge([left, right]) over the children
    as they are, which is what MerkleTree256 constrains for a "(W W)" node.  Level 0 is the root, level `depth` the leaves.  It holds `size` leaves; the
    leaves from `size` on hold one `empty` value, so every node is that of the tree over the padded list, and append() puts more leaves behind the last.
    A keyed tree (`keyed` is True; Context.merkle_tree(..., keys=)) holds its leaves at arbitrary keys below 2^depth instead and `empty` everywhere else:
    `size` is the number of keys held, put() inserts and replaces, update() replaces only, and every read works as on the other layouts."""

    def __init__(self, ctx: "Context", leaves, depth=None, empty=None, reserve=None, keys=None):
        data = bytes(leaves) if isinstance(leaves, (bytes, bytearray)) else b"".join(_exact("leaf", x, 32) for x in leaves)
        n = len(data) // 32
        self.keyed = keys is not None
        if self.keyed:
            keys = [int(k) for k in keys]
            if depth is None:
                raise ValueError("`keys` belong to a tree built with `depth`")
            if reserve is not None:
                raise ValueError("a keyed tree has no `reserve`")
            if len(data) % 32 or len(keys) != n:
                raise ValueError("one 32-byte leaf per key")
            empty = None if empty is None else _exact("empty", empty, 32)
            self.ctx, self.depth, self._h = ctx, int(depth), C.c_void_p()
            _chk(lib().bpg_merkle_build_keyed(ctx._h, C.c_uint32(self.depth), C.c_uint64(n), (C.c_uint64 * n)(*keys) if n else None, data if n else None, empty, C.byref(self._h)))
            return
        if depth is None and reserve is not None:
            raise ValueError("`reserve` belongs to a tree built with `depth`")
        if depth is None:
            if empty is not None:
                raise ValueError("`empty` belongs to a tree built with `depth`")
            if len(data) % 32 or n < 1 or n & (n - 1):
                raise ValueError("a tree built without `depth` has 2^depth leaves of 32 bytes each")
            self.ctx, self.depth, self._h = ctx, n.bit_length() - 1, C.c_void_p()
            _chk(lib().bpg_merkle_build(ctx._h, C.c_uint32(self.depth), data, C.byref(self._h)))
            return
        if len(data) % 32:
            raise ValueError("leaves are 32 bytes each")
        empty = None if empty is None else _exact("empty", empty, 32)
        self.ctx, self.depth, self._h = ctx, int(depth), C.c_void_p()
        if reserve is not None:
            _chk(lib().bpg_merkle_build_prefix(ctx._h, C.c_uint32(self.depth), C.c_uint64(int(reserve)), C.c_uint64(n), data if n else None, empty, C.byref(self._h)))
            return
        _chk(lib().bpg_merkle_build_partial(ctx._h, C.c_uint32(self.depth), C.c_uint64(n), data if n else None, empty, C.byref(self._h)))

    def _handle(self):
        if not self._h:
            raise ValueError("this tree has been freed")
        return self._h

    @property
    def size(self):
        """The number of leaves the tree holds (bpg_merkle_size): leaves [size, capacity) hold the empty value."""
        out = C.c_uint64()
        _chk(lib().bpg_merkle_size(self.ctx._h, self._handle(), C.byref(out), None))
        return out.value

    @property
    def capacity(self):
        return 1 << self.depth

    @property
    def reserved(self):
        """bpg_merkle_reserved: (the leaves there is room for, the device bytes the tree holds); a tree of the dense layout: (2^depth, its array)."""
        r, b = C.c_uint64(), C.c_uint64()
        _chk(lib().bpg_merkle_reserved(self.ctx._h, self._handle(), C.byref(r), C.byref(b)))
        return r.value, b.value

    def reserve(self, n):
        """bpg_merkle_reserve: room for at least n leaves in a tree of the prefix layout (a no-op when there is; a reserve never shrinks)."""
        _chk(lib().bpg_merkle_reserve(self.ctx._h, self._handle(), C.c_uint64(int(n))))

    def append(self, leaves, return_root=False):
        """bpg_merkle_append: the leaves go behind the last one and only their ancestors are recomputed; returns the index of the first new leaf, and the new
        root with it when return_root is set."""
        data = bytes(leaves) if isinstance(leaves, (bytes, bytearray)) else b"".join(_exact("leaf", x, 32) for x in leaves)
        if len(data) % 32:
            raise ValueError("leaves are 32 bytes each")
        first, root = C.c_uint64(), _buf(32)
        _chk(lib().bpg_merkle_append(self.ctx._h, self._handle(), C.c_uint64(len(data) // 32), data if data else None, C.byref(first), root if return_root else None))
        return (first.value, root.raw) if return_root else first.value

    def empty_nodes(self):
        """bpg_merkle_empty_nodes: [E_0, ..., E_depth], E_k = a subtree without a leaf k levels above the leaves (E_0 = the empty value, reduced)."""
        out = _buf(32 * (self.depth + 1))
        _chk(lib().bpg_merkle_empty_nodes(self.ctx._h, self._handle(), out))
        raw = out.raw
        return [raw[32 * k:32 * k + 32] for k in range(self.depth + 1)]

    def root(self):
        out = _buf(32)
        _chk(lib().bpg_merkle_root(self.ctx._h, self._handle(), out))
        return out.raw

    def nodes(self, level, first=0, count=None):
        """`count` nodes of `level` from node `first` (default: the rest of the level) as 32-byte scalars."""
        if count is None:
            count = (1 << level) - first
        out = _buf(32 * max(count, 0))
        _chk(lib().bpg_merkle_nodes(self.ctx._h, self._handle(), C.c_uint32(level), C.c_uint64(first), C.c_uint64(count), out))
        raw = out.raw
        return [raw[32 * i:32 * i + 32] for i in range(count)]

    def paths(self, indices):
        """For every leaf index its `depth` siblings from the leaf level upward: [[sibling of the leaf, sibling of its parent, ...], ...]."""
        k, d = len(indices), self.depth
        out = _buf(32 * d * k)
        _chk(lib().bpg_merkle_paths(self.ctx._h, self._handle(), C.c_uint64(k), (C.c_uint64 * max(k, 1))(*indices), out))
        raw = out.raw
        return [[raw[32 * (i * d + j):32 * (i * d + j) + 32] for j in range(d)] for i in range(k)]

    def path_nodes(self, indices):
        """bpg_merkle_path_nodes: for every leaf index the `depth` nodes ON its path, from the leaf's parent upward, the root last - the checkpoint values of
        a path template (workloads.merkle_path_pattern), where paths() gives its committed values."""
        k, d = len(indices), self.depth
        out = _buf(32 * d * k)
        _chk(lib().bpg_merkle_path_nodes(self.ctx._h, self._handle(), C.c_uint64(k), (C.c_uint64 * max(k, 1))(*indices), out))
        raw = out.raw
        return [[raw[32 * (i * d + j):32 * (i * d + j) + 32] for j in range(d)] for i in range(k)]

    def path_inputs(self, indices):
        """The public inputs of a MerklePath256 template for every leaf index: paths() and root() through merkle_path_inputs, one list of 4 * depth + 1
        scalars per index - what assign(inputs=), prove_batch_inputs and verify_batch take."""
        root = self.root()
        return [merkle_path_inputs(i, sib, root) for i, sib in zip(indices, self.paths(indices))]

    def update(self, indices, leaves):
        """Replace leaf indices[i] by leaves[i] (distinct indices) and recompute their ancestors."""
        k = len(indices)
        data = bytes(leaves) if isinstance(leaves, (bytes, bytearray)) else b"".join(_exact("leaf", x, 32) for x in leaves)
        if len(data) != 32 * k:
            raise ValueError("one 32-byte leaf per index")
        _chk(lib().bpg_merkle_update(self.ctx._h, self._handle(), C.c_uint64(k), (C.c_uint64 * max(k, 1))(*indices), data))

    def put(self, keys, leaves, return_root=False):
        """bpg_merkle_put on a keyed tree: the leaf of a held key is replaced, a key that is not held is inserted (distinct keys, any order); only the
        ancestors of the put keys are recomputed.  Returns how many keys were inserted, and the new root with it when return_root is set."""
        keys = [int(k) for k in keys]
        k = len(keys)
        data = bytes(leaves) if isinstance(leaves, (bytes, bytearray)) else b"".join(_exact("leaf", x, 32) for x in leaves)
        if len(data) != 32 * k:
            raise ValueError("one 32-byte leaf per key")
        inserted, root = C.c_uint64(), _buf(32)
        _chk(lib().bpg_merkle_put(self.ctx._h, self._handle(), C.c_uint64(k), (C.c_uint64 * k)(*keys) if k else None, data if k else None, C.byref(inserted),
                                  root if return_root else None))
        return (inserted.value, root.raw) if return_root else inserted.value

    def get(self, keys):
        """bpg_merkle_get: (the leaves at `keys`, whether each key is held).  A key that is not held reads as the empty value; on a dense or prefix tree
        a key is a leaf index, held when it is below `size`."""
        keys = [int(k) for k in keys]
        k = len(keys)
        out, held = _buf(32 * k), _buf(max(k, 1))
        _chk(lib().bpg_merkle_get(self.ctx._h, self._handle(), C.c_uint64(k), (C.c_uint64 * max(k, 1))(*keys), out, held))
        raw, h = out.raw, held.raw
        return [raw[32 * i:32 * i + 32] for i in range(k)], [bool(h[i]) for i in range(k)]

    def keys(self, first=0, count=None):
        """bpg_merkle_keys: held keys in ascending order, `count` of them from the `first` one (default: the rest).  Dense and prefix trees: key i = i."""
        if count is None:
            count = self.size - first
        out = (C.c_uint64 * max(count, 1))()
        _chk(lib().bpg_merkle_keys(self.ctx._h, self._handle(), C.c_uint64(first), C.c_uint64(count), out))
        return [int(out[i]) for i in range(count)]

    @property
    def node_counts(self):
        """bpg_merkle_node_counts of a keyed tree: ([stored nodes of height 0 (the leaves), ..., of height depth (the root)], device bytes held)."""
        counts, b = (C.c_uint64 * (self.depth + 1))(), C.c_uint64()
        _chk(lib().bpg_merkle_node_counts(self.ctx._h, self._handle(), counts, C.byref(b)))
        return [int(x) for x in counts], b.value

    def free(self):
        if getattr(self, "_h", None):
            lib().bpg_merkle_free(getattr(self.ctx, "_h", None), self._h)      # (a closed context released the tree's memory; the handle goes here)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ChainPool:
    """bpg_chain_pool_*: host threads that draw the blinding chains of every context attached to them; lanes[k] = chains thread k draws in lockstep."""

    def __init__(self, lanes):
        lanes = [int(x) for x in lanes]
        self._h = C.c_void_p()
        arr = (C.c_uint32 * len(lanes))(*lanes)
        _chk(lib().bpg_chain_pool_create(C.c_uint32(len(lanes)), arr, C.byref(self._h)))
        self.lanes, self.capacity = lanes, sum(lanes)

    def close(self):
        if getattr(self, "_h", None):
            lib().bpg_chain_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _verify_flat(ctx, inst, transcript_state, commitments, proof, seed=None, flags=0):
    ts = _buf(203); ts.raw = _exact("transcript_state", transcript_state, 203)
    seed, commitments, proof = _seed32(seed), _exact("commitments", commitments, 32 * inst.m), bytes(proof)
    cs = inst.cstruct()
    cs.aL = cs.aR = cs.aO = None
    return lib().bpg_r1cs_verify(ctx._h, C.byref(cs), ts, C.c_uint64(inst.m), commitments, proof, C.c_uint64(len(proof)), seed, C.c_uint32(flags))


def test_verify_replay(n, m, gens_capacity, transcript_state, proof, seed, flags=0):
    """bpg_test_verify_replay (no device): the host half of bpg_r1cs_verify - R1CSProof::from_bytes and the Fiat-Shamir replay - alone ->
    (status, decided): decided = False means the proof got past it and the device decides."""
    status, decided = C.c_int32(-1), C.c_int32(-1)
    proof = bytes(proof)
    _chk(lib().bpg_test_verify_replay(C.c_uint64(n), C.c_uint64(m), C.c_uint64(gens_capacity), _exact("transcript_state", transcript_state, 203), proof,
                                      C.c_uint64(len(proof)), _exact("seed", seed, 32), C.c_uint32(flags), C.byref(status), C.byref(decided)))
    return status.value, bool(decided.value)


def _script_bytes(script):
    """a script of challenges (y, z, u, x, w, u_1 .. u_lgN: 32-byte scalars) -> (bytes, count); the library checks what it holds"""
    script = [bytes(s) for s in script]
    if any(len(s) != 32 for s in script):
        raise ValueError("every script entry is a 32-byte scalar")
    return b"".join(script), len(script)


def _script_arrays(scripts):
    """one script per item -> (const uint8_t *const *, uint64_t *, keep-alive)"""
    packed = [_script_bytes(s) for s in scripts]
    n = max(len(packed), 1)
    ptrs, lens = (C.c_char_p * n)(), (C.c_uint64 * n)()
    for k, (b, ln) in enumerate(packed):
        ptrs[k], lens[k] = b, ln
    return ptrs, lens, packed


def test_verify_replay_scripted(n, m, gens_capacity, transcript_state, proof, seed, flags=0, script=None):
    """bpg_test_verify_replay_scripted (no device): test_verify_replay on a transcript that hands out `script` (None: a plain transcript) ->
    (status, transcript state after, the challenges the replay drew - zero where it did not get -, script entries consumed).  Raises BpgError
    (INVALID_ARGUMENT) for a script the hooks refuse."""
    N = 1
    while N < n:
        N *= 2
    count = 5 + N.bit_length() - 1
    ts = _buf(203); ts.raw = _exact("transcript_state", transcript_state, 203)
    status, consumed, ch = C.c_int32(-1), C.c_uint64(0), _buf(32 * count)
    proof = bytes(proof)
    sb, sn = _script_bytes(script) if script is not None else (None, 0)
    _chk(lib().bpg_test_verify_replay_scripted(C.c_uint64(n), C.c_uint64(m), C.c_uint64(gens_capacity), ts, proof, C.c_uint64(len(proof)), _exact("seed", seed, 32),
                                               C.c_uint32(flags), sb, C.c_uint64(sn), C.byref(status), ch, C.byref(consumed)))
    return status.value, ts.raw[:203], [ch.raw[32 * k:32 * k + 32] for k in range(count)], consumed.value


def test_check_host(inst, v=None, max_rows=16) -> "CheckReport":
    """bpg_test_check_host (no device): the definition of bpg_r1cs_check in host C++ on an instance with its witness; v: the m committed values (None: inst.v)"""
    v = inst.v if v is None else v
    cs = inst.cstruct()
    if not inst.aL and inst.n:
        cs.aL = cs.aR = cs.aO = None
    rows = (C.c_uint64 * max(max_rows, 1))()
    have, rep = C.c_uint64(), CheckReportView()
    _chk(lib().bpg_test_check_host(C.byref(cs), _scalars32("v", v, inst.m) if inst.m else None, C.c_uint64(max_rows), rows if max_rows else None, C.byref(have), C.byref(rep)))
    return CheckReport(rep, rows[:have.value])


def test_template_repeat_instance(inst, program, hints, count, param_values=None):
    """bpg_test_template_repeat_instance (no device): the instance of `program`'s template repeated `count` times, row-major, as it stands after an assign of
    param_values (count x n_params scalars, item-major; None: the constants of the template's own rows) -> (row_ptr, term_var, term_coef, coef bytes)"""
    import numpy as np
    cs, cp = inst.cstruct(), program.cstruct()
    ch = hints.cstruct() if hints is not None and len(hints) else None
    npar = len(program.param_rows)
    rows, terms, ncoef = count * inst.q + 1, count * (inst.nnz + npar), inst.ncoef + count * npar
    row_ptr, tv, tc, coef = np.zeros(rows, np.uint64), np.zeros(max(terms, 1), np.uint32), np.zeros(max(terms, 1), np.uint32), _buf(32 * ncoef)
    nnz, nc = C.c_uint64(), C.c_uint64()
    pv = None if param_values is None else _scalars32("param_values", param_values, count * npar)
    _chk(lib().bpg_test_template_repeat_instance(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.c_uint64(count), pv,
                                                 C.c_void_p(row_ptr.ctypes.data), C.c_uint64(rows), C.c_void_p(tv.ctypes.data), C.c_void_p(tc.ctypes.data),
                                                 C.c_uint64(terms), coef, C.c_uint64(ncoef), C.byref(nnz), C.byref(nc)))
    return row_ptr, tv[:nnz.value].copy(), tc[:nnz.value].copy(), coef.raw[:32 * nc.value]


class TemplatePart(C.Structure):
    """bpg_template_part (frozen): one part of bpg_r1cs_template_join."""
    _fields_ = [("tmpl", C.c_void_p), ("count", C.c_uint64)]


class TestJoinPart(C.Structure):
    """bpg_test_join_part: one part of the join test hooks."""
    _fields_ = [("inst", C.POINTER(R1CSInstance)), ("program", C.POINTER(WitnessProgramView)), ("hints", C.POINTER(WitnessHintsView)),
                ("checkpoints", C.POINTER(WitnessCheckpointsView)), ("count", C.c_uint64)]


def join_layout(dims):
    """[(n, m, q, n_params, n_ck, count)] -> per part a dict of these and the five bases (base_n, base_m, base_q, base_n_params, base_n_ck): where the part's
    first copy starts in the joined multipliers, committed values, constraint rows, parameters and checkpoints (include/bpg.h bpg_r1cs_template_join)"""
    names = ("n", "m", "q", "n_params", "n_ck")
    base, out = dict.fromkeys(names + ("n_inputs",), 0), []
    for d in dims:
        part = dict(zip(names + ("count",), (int(x) for x in d)))
        if len(d) > 6:                      # Context.join_inputs: the public inputs of the part's template as well
            part["n_inputs"] = int(d[6])
        for k in names + (("n_inputs",) if len(d) > 6 else ()):
            part["base_" + k] = base[k]
            base[k] += part["count"] * part[k]
        out.append(part)
    return out


def _test_join_parts(parts):
    """[(inst, program, hints, count) or (inst, program, hints, count, checkpoint variables)] -> (bpg_test_join_part array, keep-alive, layout)"""
    arr, keep, dims = (TestJoinPart * max(len(parts), 1))(), [], []
    for k, part in enumerate(parts):
        inst, program, hints, count = part[:4]
        cks = list(part[4]) if len(part) > 4 and part[4] is not None else []
        cs, cp = inst.cstruct(), program.cstruct()
        ch = hints.cstruct() if hints is not None and len(hints) else None
        ck = _checkpoints_cstruct(cks) if cks else None
        keep.append((cs, cp, ch, ck))
        arr[k].inst, arr[k].program, arr[k].count = C.pointer(cs), C.pointer(cp), count
        if ch is not None:
            arr[k].hints = C.pointer(ch)
        if ck is not None:
            arr[k].checkpoints = C.pointer(ck)
        dims.append((inst.n, inst.m, inst.q, len(program.param_rows), len(cks), count))
    return arr, keep, dims


def test_template_join_instance(parts, param_values=None):
    """bpg_test_template_join_instance (no device): the instance of the templates joined - parts = [(inst, program, hints, count[, checkpoints])] - row-major, as
    it stands after an assign of param_values (the joined parameters in order; None: the constants of the templates' own rows) ->
    (row_ptr, term_var, term_coef, coef bytes)"""
    import numpy as np
    arr, keep, dims = _test_join_parts(parts)
    rows = sum(c * q for _, _, q, _, _, c in dims) + 1
    terms = sum(part[3] * (part[0].nnz + len(part[1].param_rows)) for part in parts)
    ncoef = sum(part[0].ncoef + part[3] * len(part[1].param_rows) for part in parts)
    npar = sum(c * p for _, _, _, p, _, c in dims)
    row_ptr, tv, tc, coef = np.zeros(rows, np.uint64), np.zeros(max(terms, 1), np.uint32), np.zeros(max(terms, 1), np.uint32), _buf(32 * ncoef)
    nnz, nc = C.c_uint64(), C.c_uint64()
    pv = None if param_values is None else _scalars32("param_values", param_values, npar)
    _chk(lib().bpg_test_template_join_instance(C.c_uint64(len(parts)), arr, pv, C.c_void_p(row_ptr.ctypes.data), C.c_uint64(rows), C.c_void_p(tv.ctypes.data),
                                               C.c_void_p(tc.ctypes.data), C.c_uint64(terms), coef, C.c_uint64(ncoef), C.byref(nnz), C.byref(nc)))
    return row_ptr, tv[:nnz.value].copy(), tc[:nnz.value].copy(), coef.raw[:32 * nc.value]


def test_template_eval_join(parts, values, ck_values=None):
    """bpg_test_template_eval_join (no device): the join-layout witness interpreter compiled for the host (levels in order; parts, segments and items of a level
    in reverse): the joined committed values (and checkpoint values) -> (a_L, a_R, a_O, first mismatching flat checkpoint index or None)"""
    arr, keep, dims = _test_join_parts(parts)
    n, m, nck = (sum(d[5] * d[i] for d in dims) for i in (0, 1, 4))
    out = [_buf(32 * n) for _ in range(3)]
    v = _scalars32("values", values, m)
    ck = None if ck_values is None else _scalars32("ck_values", ck_values, nck)
    first = C.c_uint64()
    _chk(lib().bpg_test_template_eval_join(C.c_uint64(len(parts)), arr, v if v else None, ck if ck else None, *out, C.byref(first)))
    return tuple(o.raw[:32 * n] for o in out) + (None if first.value == 2**64 - 1 else int(first.value),)


def test_template_eval_repeat(inst, program, hints, count, values):
    """bpg_test_template_eval_repeat (no device): the repeat-layout witness interpreter compiled for the host: count x m committed values ->
    (a_L, a_R, a_O) of count x n scalars each"""
    cs, cp = inst.cstruct(), program.cstruct()
    ch = hints.cstruct() if hints is not None and len(hints) else None
    out = [_buf(32 * count * inst.n) for _ in range(3)]
    v = _scalars32("values", values, count * inst.m)
    _chk(lib().bpg_test_template_eval_repeat(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.c_uint64(count), v if v else None, *out))
    return tuple(o.raw[:32 * count * inst.n] for o in out)


class TestJoinInputsPart(C.Structure):
    """bpg_test_join_inputs_part: one part of the join test hooks for programs with public inputs."""
    _fields_ = TestJoinPart._fields_ + [("n_inputs", C.c_uint64)]


def _hook_instance_buffers(rows, terms, ncoef, sizes=None):
    """the four output buffers of an instance hook at the sizes given (sizes = (rows, terms, ncoef) overrides the caller's formulas).  The arrays start as
    0xff so that a refused call can be shown to have written nothing."""
    import numpy as np
    if sizes is not None:
        rows, terms, ncoef = sizes
    return (np.full(max(rows, 1), 2**64 - 1, np.uint64), np.full(max(terms, 1), 2**32 - 1, np.uint32), np.full(max(terms, 1), 2**32 - 1, np.uint32),
            C.create_string_buffer(b"\xff" * (32 * max(ncoef, 1)), 32 * max(ncoef, 1)), rows, terms, ncoef)


def test_template_repeat_inputs_instance(inst, program, hints, n_inputs, count, param_values=None, input_values=None, n_slots=0, sizes=None, buffers=None):
    """bpg_test_template_repeat_inputs_instance (no device): test_template_repeat_instance for a template with n_inputs public inputs, as an assign of
    param_values and input_values (count x n_inputs scalars, item-major) leaves it.  n_slots: the template's derived slots (the coefficient table holds
    ncoef + count x (n_params + n_slots) scalars).  sizes = (row_ptr entries, term entries, coef scalars): the capacities to hand over instead of the
    formulas' own; buffers: a list that receives the four arrays -> (row_ptr, term_var, term_coef, coef bytes)"""
    cs, cp = inst.cstruct(), program.cstruct()
    cs.aL = cs.aR = cs.aO = None
    ch = hints.cstruct() if hints is not None and len(hints) else None
    npar = len(program.param_rows)
    row_ptr, tv, tc, coef, rows, terms, ncoef = _hook_instance_buffers(count * inst.q + 1, count * (inst.nnz + npar), inst.ncoef + count * (npar + n_slots), sizes)
    if buffers is not None:
        buffers += [row_ptr, tv, tc, coef]
    nnz, nc = C.c_uint64(), C.c_uint64()
    pv = None if param_values is None else _scalars32("param_values", param_values, count * npar)
    iv = None if input_values is None else _scalars32("input_values", input_values, count * n_inputs)
    _chk(lib().bpg_test_template_repeat_inputs_instance(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.c_uint64(n_inputs), C.c_uint64(count), pv, iv,
                                                        C.c_void_p(row_ptr.ctypes.data), C.c_uint64(rows), C.c_void_p(tv.ctypes.data), C.c_void_p(tc.ctypes.data),
                                                        C.c_uint64(terms), coef, C.c_uint64(ncoef), C.byref(nnz), C.byref(nc)))
    return row_ptr, tv[:nnz.value].copy(), tc[:nnz.value].copy(), coef.raw[:32 * nc.value]


def test_template_eval_repeat_inputs(inst, program, hints, checkpoints, n_inputs, count, values, ck_values=None, input_values=None):
    """bpg_test_template_eval_repeat_inputs (no device): the repeat-layout interpreter compiled for the host for a source with inputs and / or checkpoints
    (poisoned vectors; segments and items of a level in reverse) -> (a_L, a_R, a_O, first mismatching flat checkpoint index or None)"""
    cs, cp = inst.cstruct(), program.cstruct()
    cs.aL = cs.aR = cs.aO = None
    ch = hints.cstruct() if hints is not None and len(hints) else None
    cks = list(checkpoints or [])
    ck = _checkpoints_cstruct(cks) if cks else None
    out = [_buf(32 * count * inst.n) for _ in range(3)]
    v = _scalars32("values", values, count * inst.m)
    ckv = None if ck_values is None else _scalars32("ck_values", ck_values, count * len(cks))
    iv = None if input_values is None else _scalars32("input_values", input_values, count * n_inputs)
    first = C.c_uint64()
    _chk(lib().bpg_test_template_eval_repeat_inputs(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.byref(ck) if ck is not None else None,
                                                    C.c_uint64(n_inputs), C.c_uint64(count), v if v else None, ckv if ckv else None, iv if iv else None, *out,
                                                    C.byref(first)))
    return tuple(o.raw[:32 * count * inst.n] for o in out) + (None if first.value == 2**64 - 1 else int(first.value),)


def _test_join_inputs_parts(parts):
    """[(inst, program, hints, count, checkpoint variables or None, n_inputs)] -> (bpg_test_join_inputs_part array, keep-alive, layout dims with n_inputs last)"""
    arr, keep, dims = (TestJoinInputsPart * max(len(parts), 1))(), [], []
    for k, (inst, program, hints, count, cks, n_inputs) in enumerate(parts):
        cks = list(cks or [])
        cs, cp = inst.cstruct(), program.cstruct()
        cs.aL = cs.aR = cs.aO = None
        ch = hints.cstruct() if hints is not None and len(hints) else None
        ck = _checkpoints_cstruct(cks) if cks else None
        keep.append((cs, cp, ch, ck))
        arr[k].inst, arr[k].program, arr[k].count, arr[k].n_inputs = C.pointer(cs), C.pointer(cp), count, n_inputs
        if ch is not None:
            arr[k].hints = C.pointer(ch)
        if ck is not None:
            arr[k].checkpoints = C.pointer(ck)
        dims.append((inst.n, inst.m, inst.q, len(program.param_rows), len(cks), count, n_inputs))
    return arr, keep, dims


def test_template_join_inputs_instance(parts, param_values=None, input_values=None, n_slots=(), sizes=None, buffers=None):
    """bpg_test_template_join_inputs_instance (no device): test_template_join_instance where parts = [(inst, program, hints, count, checkpoints, n_inputs)]
    may have public inputs; input_values: the joined inputs, part-major then item-major; n_slots: per part the derived slots of its template.  Buffers of
    the sizes the formulas give (sizes / buffers as for the repeat hook) -> (row_ptr, term_var, term_coef, coef bytes)"""
    arr, keep, dims = _test_join_inputs_parts(parts)
    n_slots = list(n_slots) + [0] * (len(parts) - len(n_slots))
    rows = sum(d[5] * d[2] for d in dims) + 1
    terms = sum(part[3] * (part[0].nnz + len(part[1].param_rows)) for part in parts)
    ncoef = sum(part[0].ncoef + part[3] * (len(part[1].param_rows) + ns) for part, ns in zip(parts, n_slots))
    npar, nin = sum(d[5] * d[3] for d in dims), sum(d[5] * d[6] for d in dims)
    row_ptr, tv, tc, coef, rows, terms, ncoef = _hook_instance_buffers(rows, terms, ncoef, sizes)
    if buffers is not None:
        buffers += [row_ptr, tv, tc, coef]
    nnz, nc = C.c_uint64(), C.c_uint64()
    pv = None if param_values is None else _scalars32("param_values", param_values, npar)
    iv = None if input_values is None else _scalars32("input_values", input_values, nin)
    _chk(lib().bpg_test_template_join_inputs_instance(C.c_uint64(len(parts)), arr, pv, iv, C.c_void_p(row_ptr.ctypes.data), C.c_uint64(rows), C.c_void_p(tv.ctypes.data),
                                                      C.c_void_p(tc.ctypes.data), C.c_uint64(terms), coef, C.c_uint64(ncoef), C.byref(nnz), C.byref(nc)))
    return row_ptr, tv[:nnz.value].copy(), tc[:nnz.value].copy(), coef.raw[:32 * nc.value]


def test_template_eval_join_inputs(parts, values, ck_values=None, input_values=None):
    """bpg_test_template_eval_join_inputs (no device): test_template_eval_join where parts (as for test_template_join_inputs_instance) may have public inputs
    -> (a_L, a_R, a_O, first mismatching flat checkpoint index or None)"""
    arr, keep, dims = _test_join_inputs_parts(parts)
    n, m, nck, nin = (sum(d[5] * d[i] for d in dims) for i in (0, 1, 4, 6))
    out = [_buf(32 * n) for _ in range(3)]
    v = _scalars32("values", values, m)
    ck = None if ck_values is None else _scalars32("ck_values", ck_values, nck)
    iv = None if input_values is None else _scalars32("input_values", input_values, nin)
    first = C.c_uint64()
    _chk(lib().bpg_test_template_eval_join_inputs(C.c_uint64(len(parts)), arr, v if v else None, ck if ck else None, iv if iv else None, *out, C.byref(first)))
    return tuple(o.raw[:32 * n] for o in out) + (None if first.value == 2**64 - 1 else int(first.value),)


class VerifyItem(C.Structure):
    """bpg_verify_item (frozen): one proof of bpg_r1cs_verify_batch."""
    _fields_ = [("inst", C.POINTER(R1CSInstance)), ("circuit", C.c_void_p), ("transcript_state", C.c_void_p), ("m", C.c_uint64), ("V", C.c_char_p),
                ("proof", C.c_char_p), ("proof_len", C.c_uint64), ("seed", C.c_char_p), ("flags", C.c_uint32)]


class VerifyResidentItem(C.Structure):
    """bpg_verify_resident_item (frozen): one proof of bpg_r1cs_verify_resident_batch."""
    _fields_ = [("transcript_state", C.c_void_p), ("V", C.c_char_p), ("proof", C.c_char_p), ("proof_len", C.c_uint64), ("seed", C.c_char_p), ("flags", C.c_uint32),
                ("param_values", C.c_char_p), ("input_values", C.c_char_p)]


def _verify_items(items):
    """[(FlatInstance | ResidentCircuit, transcript_state, commitments, proof, seed=None, flags=0)] -> (VerifyItem array, state buffers, keep-alive)"""
    n = len(items)
    arr = (VerifyItem * max(n, 1))()
    states, keep = [], []
    for k, it in enumerate(items):
        target, state, coms, proof = it[0], it[1], it[2], it[3]
        seed = _seed32(it[4] if len(it) > 4 else None)
        flags = it[5] if len(it) > 5 else 0
        ts = _buf(203); ts.raw = _exact("transcript_state", state, 203)
        coms, proof = _exact("commitments", coms, 32 * target.m), bytes(proof)
        if isinstance(target, ResidentCircuit):
            arr[k].circuit = target._h
        else:
            cs = target.cstruct()
            cs.aL = cs.aR = cs.aO = None                        # verifier side: no assignments
            arr[k].inst = C.pointer(cs)
            keep.append(cs)
        arr[k].transcript_state = C.cast(ts, C.c_void_p); arr[k].m = target.m; arr[k].V = coms
        arr[k].proof = proof; arr[k].proof_len = len(proof); arr[k].seed = seed; arr[k].flags = flags
        states.append(ts); keep.append((coms, proof, seed))
    return arr, states, keep


def _context_verify_batch(self, items, batch_seed=None, return_status=False):
    """bpg_r1cs_verify_batch: items = [(FlatInstance | ResidentCircuit, transcript_state, commitments, proof, seed=None, flags=0)] ->
    (statuses, transcript states after); each status is what verify_flat / ResidentCircuit.verify gives for that item alone.  All items go into ONE
    multiscalar multiplication with random weights (batch_seed: fresh randomness unless pinned).  return_status=True: (call status, statuses, states).
    A refused call (INVALID_ARGUMENT) or a device failure raises BpgError."""
    arr, states, keep = _verify_items(items)
    n = len(items)
    status = (C.c_int32 * max(n, 1))()
    rc = lib().bpg_r1cs_verify_batch(self._h, C.c_uint64(n), arr, _seed32(batch_seed), status)
    if rc not in (0, 1, 2, 3):
        _chk(rc)
    out = ([status[k] for k in range(n)], [ts.raw[:203] for ts in states])
    return (rc,) + out if return_status else out


Context.verify_batch = _context_verify_batch


def _context_test_verify_batch_scripted(self, items, scripts, batch_seed=None):
    """bpg_test_verify_batch_scripted: verify_batch(items) with item k's transcript handing out scripts[k] (the weights stay real) ->
    (call status, statuses, transcript states after).  A scripted acceptance says nothing about a statement.  A refused call raises BpgError."""
    if len(scripts) != len(items):
        raise ValueError("one script per item")
    arr, states, keep = _verify_items(items)
    ptrs, lens, keep2 = _script_arrays(scripts)
    n = len(items)
    status = (C.c_int32 * max(n, 1))()
    rc = lib().bpg_test_verify_batch_scripted(self._h, C.c_uint64(n), arr, ptrs, lens, _seed32(batch_seed), status)
    if rc not in (0, 1, 2, 3):
        _chk(rc)
    return rc, [status[k] for k in range(n)], [ts.raw[:203] for ts in states]


Context.test_verify_batch_scripted = _context_test_verify_batch_scripted


def _context_join(self, parts):
    """bpg_r1cs_template_join: parts = [(template, count)] -> ONE resident template that holds count_0 copies of part 0, then count_1 of part 1, ... - the
    circuit of one host assembly of the parts' gadget code in that order, made on the device from the resident templates (a mixed statement, one proof).
    .layout lists per part n, m, q, n_params, n_ck, count and the bases of its first copy (join_layout).  assign(values, params, checkpoints=) takes the
    concatenated lists, part-major then item-major; CheckReport.parts(layout) maps the rows of check() back.  Independent of its sources."""
    parts = [(t, int(c)) for t, c in parts]
    arr = (TemplatePart * max(len(parts), 1))()
    for k, (t, c) in enumerate(parts):
        if c < 0 or c >= 2**64:
            raise ValueError("count out of range")
        arr[k].tmpl, arr[k].count = (t._h if t is not None else None), c
    h = C.c_void_p()
    _chk(lib().bpg_r1cs_template_join(self._h, C.c_uint64(len(parts)), arr, C.byref(h)))
    layout = join_layout([(t.n, t.m, t.q or 0, t.n_params, t.n_ck, c) for t, c in parts])
    tot = lambda k: sum(p["count"] * p[k] for p in layout)
    res = ResidentCircuit(self, h, tot("n"), tot("m"), n_params=tot("n_params"), q=None if any(t.q is None for t, _ in parts) else tot("q"), n_ck=tot("n_ck"))
    res.layout = layout
    return res


Context.join = _context_join


def _context_join_inputs(self, parts):
    """bpg_r1cs_template_join_inputs: Context.join where any part may be a template with public inputs.  .layout also carries n_inputs and base_n_inputs per
    part; assign(values, params, checkpoints=, inputs=) takes the concatenated lists, part-major then item-major.  Without inputs in any part it is join()."""
    parts = [(t, int(c)) for t, c in parts]
    arr = (TemplatePart * max(len(parts), 1))()
    for k, (t, c) in enumerate(parts):
        if c < 0 or c >= 2**64:
            raise ValueError("count out of range")
        arr[k].tmpl, arr[k].count = (t._h if t is not None else None), c
    h = C.c_void_p()
    _chk(lib().bpg_r1cs_template_join_inputs(self._h, C.c_uint64(len(parts)), arr, C.byref(h)))
    layout = join_layout([(t.n, t.m, t.q or 0, t.n_params, t.n_ck, c, t.n_inputs) for t, c in parts])
    tot = lambda k: sum(p["count"] * p[k] for p in layout)
    res = ResidentCircuit(self, h, tot("n"), tot("m"), n_params=tot("n_params"), q=None if any(t.q is None for t, _ in parts) else tot("q"), n_ck=tot("n_ck"),
                          n_inputs=tot("n_inputs"))
    res.layout = layout
    return res


Context.join_inputs = _context_join_inputs


def verify_batch(ctx, verifiers, proofs, bp_gens, seeds=None, flags=0, batch_seed=None):
    """Verifier::verify of many bpg.Verifier objects in one bpg_r1cs_verify_batch call -> list of statuses (0 accepted, 1 INVALID_GENERATORS_LENGTH,
    2 FORMAT_ERROR, 3 VERIFICATION_ERROR), each what Verifier.verify(proof, ctx, bp_gens, seed, flags) decides alone.  The verifiers' own
    transcripts are left as they are."""
    capacity = bp_gens.gens_capacity if isinstance(bp_gens, BulletproofGens) else int(bp_gens)
    ctx.gens_ensure(capacity)
    statuses, items, where = [None] * len(verifiers), [], []
    for k, (v, proof) in enumerate(zip(verifiers, proofs)):
        inst = v.instance()
        N = 1
        while N < inst.n:
            N *= 2
        if capacity < N:
            statuses[k] = 1
            continue
        items.append((inst, v.transcript.state, inst.commitments, proof, seeds[k] if seeds else None, flags))
        where.append(k)
    if items:
        st, _ = ctx.verify_batch(items, batch_seed)
        for k, s in zip(where, st):
            statuses[k] = s
    return statuses


class _BatchItem(C.Structure):
    _fields_ = [("inst", C.POINTER(R1CSInstance)), ("transcript_state", C.c_void_p), ("m", C.c_uint64), ("v_blinding", C.c_char_p),
                ("rng_seed", C.c_char_p), ("flags", C.c_uint32), ("proof_out", C.c_void_p), ("proof_len", C.POINTER(C.c_uint64))]


def _batch_items(items):
    """bpg_batch_item array of [(FlatInstance, transcript_state, v_blinding, rng_seed, flags)] and the buffers it points into:
    (instance, transcript state, proof buffer, proof length, v_blinding, seed) per item"""
    n = len(items)
    arr = (_BatchItem * max(n, 1))()
    keep = []
    for k, (inst, state, vb, seed, flags) in enumerate(items):
        cs = inst.cstruct()
        ts = _buf(203); ts.raw = bytes(state)
        cap = lib().bpg_proof_size(inst.n, flags)
        out = _buf(cap); ln = C.c_uint64(cap)
        keep.append((cs, ts, out, ln, vb, seed))
        arr[k].inst = C.pointer(cs); arr[k].transcript_state = C.cast(ts, C.c_void_p); arr[k].m = inst.m
        arr[k].v_blinding = vb; arr[k].rng_seed = seed; arr[k].flags = flags
        arr[k].proof_out = C.cast(out, C.c_void_p); arr[k].proof_len = C.pointer(ln)
    return arr, keep


def _context_prove_batch(self, items, return_status=False):
    """bpg_r1cs_prove_batch: items = [(FlatInstance, transcript_state, v_blinding, rng_seed, flags)] (as ProverPool.prove_batch) ->
    [(proof, transcript state after)], each exactly what prove_flat gives for that item alone; small circuits (N <= 2^14) share every launch.
    Raises BpgError on the first failing item; return_status=True returns (results, statuses) instead, with (None, state as given) for a failed item."""
    arr, keep = _batch_items(items)
    n = len(items)
    status = (C.c_int32 * max(n, 1))()
    rc = lib().bpg_r1cs_prove_batch(self._h, C.c_uint64(n), arr, status)
    if not return_status:
        _chk(rc)
    st = [status[k] for k in range(n)]
    res = [(k[2].raw[:k[3].value] if s == 0 else None, k[1].raw[:203]) for k, s in zip(keep, st)]
    return (res, st) if return_status else res


Context.prove_batch = _context_prove_batch


def _context_test_prove_batch_scripted(self, items, scripts):
    """bpg_test_prove_batch_scripted: prove_batch(items), every item in lockstep, with item k's transcript handing out scripts[k] ->
    [(proof, transcript state after)].  NOT sound proofs.  Raises BpgError: a script the hook refuses or an item off the lockstep path refuses the whole call."""
    if len(scripts) != len(items):
        raise ValueError("one script per item")
    arr, keep = _batch_items(items)
    ptrs, lens, keep2 = _script_arrays(scripts)
    n = len(items)
    status = (C.c_int32 * max(n, 1))()
    _chk(lib().bpg_test_prove_batch_scripted(self._h, C.c_uint64(n), arr, ptrs, lens, status))
    return [(k[2].raw[:k[3].value], k[1].raw[:203]) for k in keep]


Context.test_prove_batch_scripted = _context_test_prove_batch_scripted


class ProverPool:
    """bpg_pool_*: `workers` engine contexts + host threads on one GPU that prove a batch of independent instances concurrently (the
    serial TranscriptRng chain of one proof overlaps the kernels of the others). Same bytes as proving the items one by one."""

    def __init__(self, device: int = 0, workers: int = 8, gens_capacity: int = 0, profile=None, **config):
        self._h = C.c_void_p()
        cfg = make_config(profile, **config) if (profile is not None or config) else None
        _chk(lib().bpg_pool_create_ex(C.c_int32(device), C.c_uint32(workers), C.c_uint64(gens_capacity), C.byref(cfg) if cfg is not None else None, C.byref(self._h)))
        self.workers = workers

    def prove_batch(self, items):
        """items: [(FlatInstance, transcript_state, v_blinding, rng_seed, flags)] -> [(proof bytes, transcript state after)]"""
        arr, keep = _batch_items(items)
        status = (C.c_int32 * max(len(items), 1))()
        _chk(lib().bpg_pool_prove(self._h, C.c_uint64(len(items)), arr, status))
        return [(k[2].raw[:k[3].value], k[1].raw[:203]) for k in keep]

    def close(self):
        if getattr(self, "_h", None):
            lib().bpg_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TemplateItem(C.Structure):
    _fields_ = [("v", C.c_char_p), ("param_values", C.c_char_p), ("transcript_state", C.c_void_p), ("v_blinding", C.c_char_p),
                ("rng_seed", C.c_char_p), ("flags", C.c_uint32), ("proof_out", C.c_void_p), ("proof_len", C.POINTER(C.c_uint64))]


class _TemplateCommitItem(C.Structure):
    """bpg_template_commit_item (frozen): bpg_template_item and the buffer of the item's commitments."""
    _fields_ = _TemplateItem._fields_ + [("commitments_out", C.c_void_p)]


class _TemplateCkItem(C.Structure):
    """bpg_template_ck_item (frozen): bpg_template_commit_item, the item's checkpoint values and where its lowest mismatch goes."""
    _fields_ = _TemplateCommitItem._fields_ + [("ck_values", C.c_char_p), ("first_mismatch", C.POINTER(C.c_uint64))]


class _TemplateInItem(C.Structure):
    """bpg_template_in_item (frozen): bpg_template_ck_item and the item's public input values."""
    _fields_ = _TemplateCkItem._fields_ + [("input_values", C.c_char_p)]


class ResidentCircuit:
    def __init__(self, ctx, h, n, m, n_params=None, q=None, n_ck=0, n_inputs=0):
        self.ctx, self._h, self.n, self.m = ctx, h, n, m
        self.n_inputs = n_inputs            # public input values assign() takes (a template uploaded with inputs: Prover.input)
        self.n_ck = n_ck                    # checkpoint values assign() takes (a template uploaded with checkpoints; a repeat of one: count x as many)
        self.n_params = n_params            # None: a plain upload; a number: a circuit template (Prover.template / Context.upload_template)
        self.q = q                          # constraint rows (None: made by a caller that did not say)
        self.layout = None                  # Context.join: the parts of the join and where each starts (join_layout)

    def assign(self, values, params=(), checkpoints=None, inputs=None):
        """bpg_r1cs_assign: a fresh witness for a circuit template - the m committed values (and the constant term of every parameter row); the device
        computes a_L, a_R, a_O.  The caller commits to the same values and proves with prove().
        checkpoints (bpg_r1cs_assign_checkpointed, a template uploaded with checkpoints): their values, in the order they were named (a repeat: item-major).
        A value that is not what the circuit computes raises BpgError(CHECKPOINT_MISMATCH) whose .first_mismatch is the lowest such flat index; the circuit
        then holds no witness.
        inputs (bpg_r1cs_assign_inputs, a template with public inputs): their values in input order - the bound, the set, the siblings of THIS proof."""
        v = _scalars32("values", values, self.m)
        pv = bytes(params) if isinstance(params, (bytes, bytearray)) else b"".join(_exact("params", x, 32) for x in params)
        if len(pv) % 32:
            raise ValueError("params must be a multiple of 32 bytes")
        if inputs is not None:
            iv = bytes(inputs) if isinstance(inputs, (bytes, bytearray)) else b"".join(_exact("inputs", x, 32) for x in inputs)
            if len(iv) % 32:
                raise ValueError("inputs must be a multiple of 32 bytes")
            ck = b"" if checkpoints is None else (bytes(checkpoints) if isinstance(checkpoints, (bytes, bytearray)) else b"".join(_exact("checkpoints", x, 32) for x in checkpoints))
            if len(ck) % 32:
                raise ValueError("checkpoints must be a multiple of 32 bytes")
            first = C.c_uint64()
            st = lib().bpg_r1cs_assign_inputs(self.ctx._h, self._h, C.c_uint64(self.m), v if self.m else None, C.c_uint64(len(pv) // 32), pv if pv else None,
                                              C.c_uint64(len(ck) // 32), ck if ck else None, C.byref(first), C.c_uint64(len(iv) // 32), iv if iv else None)
            if st != 0:
                e = BpgError(st, lib().bpg_last_error().decode())
                if st == ERR_CHECKPOINT_MISMATCH:
                    e.first_mismatch = int(first.value)
                    if self.layout is not None:             # a join: (part, item, checkpoint of the part's template); the message names them too
                        e.place = _join_place(self.layout, e.first_mismatch, "n_ck")
                raise e
            return
        if checkpoints is not None:
            ck = bytes(checkpoints) if isinstance(checkpoints, (bytes, bytearray)) else b"".join(_exact("checkpoints", x, 32) for x in checkpoints)
            if len(ck) % 32:
                raise ValueError("checkpoints must be a multiple of 32 bytes")
            first = C.c_uint64()
            st = lib().bpg_r1cs_assign_checkpointed(self.ctx._h, self._h, C.c_uint64(self.m), v if self.m else None, C.c_uint64(len(pv) // 32), pv if pv else None,
                                                    C.c_uint64(len(ck) // 32), ck if ck else None, C.byref(first))
            if st != 0:
                e = BpgError(st, lib().bpg_last_error().decode())
                if st == ERR_CHECKPOINT_MISMATCH:
                    e.first_mismatch = int(first.value)
                    if self.layout is not None:             # a join: (part, item, checkpoint of the part's template); the message names them too
                        e.place = _join_place(self.layout, e.first_mismatch, "n_ck")
                raise e
            return
        _chk(lib().bpg_r1cs_assign(self.ctx._h, self._h, C.c_uint64(self.m), v if self.m else None, C.c_uint64(len(pv) // 32), pv if pv else None))

    def repeat(self, count) -> "ResidentCircuit":
        """bpg_r1cs_template_repeat: this template `count` times over as ONE resident template - the circuit of `count` host assemblies of the same gadget
        code in one prover, replicated on the device (item k at multipliers k n.., committed values k m.., parameters k n_params..).  assign() then takes
        count x m values and count x n_params constants, item-major; one prove() gives one proof for all the items.  Independent of this template.
        Refused on a repeat and on a join (Context.join with larger counts is that circuit); check_batch, which repeats, with it."""
        h = C.c_void_p()
        _chk(lib().bpg_r1cs_template_repeat(self.ctx._h, self._h, C.c_uint64(count), C.byref(h)))
        return ResidentCircuit(self.ctx, h, count * self.n, count * self.m, n_params=count * self.n_params, q=None if self.q is None else count * self.q,
                               n_ck=count * self.n_ck)

    def repeat_inputs(self, count) -> "ResidentCircuit":
        """bpg_r1cs_template_repeat_inputs: repeat() for a template with public inputs - `count` statements against `count` different public values as ONE
        proof.  assign(values, params, checkpoints=, inputs=) then takes count x n_inputs inputs as well, item-major.  Without inputs it is repeat()."""
        h = C.c_void_p()
        _chk(lib().bpg_r1cs_template_repeat_inputs(self.ctx._h, self._h, C.c_uint64(count), C.byref(h)))
        return ResidentCircuit(self.ctx, h, count * self.n, count * self.m, n_params=count * self.n_params, q=None if self.q is None else count * self.q,
                               n_ck=count * self.n_ck, n_inputs=count * self.n_inputs)

    def set_inputs(self, inputs):
        """bpg_r1cs_set_inputs: the verifier's half of assign(inputs=) - the public inputs go up and the derived coefficient slots are filled, nothing else.
        The circuit is left without a witness; verify() then checks against these inputs."""
        iv = bytes(inputs) if isinstance(inputs, (bytes, bytearray)) else b"".join(_exact("inputs", x, 32) for x in inputs)
        if len(iv) % 32:
            raise ValueError("inputs must be a multiple of 32 bytes")
        _chk(lib().bpg_r1cs_set_inputs(self.ctx._h, self._h, C.c_uint64(len(iv) // 32), iv if iv else None))

    def check_batch_inputs(self, items, max_rows=16):
        """check_batch for a template with public inputs: items = [(values, params, inputs)] -> per item the violated rows OF THE TEMPLATE.  Composition of
        repeat_inputs(), assign(inputs=) and ONE check() per chunk; this template's own witness and inputs are left alone."""
        if self.q is None:
            raise ValueError("check_batch_inputs needs the template's row count (a circuit from Context.upload_template or Prover.template)")
        out = []
        per = max(1, self.CHECK_BATCH_ROWS // max(self.q, 1))
        join = lambda x: bytes(x) if isinstance(x, (bytes, bytearray)) else b"".join(bytes(y) for y in x)
        for first in range(0, len(items), per):
            chunk = items[first:first + per]
            rep = self.repeat_inputs(len(chunk))
            try:
                rep.assign(b"".join(join(v) for v, _, _ in chunk), b"".join(join(p) for _, p, _ in chunk), inputs=b"".join(join(i) for _, _, i in chunk))
                found = [[] for _ in chunk]
                for k, r in rep.check(None, len(chunk) * self.q).items(self.q):
                    if len(found[k]) < max_rows:
                        found[k].append(r)
                out += found
            finally:
                rep.free()
        return out

    def check(self, values=None, max_rows=16) -> "CheckReport":
        """bpg_r1cs_check: which multipliers (a_L * a_R against a_O) and which constraint rows does the resident witness break - evaluated on the device, the
        witness stays where it is.  values: the m committed values (a plain upload does not keep them); None on a template: those of the last assign().
        max_rows: how many violated rows to list (the lowest, ascending); the counts are exact whatever it is.  An unsatisfying witness is no error."""
        v = None if values is None else _scalars32("values", values, self.m)
        rows = (C.c_uint64 * max(max_rows, 1))()
        have, rep = C.c_uint64(), CheckReportView()
        _chk(lib().bpg_r1cs_check(self.ctx._h, self._h, C.c_uint64(self.m), v if v else None, C.c_uint64(max_rows), rows if max_rows else None, C.byref(have), C.byref(rep)))
        return CheckReport(rep, rows[:have.value])

    CHECK_BATCH_ROWS = 1 << 22      # constraint rows of one repeat made by check_batch

    def check_batch(self, items, max_rows=16):
        """"Which of my witnesses is bad": items = [(values, params)] - fresh witnesses of this template -> per item the list of violated rows OF THE TEMPLATE
        (ascending, at most max_rows each; empty: the item is satisfying).  Composition of repeat(), assign() and ONE check() per chunk of at most
        CHECK_BATCH_ROWS constraint rows; this template's own witness is left alone."""
        if self.q is None:
            raise ValueError("check_batch needs the template's row count (a circuit from Context.upload_template or Prover.template)")
        out = []
        per = max(1, self.CHECK_BATCH_ROWS // max(self.q, 1))
        join = lambda x: bytes(x) if isinstance(x, (bytes, bytearray)) else b"".join(bytes(y) for y in x)
        for first in range(0, len(items), per):
            chunk = items[first:first + per]
            rep = self.repeat(len(chunk))
            try:
                rep.assign(b"".join(join(v) for v, _ in chunk), b"".join(join(p) for _, p in chunk))
                found = [[] for _ in chunk]
                for k, r in rep.check(None, len(chunk) * self.q).items(self.q):
                    if len(found[k]) < max_rows:
                        found[k].append(r)
                out += found
            finally:
                rep.free()
        return out

    def prove(self, transcript_state, v_blinding, rng_seed=None, flags=0, timings=False):
        ts = _buf(203); ts.raw = _exact("transcript_state", transcript_state, 203)
        v_blinding, rng_seed = _exact("v_blinding", v_blinding, 32 * self.m), _seed32(rng_seed)
        cap = lib().bpg_proof_size(self.n, flags)
        out = _buf(cap); ln = C.c_uint64(cap)
        tm = Timings()
        _chk(lib().bpg_r1cs_prove_resident(self.ctx._h, self._h, ts, C.c_uint64(self.m), v_blinding, rng_seed, C.c_uint32(flags),
                                           out, C.byref(ln), C.byref(tm) if timings else None))
        return (out.raw[:ln.value], ts.raw[:203], tm.as_dict()) if timings else (out.raw[:ln.value], ts.raw[:203])

    def test_prove_scripted(self, transcript_state, v_blinding, script, rng_seed=None, flags=0):
        """bpg_test_prove_scripted: prove() with the transcript handing out `script` (y, z, u, x, w, u_1 .. u_lgN) -> (proof, state after).  NOT a sound proof."""
        ts = _buf(203); ts.raw = _exact("transcript_state", transcript_state, 203)
        v_blinding, rng_seed = _exact("v_blinding", v_blinding, 32 * self.m), _seed32(rng_seed)
        cap = lib().bpg_proof_size(self.n, flags)
        out = _buf(cap); ln = C.c_uint64(cap)
        sb, sn = _script_bytes(script)
        _chk(lib().bpg_test_prove_scripted(self.ctx._h, self._h, ts, C.c_uint64(self.m), v_blinding, rng_seed, C.c_uint32(flags), sb, C.c_uint64(sn), out, C.byref(ln)))
        return out.raw[:ln.value], ts.raw[:203]

    def test_verify_scripted(self, transcript_state, commitments, proof, script, seed=None, flags=0):
        """bpg_test_verify_scripted: verify() with the transcript handing out `script` -> (status as verify() gives it, state after).  Raises BpgError for a
        refused script."""
        ts = _buf(203); ts.raw = _exact("transcript_state", transcript_state, 203)
        seed, commitments, proof = _seed32(seed), _exact("commitments", commitments, 32 * self.m), bytes(proof)
        sb, sn = _script_bytes(script)
        rc = lib().bpg_test_verify_scripted(self.ctx._h, self._h, ts, C.c_uint64(self.m), commitments, proof, C.c_uint64(len(proof)), seed, C.c_uint32(flags),
                                            sb, C.c_uint64(sn))
        if rc not in (0, 1, 2, 3):
            _chk(rc)
        return rc, ts.raw[:203]

    def test_weights(self, z):
        """bpg_test_weights: the verifier's flattened weights of this circuit at z (32 canonical bytes), through the code verify() runs ->
        (w_L, w_R, w_O, w_V as lists of 32-byte scalars, w_c)."""
        n, m = self.n, self.m
        out = _buf(32 * (3 * n + m + 1))
        _chk(lib().bpg_test_weights(self.ctx._h, self._h, None if z is None else _exact("z", z, 32), out))
        w = [out.raw[32 * k:32 * k + 32] for k in range(3 * n + m + 1)]
        return w[:n], w[n:2 * n], w[2 * n:3 * n], w[3 * n:3 * n + m], w[3 * n + m]

    def _template_items(self, items, struct=_TemplateItem):
        """bpg_template_item array of [(values, params, transcript_state, v_blinding, rng_seed, flags)] and the buffers it points into:
        (transcript state, proof buffer, proof length, values, params, v_blinding, seed) per item.  values / params of None stay NULL.
        struct=_TemplateCommitItem: the same fields in a bpg_template_commit_item array (commitments_out left NULL)."""
        arr = (struct * max(len(items), 1))()
        keep = []
        for k, (values, params, state, vb, seed, flags) in enumerate(items):
            v = None if values is None else bytes(values)
            pv = None if params is None else (bytes(params) if isinstance(params, (bytes, bytearray)) else b"".join(_exact("params", x, 32) for x in params))
            ts = _buf(203); ts.raw = bytes(state)
            cap = lib().bpg_proof_size(self.n, flags)
            out = _buf(cap); ln = C.c_uint64(cap)
            keep.append((ts, out, ln, v, pv, vb, seed))
            arr[k].v = v; arr[k].param_values = pv if pv else None; arr[k].transcript_state = C.cast(ts, C.c_void_p)
            arr[k].v_blinding = vb; arr[k].rng_seed = seed; arr[k].flags = flags
            arr[k].proof_out = C.cast(out, C.c_void_p); arr[k].proof_len = C.pointer(ln)
        return arr, keep

    def prove_batch(self, items, return_status=False):
        """bpg_r1cs_prove_template_batch: items = [(values, params, transcript_state, v_blinding, rng_seed, flags)] - fresh witnesses of this template ->
        [(proof, transcript state after)], each exactly what assign(values, params) + prove(...) gives for that item alone; a template of N <= 2^14
        computes all the witnesses in shared launches.  The template holds no witness afterwards.  Raises BpgError on the first failing item;
        return_status=True returns (results, statuses) instead, with (None, state as given) for a failed item (the conventions of Context.prove_batch)."""
        arr, keep = self._template_items(items)
        n = len(items)
        status = (C.c_int32 * max(n, 1))()
        rc = lib().bpg_r1cs_prove_template_batch(self.ctx._h, self._h, C.c_uint64(n), arr, status)
        if not return_status:
            _chk(rc)
        st = [status[k] for k in range(n)]
        res = [(k[1].raw[:k[2].value] if s == 0 else None, k[0].raw[:203]) for k, s in zip(keep, st)]
        return (res, st) if return_status else res

    def prove_batch_commit(self, items, return_status=False):
        """bpg_r1cs_prove_template_batch_commit: items = [(values, params, state_before_commitments, blindings, rng_seed, flags)] ->
        [(proof, transcript state after, commitments)]: prove_batch that makes the m Pedersen commitments of every item itself (a wave's in one launch)
        and appends them to the item's transcript as "V", as Prover.commit does, before it proves.  commitments: m x 32 bytes in commit order.  Raises
        BpgError on the first failing item; return_status=True returns (results, statuses) instead, with (None, state as given, None) for a failed item."""
        arr, keep = self._template_items(items, _TemplateCommitItem)
        n = len(items)
        coms = [_buf(32 * self.m) for _ in range(n)]
        for k in range(n):
            arr[k].commitments_out = C.cast(coms[k], C.c_void_p)
        status = (C.c_int32 * max(n, 1))()
        rc = lib().bpg_r1cs_prove_template_batch_commit(self.ctx._h, self._h, C.c_uint64(n), arr, status)
        if not return_status:
            _chk(rc)
        st = [status[k] for k in range(n)]
        res = [(k[1].raw[:k[2].value], k[0].raw[:203], c.raw[:32 * self.m]) if s == 0 else (None, k[0].raw[:203], None) for k, c, s in zip(keep, coms, st)]
        return (res, st) if return_status else res

    def prove_batch_checkpointed(self, items, commit=False, return_status=False):
        """bpg_r1cs_prove_template_batch_checkpointed: items = [(values, params, transcript_state, v_blinding, rng_seed, flags, checkpoints)] - fresh witnesses
        of this checkpointed template, each with what assign(checkpoints=...) takes -> [(proof, transcript state after)], or with commit=True (the state comes
        in BEFORE the commitments, as for prove_batch_commit) [(proof, transcript state after, commitments)]: each exactly what assign + prove give for that
        item alone, the witnesses of a wave evaluated in the one or two levels of the checkpointed schedule.  The template holds no witness afterwards.
        Raises BpgError on the first failing item; a checkpoint mismatch carries .item and .first_mismatch (the item's lowest bad checkpoint).
        return_status=True returns (results, statuses, first_mismatches) instead, with (None, state as given[, None]) for a failed item and None for an
        item without a mismatch.  On a template without checkpoints: prove_batch / prove_batch_commit (checkpoints of None or empty)."""
        arr, keep = self._template_items([it[:6] for it in items], _TemplateCkItem)
        n = len(items)
        coms = [_buf(32 * self.m) for _ in range(n)] if commit else []
        firsts = [C.c_uint64(2**64 - 1) for _ in range(n)]
        cks = []
        for k in range(n):
            ck = items[k][6]
            ck = None if ck is None else (bytes(ck) if isinstance(ck, (bytes, bytearray)) else b"".join(_exact("checkpoints", x, 32) for x in ck))
            cks.append(ck)
            arr[k].ck_values = ck if ck else None
            arr[k].first_mismatch = C.pointer(firsts[k])
            if commit:
                arr[k].commitments_out = C.cast(coms[k], C.c_void_p)
        status = (C.c_int32 * max(n, 1))()
        rc = lib().bpg_r1cs_prove_template_batch_checkpointed(self.ctx._h, self._h, C.c_uint64(n), arr, C.c_int32(1 if commit else 0), status)
        st = [status[k] for k in range(n)]
        first = [None if f.value == 2**64 - 1 else int(f.value) for f in firsts]
        bad = [k for k in range(n) if st[k] != 0]
        if rc != 0 and not (return_status and bad):
            e = BpgError(rc, lib().bpg_last_error().decode())
            if bad:                                             # (a whole-call refusal fills no status)
                e.item = bad[0]
                if st[bad[0]] == ERR_CHECKPOINT_MISMATCH:
                    e.first_mismatch = first[bad[0]]
            raise e
        res = []
        for k in range(n):
            ts, out, ln = keep[k][:3]
            if st[k] != 0:
                res.append((None, ts.raw[:203], None) if commit else (None, ts.raw[:203]))
            elif commit:
                res.append((out.raw[:ln.value], ts.raw[:203], coms[k].raw[:32 * self.m]))
            else:
                res.append((out.raw[:ln.value], ts.raw[:203]))
        return (res, st, first) if return_status else res

    def prove_batch_inputs(self, items, commit=False, return_status=False):
        """bpg_r1cs_prove_template_batch_inputs: prove_batch_checkpointed for a template with public inputs - items = [(values, params, transcript_state,
        v_blinding, rng_seed, flags, checkpoints, inputs)], inputs what assign(inputs=...) takes for that item (checkpoints None on a template without).
        Results, errors and return_status as for prove_batch_checkpointed; on a template without inputs it is that call."""
        arr, keep = self._template_items([it[:6] for it in items], _TemplateInItem)
        n = len(items)
        coms = [_buf(32 * self.m) for _ in range(n)] if commit else []
        firsts = [C.c_uint64(2**64 - 1) for _ in range(n)]
        held = []
        join = lambda name, x: None if x is None else (bytes(x) if isinstance(x, (bytes, bytearray)) else b"".join(_exact(name, y, 32) for y in x))
        for k in range(n):
            ck, iv = join("checkpoints", items[k][6]), join("inputs", items[k][7])
            held.append((ck, iv))
            arr[k].ck_values = ck if ck else None
            arr[k].input_values = iv if iv else None
            arr[k].first_mismatch = C.pointer(firsts[k])
            if commit:
                arr[k].commitments_out = C.cast(coms[k], C.c_void_p)
        status = (C.c_int32 * max(n, 1))()
        rc = lib().bpg_r1cs_prove_template_batch_inputs(self.ctx._h, self._h, C.c_uint64(n), arr, C.c_int32(1 if commit else 0), status)
        st = [status[k] for k in range(n)]
        first = [None if f.value == 2**64 - 1 else int(f.value) for f in firsts]
        bad = [k for k in range(n) if st[k] != 0]
        if rc != 0 and not (return_status and bad):
            e = BpgError(rc, lib().bpg_last_error().decode())
            if bad:                                             # (a whole-call refusal fills no status)
                e.item = bad[0]
                if st[bad[0]] == ERR_CHECKPOINT_MISMATCH:
                    e.first_mismatch = first[bad[0]]
            raise e
        res = []
        for k in range(n):
            ts, out, ln = keep[k][:3]
            if st[k] != 0:
                res.append((None, ts.raw[:203], None) if commit else (None, ts.raw[:203]))
            elif commit:
                res.append((out.raw[:ln.value], ts.raw[:203], coms[k].raw[:32 * self.m]))
            else:
                res.append((out.raw[:ln.value], ts.raw[:203]))
        return (res, st, first) if return_status else res

    def verify(self, transcript_state, commitments, proof, seed=None, flags=0):
        """bpg_r1cs_verify_resident: 0 = accepted, 3 = VERIFICATION_ERROR, 2 = FORMAT_ERROR, 1 = INVALID_GENERATORS_LENGTH."""
        ts = _buf(203); ts.raw = _exact("transcript_state", transcript_state, 203)
        seed, commitments, proof = _seed32(seed), _exact("commitments", commitments, 32 * self.m), bytes(proof)
        return lib().bpg_r1cs_verify_resident(self.ctx._h, self._h, ts, C.c_uint64(self.m), commitments, proof, C.c_uint64(len(proof)), seed, C.c_uint32(flags))

    def verify_batch(self, items, batch_seed=None, return_status=False):
        """bpg_r1cs_verify_resident_batch: K proofs of THIS circuit in lockstep launches.  items = [(transcript_state, commitments, proof, seed=None, flags=0,
        params=None, inputs=None)]; params / inputs: the item's own parameter values (n_params x 32 bytes) and public inputs (n_inputs x 32 bytes), or None for
        the circuit's standing slots (a single template only) -> (statuses, transcript states after), each status what verify() gives for that item alone with
        its constants standing.  return_status=True: (call status, statuses, states).  A refused call (INVALID_ARGUMENT) or a device failure raises BpgError."""
        n = len(items)
        arr = (VerifyResidentItem * max(n, 1))()
        states, keep = [], []
        for k, it in enumerate(items):
            it = tuple(it) + (None, 0, None, None)[len(it) - 3:]
            state, coms, proof, seed, flags, params, inputs = it
            ts = _buf(203); ts.raw = _exact("transcript_state", state, 203)
            coms, proof, seed = _exact("commitments", coms, 32 * self.m), bytes(proof), _seed32(seed)
            # (lengths are held to the circuit's where it has such values; where it has none the library refuses the item)
            params = None if params is None else b"".join(params) if isinstance(params, (list, tuple)) else bytes(params)
            inputs = None if inputs is None else b"".join(inputs) if isinstance(inputs, (list, tuple)) else bytes(inputs)
            if params is not None and self.n_params:
                params = _exact("params", params, 32 * self.n_params)
            if inputs is not None and self.n_inputs:
                inputs = _exact("inputs", inputs, 32 * self.n_inputs)
            arr[k].transcript_state = C.cast(ts, C.c_void_p); arr[k].V = coms; arr[k].proof = proof; arr[k].proof_len = len(proof); arr[k].seed = seed
            arr[k].flags = flags; arr[k].param_values = params; arr[k].input_values = inputs
            states.append(ts); keep.append((coms, proof, seed, params, inputs))
        status = (C.c_int32 * max(n, 1))()
        rc = lib().bpg_r1cs_verify_resident_batch(self.ctx._h, self._h, C.c_uint64(n), arr, _seed32(batch_seed), status)
        if rc not in (0, 1, 2, 3):
            _chk(rc)
        out = ([status[k] for k in range(n)], [ts.raw[:203] for ts in states])
        return (rc,) + out if return_status else out

    def test_verify_wave_scalars(self, challenges, params=None, inputs=None):
        """bpg_test_verify_wave_scalars: the wave kernels of verify_batch() on challenge records of the caller's choosing.  challenges = one record per item:
        a list of 7 + 2 lg N scalars of 32 bytes (y^-1, z, x, u, a, b, rho, u_1 .. u_lgN, their inverses); params / inputs: None or one byte string per item
        -> (g, h as lists of N 32-byte scalars, slots = per item the list [w_V .. | w_c | delta], evidence dict)."""
        import json
        K = len(challenges)
        N = 1
        while N < self.n:
            N *= 2
        ch = b"".join(b"".join(rec) for rec in challenges)
        g, h, small, ev = _buf(32 * N), _buf(32 * N), _buf(32 * K * (self.m + 2)), _buf(4096)
        pv = None if params is None else b"".join(params)
        iv = None if inputs is None else b"".join(inputs)
        _chk(lib().bpg_test_verify_wave_scalars(self.ctx._h, self._h, C.c_uint64(K), ch, pv, iv, g, h, small, ev, C.c_uint64(4096)))
        cut = lambda b, cnt: [b.raw[32 * k:32 * k + 32] for k in range(cnt)]
        sl = cut(small, K * (self.m + 2))
        return cut(g, N), cut(h, N), [sl[k * (self.m + 2):(k + 1) * (self.m + 2)] for k in range(K)], json.loads(ev.value.decode())

    def free(self):
        if self._h:
            lib().bpg_r1cs_free(self.ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class WitnessProgram:
    """Owned copy of a bpg_witness_program: multiplier i has left = terms [lc_ptr[2i], lc_ptr[2i+1]) and right = [lc_ptr[2i+1], lc_ptr[2i+2]); a term is
    (term_var = kind << 29 | index, term_coef = index into the instance's coefficient table); param_rows: constraint rows whose constant term is assigned per witness."""

    def __init__(self, lc_ptr, term_var, term_coef, param_rows=()):
        import numpy as np
        self.lc_ptr = np.ascontiguousarray(lc_ptr, dtype=np.uint64)
        self.term_var = np.ascontiguousarray(term_var, dtype=np.uint32)
        self.term_coef = np.ascontiguousarray(term_coef, dtype=np.uint32)
        self.param_rows = [int(r) for r in param_rows]

    def cstruct(self):
        import numpy as np
        rows = np.ascontiguousarray(self.param_rows, dtype=np.uint64)
        c = WitnessProgramView()
        c.lc_ptr, c.term_var, c.term_coef = self.lc_ptr.ctypes.data, self.term_var.ctypes.data, self.term_coef.ctypes.data
        c.n_params, c.param_rows = len(rows), rows.ctypes.data if len(rows) else None
        c._owner = (self, rows)
        return c


class WitnessHints:
    """Owned copy of a bpg_witness_hints: multiplier mul[k] (strictly ascending) is a hint of kind[k] (HINT_BIT_PAIR: a_L = 1 - b, a_R = b, a_O = 0) with
    b = bit arg[k] of the canonical value of its source, the left list of that multiplier in the witness program (its right list is empty)."""

    def __init__(self, mul=(), kind=(), arg=()):
        import numpy as np
        self.mul = np.ascontiguousarray(mul, dtype=np.uint32)
        self.kind = np.ascontiguousarray(kind, dtype=np.uint32)
        self.arg = np.ascontiguousarray(arg, dtype=np.uint32)
        if not len(self.mul) == len(self.kind) == len(self.arg):
            raise ValueError("mul, kind and arg must have one entry per hint")

    def __len__(self):
        return len(self.mul)

    def cstruct(self):
        c = WitnessHintsView()
        c.n_hints = len(self.mul)
        c.hint_mul, c.hint_kind, c.hint_arg = (a.ctypes.data if len(a) else None for a in (self.mul, self.kind, self.arg))
        c._owner = self
        return c


def _scalars32(name, values, count):
    """count x 32 bytes from bytes or a sequence of 32-byte strings"""
    data = bytes(values) if isinstance(values, (bytes, bytearray)) else b"".join(_exact(name, x, 32) for x in values)
    return _exact(name, data, 32 * count)


class FlatInstance:
    """Owned copy of a bpg_r1cs_instance (numpy arrays + bytes); also what tests hand to the oracle."""

    def __init__(self, view: R1CSInstance, v=None, v_blinding=None, commitments=None):
        import numpy as np
        self.n, self.q, self.m, self.nnz, self.ncoef = view.n, view.q, view.m, view.nnz, view.ncoef
        def grab(ptr, nbytes): return C.string_at(ptr, nbytes) if ptr and nbytes else b""
        self.aL, self.aR, self.aO = grab(view.aL, 32 * self.n), grab(view.aR, 32 * self.n), grab(view.aO, 32 * self.n)
        self.row_ptr = np.frombuffer(grab(view.row_ptr, 8 * (self.q + 1)), dtype=np.uint64).copy()
        self.term_var = np.frombuffer(grab(view.term_var, 4 * self.nnz), dtype=np.uint32).copy()
        self.term_coef = np.frombuffer(grab(view.term_coef, 4 * self.nnz), dtype=np.uint32).copy()
        self.coef = grab(view.coef, 32 * self.ncoef)
        self.v, self.v_blinding, self.commitments = v, v_blinding, commitments

    def cstruct(self):
        c = R1CSInstance()
        c.n, c.q, c.m, c.nnz, c.ncoef = self.n, self.q, self.m, self.nnz, self.ncoef
        # one set of C buffers per instance, shared by every struct handed out (a struct must never outlive or invalidate another:
        # a batch holds many structs of the same instance at once)
        src = (self.aL, self.aR, self.aO, self.coef)
        if getattr(self, "_cbufs_src", None) is None or any(a is not b for a, b in zip(self._cbufs_src, src)):
            # a witness-free instance (a verifier's) still hands out non-NULL a_L, a_R, a_O, which bpg_r1cs_upload reads as n scalars each: the
            # buffers hold n zero scalars then, never fewer bytes than the struct claims (a 1-byte buffer let upload() read past the heap block)
            need = (32 * self.n, 32 * self.n, 32 * self.n, 0)
            self._cbufs = [C.create_string_buffer(x, max(len(x), k, 1)) for x, k in zip(src, need)]
            self._cbufs_src = src
        c.aL, c.aR, c.aO, c.coef = [C.cast(k, C.c_void_p).value for k in self._cbufs]
        c.row_ptr, c.term_var, c.term_coef = self.row_ptr.ctypes.data, self.term_var.ctypes.data, self.term_coef.ctypes.data
        c._owner = (self, self._cbufs)                       # keeps the buffers alive as long as the struct is
        return c


# ------------------------------------------------------------------------------------------------ transcript / prover / verifier
class Transcript:
    """merlin::Transcript::new(label)."""

    def __init__(self, label: bytes):
        self._h = C.c_void_p()
        self.label = bytes(label)           # a verifier rebuilds its transcript from the same label
        _chk(lib().bpg_transcript_new(self.label, C.c_uint64(len(label)), C.byref(self._h)))

    def append_message(self, label: bytes, msg: bytes):
        _chk(lib().bpg_transcript_append_message(self._h, label, bytes(msg), C.c_uint64(len(msg))))

    def challenge_bytes(self, label: bytes, n: int):
        out = _buf(n)
        _chk(lib().bpg_transcript_challenge_bytes(self._h, label, out, C.c_uint64(n)))
        return out.raw[:n]

    @property
    def state(self):
        out = _buf(203)
        _chk(lib().bpg_transcript_state(self._h, out))
        return out.raw[:203]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().bpg_transcript_free(self._h)
                self._h = None
        except Exception:       # interpreter shutdown: the module globals may be gone
            pass


class Prover:
    """bulletproofs::r1cs::Prover::new(&pc_gens, &mut transcript)."""

    def __init__(self, ctx: Context, transcript: Transcript):
        self.ctx, self.transcript = ctx, transcript
        self._h = C.c_void_p()
        # ctx=None gives an assembly-only prover (no commitments, no prove) - used by the CPU tests of the host logic
        _chk(lib().bpg_prover_new(ctx._h if ctx is not None else None, transcript._h, C.byref(self._h)))

    def commit(self, v: bytes, v_blinding: bytes):
        """Prover::commit(v, v_blinding) -> (CompressedRistretto, Variable)."""
        com, var = _buf(32), C.c_uint32()
        _chk(lib().bpg_prover_commit(self._h, v, v_blinding, com, C.byref(var)))
        return com.raw, Variable(var.value)

    def commit_many(self, vs, blindings):
        k = len(vs)
        coms, vars_ = _buf(32 * k), (C.c_uint32 * max(k, 1))()
        _chk(lib().bpg_prover_commit_many(self._h, C.c_uint64(k), b"".join(vs), b"".join(blindings), coms, vars_))
        return [coms.raw[32 * i:32 * i + 32] for i in range(k)], [Variable(vars_[i]) for i in range(k)]

    def commit_precomputed(self, v: bytes, v_blinding: bytes, commitment: bytes):
        """bpg_prover_commit_precomputed: Prover::commit with the Pedersen commitment supplied by the caller (works without a device context)."""
        var = C.c_uint32()
        _chk(lib().bpg_prover_commit_precomputed(self._h, _exact("v", v, 32), _exact("v_blinding", v_blinding, 32), _exact("commitment", commitment, 32), C.byref(var)))
        return Variable(var.value)

    def test_stub_commitments(self):
        """bpg_test_prover_stub_commitments (TEST HOOK): commitments of this prover become 32 hash bytes of (value, blinding) made on the host - not group
        elements - so that a device-less prover can run a driver's parsing and assembly under sanitizers; prove() stays refused."""
        _chk(lib().bpg_test_prover_stub_commitments(self._h))

    def defer_commitments(self, on: bool = True):
        """Extension (bpg_prover_defer_commitments): while on, commit / commit_many / Gadget.setup register their variables and return zero bytes;
        flush_commitments() computes every pending commitment in one kernel launch and appends them to the transcript in commit order."""
        _chk(lib().bpg_prover_defer_commitments(self._h, C.c_int32(1 if on else 0)))

    def flush_commitments(self):
        _chk(lib().bpg_prover_flush_commitments(self._h))

    def commitment(self, index: int) -> bytes:
        """The commitment of committed variable `index` (commit order), once flushed."""
        out = _buf(32)
        _chk(lib().bpg_prover_commitment(self._h, C.c_uint64(index), out))
        return out.raw

    def multiply(self, left, right):
        out = (C.c_uint32 * 3)()
        l, r = LinearCombination.of(left)._c(), LinearCombination.of(right)._c()
        _chk(lib().bpg_prover_multiply(self._h, C.byref(l), C.byref(r), out))
        return Variable(out[0]), Variable(out[1]), Variable(out[2])

    def allocate_multiplier(self, assignment):
        out = (C.c_uint32 * 3)()
        if assignment is None:
            _chk(lib().bpg_prover_allocate_multiplier(self._h, C.c_int32(0), None, None, out))
        else:
            _chk(lib().bpg_prover_allocate_multiplier(self._h, C.c_int32(1), assignment[0], assignment[1], out))
        return Variable(out[0]), Variable(out[1]), Variable(out[2])

    def allocate(self, assignment):
        out = C.c_uint32()
        _chk(lib().bpg_prover_allocate(self._h, C.c_int32(0 if assignment is None else 1), assignment, C.byref(out)))
        return Variable(out.value)

    def constrain(self, lc):
        c = LinearCombination.of(lc)._c()
        _chk(lib().bpg_prover_constrain(self._h, C.byref(c)))

    def num_constraints(self): return lib().bpg_prover_num_constraints(self._h)
    def get_num_multiplications(self): return lib().bpg_prover_num_multiplications(self._h)
    def num_committed(self): return lib().bpg_prover_num_committed(self._h)

    def instance(self) -> FlatInstance:
        view, v, vb = R1CSInstance(), C.c_void_p(), C.c_void_p()
        _chk(lib().bpg_prover_instance(self._h, C.byref(view), C.byref(v), C.byref(vb)))
        m = view.m
        return FlatInstance(view, v=C.string_at(v, 32 * m) if m else b"", v_blinding=C.string_at(vb, 32 * m) if m else b"")

    def input(self, value: bytes) -> "Variable":
        """bpg_prover_input: a public input of this proof with this value - a Variable (kind VAR_INPUT) to name wherever a constant stood (the bound of
        LessThan, an instance set, instance siblings).  To prove() it is that constant; template() keeps it a variable whose value every assign brings."""
        var = C.c_uint32()
        _chk(lib().bpg_prover_input(self._h, _exact("value", value, 32), C.byref(var)))
        self._n_inputs = getattr(self, "_n_inputs", 0) + 1
        return Variable(var.value)

    def gate(self, x: "Variable", var: "Variable") -> "Variable":
        """bpg_prover_gate: the variable whose value is x * var (kind VAR_GATED) - x a public input of this prover, var a multiplier variable or a committed
        value.  Named in linear combinations like any variable; prove() and instance() see (var, coefficient * x), template() keeps the gate and every
        assign brings x: ONE template for circuits that differ in which terms are switched on (MerklePath256: a path for every leaf index)."""
        out = C.c_uint32()
        _chk(lib().bpg_prover_gate(self._h, C.c_uint32(int(x)), C.c_uint32(int(var)), C.byref(out)))
        return Variable(out.value)

    def gates(self):
        """bpg_prover_gates: the gate table -> [(gated Variable, input index)], in the order gate() made them."""
        gv = WitnessGatesView()
        _chk(lib().bpg_prover_gates(self._h, C.byref(gv)))
        return [(Variable(gv.gate_var[k]), int(gv.gate_input[k])) for k in range(gv.n_gates)]

    def template_instance(self):
        """bpg_prover_template_instance -> (FlatInstance whose rows keep their input terms, the values of the inputs in input order)."""
        view, v, vb, n_in, iv = R1CSInstance(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_void_p()
        _chk(lib().bpg_prover_template_instance(self._h, C.byref(view), C.byref(v), C.byref(vb), C.byref(n_in), C.byref(iv)))
        m = view.m
        inst = FlatInstance(view, v=C.string_at(v, 32 * m) if m else b"", v_blinding=C.string_at(vb, 32 * m) if m else b"")
        raw = C.string_at(iv, 32 * n_in.value) if n_in.value else b""
        return inst, [raw[32 * i:32 * i + 32] for i in range(n_in.value)]

    def witness_program(self, hints=False):
        """bpg_prover_witness_program: how every multiplier's assignment follows from committed values and earlier multipliers (owned copy).
        INVALID_ARGUMENT for a circuit with free multipliers (allocate / allocate_multiplier) or with none.
        hints=True (bpg_prover_witness_program_hinted) -> (program, WitnessHints): the multipliers of range proofs are exported as bit hints, not refused."""
        import numpy as np
        view, hv = WitnessProgramView(), WitnessHintsView()
        if hints:
            _chk(lib().bpg_prover_witness_program_hinted(self._h, C.byref(view), C.byref(hv)))
        else:
            _chk(lib().bpg_prover_witness_program(self._h, C.byref(view)))
        n = self.get_num_multiplications()
        lc_ptr = np.frombuffer(C.string_at(view.lc_ptr, 8 * (2 * n + 1)), dtype=np.uint64).copy()
        nt = int(lc_ptr[-1])
        grab = lambda ptr, dt, k: np.frombuffer(C.string_at(ptr, k * np.dtype(dt).itemsize) if k else b"", dtype=dt).copy()
        prog = WitnessProgram(lc_ptr, grab(view.term_var, np.uint32, nt), grab(view.term_coef, np.uint32, nt), grab(view.param_rows, np.uint64, view.n_params))
        if not hints:
            return prog
        return prog, WitnessHints(*(grab(ptr, np.uint32, hv.n_hints) for ptr in (hv.hint_mul, hv.hint_kind, hv.hint_arg)))

    def allocate_bit(self, source, bit: int, source_value: bytes):
        """bpg_prover_allocate_bit: the multiplier range_proof makes for bit `bit` of `source` (a_L = 1 - b, a_R = b), recorded as a hint."""
        out = (C.c_uint32 * 3)()
        lc = LinearCombination.of(source)._c()
        _chk(lib().bpg_prover_allocate_bit(self._h, C.byref(lc), C.c_uint32(bit), _exact("source_value", source_value, 32), out))
        return Variable(out[0]), Variable(out[1]), Variable(out[2])

    NOTE_LAST_BLOCK = 1 << 31

    def noted(self):
        """bpg_prover_noted: the checkpoint candidates the gadgets pointed out, in the order they were made -> [(Variable, block, is_last)].  MimcHash256 (and
        MerkleTree256 through it) notes the sponge state after every absorbed block; is_last marks a sponge's digest (a Merkle node)."""
        n = C.c_uint64()
        _chk(lib().bpg_prover_noted(self._h, None, None, C.c_uint64(0), C.byref(n)))
        k = n.value
        vs, ts = (C.c_uint32 * max(k, 1))(), (C.c_uint32 * max(k, 1))()
        _chk(lib().bpg_prover_noted(self._h, vs, ts, C.c_uint64(k), C.byref(n)))
        return [(Variable(vs[i]), ts[i] & (self.NOTE_LAST_BLOCK - 1), bool(ts[i] & self.NOTE_LAST_BLOCK)) for i in range(k)]

    def mark_param_row(self, row: int):
        """bpg_prover_mark_param_row: the constant term of constraint `row` changes with the witness (num_constraints() - 1 right after the constrain call)."""
        _chk(lib().bpg_prover_mark_param_row(self._h, C.c_uint64(row)))

    def template(self, ctx: "Context", param_rows=(), checkpoints=()) -> "ResidentCircuit":
        """This circuit as a template resident on `ctx` (with this prover's witness): ResidentCircuit.assign(values, params) then gives it the witness of
        further proofs of the same shape without another host assembly.  param_rows: rows whose constant term is assigned per witness, besides the marked ones.
        checkpoints: multiplier Variables (noted() lists candidates) whose values assign(..., checkpoints=) takes from the caller."""
        prog, hints = self.witness_program(hints=True)
        prog.param_rows = prog.param_rows + [int(r) for r in param_rows]
        if ctx is None:
            raise BpgError(4, "template: no device context")
        if getattr(self, "_n_inputs", 0):       # public inputs: the rows keep their input terms, and assign(..., inputs=) brings the values
            inst, values = self.template_instance()
            return ctx.upload_template(inst, prog, hints, checkpoints=list(checkpoints), inputs=values, gates=self.gates() or None)       # (a gadget may have made the gates: ask the prover)
        return ctx.upload_template(self.instance(), prog, hints, checkpoints=list(checkpoints))

    def start_blinding(self, rng_seed: bytes = None, max_multipliers: int = 1 << 20):
        """Extension (include/bpg.h bpg_prover_start_blinding): all commitments made - start the serial TranscriptRng chain of the coming
        prove(rng_seed) on a host thread while the constraints are still being assembled. The proof bytes do not change."""
        self._stream_seed = _seed32(rng_seed)      # prove() without an explicit seed continues with this one
        _chk(lib().bpg_prover_start_blinding(self._h, self._stream_seed, C.c_uint64(max_multipliers)))

    def prove(self, bp_gens, rng_seed: bytes = None, flags: int = 0):
        """Prover::prove(&bp_gens) -> R1CSProof::to_bytes(); rng_seed stands in for thread_rng(): 32 fresh random bytes unless given
        (a pinned seed is for tests and benchmarks only)."""
        if rng_seed is None and getattr(self, "_stream_seed", None) is not None:
            rng_seed = self._stream_seed
        rng_seed = _seed32(rng_seed)
        capacity = bp_gens.gens_capacity if isinstance(bp_gens, BulletproofGens) else int(bp_gens)
        cap = lib().bpg_proof_size(self.get_num_multiplications(), flags)
        out = _buf(cap); ln = C.c_uint64(cap)
        _chk(lib().bpg_prover_prove(self._h, C.c_uint64(capacity), rng_seed, C.c_uint32(flags), out, C.byref(ln), None))
        return out.raw[:ln.value]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().bpg_prover_free(self._h)
                self._h = None
        except Exception:       # interpreter shutdown: the module globals may be gone
            pass


class Verifier:
    """bulletproofs::r1cs::Verifier::new(&mut transcript): constraint assembly on the host, verify() / is_valid() on the GPU (bpg_verifier_verify)."""

    def __init__(self, transcript: Transcript):
        self.transcript = transcript
        self._h = C.c_void_p()
        _chk(lib().bpg_verifier_new(transcript._h, C.byref(self._h)))

    def commit(self, com: bytes):
        var = C.c_uint32()
        _chk(lib().bpg_verifier_commit(self._h, com, C.byref(var)))
        return Variable(var.value)

    def input(self, value: bytes) -> "Variable":
        """bpg_verifier_input: the verifier's side of Prover.input - the same values in the same order."""
        var = C.c_uint32()
        _chk(lib().bpg_verifier_input(self._h, _exact("value", value, 32), C.byref(var)))
        return Variable(var.value)

    def gate(self, x: "Variable", var: "Variable") -> "Variable":
        """bpg_verifier_gate: the verifier's side of Prover.gate - the same gates in the same order."""
        out = C.c_uint32()
        _chk(lib().bpg_verifier_gate(self._h, C.c_uint32(int(x)), C.c_uint32(int(var)), C.byref(out)))
        return Variable(out.value)

    def get_num_vars(self): return lib().bpg_verifier_num_vars(self._h)

    def verify(self, proof: bytes, ctx: "Context", bp_gens, seed: bytes = None, flags: int = 0):
        """Verifier::verify(&proof, &pc_gens, &bp_gens) on the GPU: returns None, raises BpgError(VERIFICATION_ERROR / FORMAT_ERROR ...)."""
        capacity = bp_gens.gens_capacity if isinstance(bp_gens, BulletproofGens) else int(bp_gens)
        seed, proof = _seed32(seed), bytes(proof)
        _chk(lib().bpg_verifier_verify(self._h, ctx._h, C.c_uint64(capacity), proof, C.c_uint64(len(proof)), seed, C.c_uint32(flags)))

    def is_valid(self, proof, ctx, bp_gens, seed=None, flags=0):
        try:
            self.verify(proof, ctx, bp_gens, seed, flags)
            return True
        except BpgError as e:
            if e.status in (2, 3):
                return False
            raise

    def instance(self) -> FlatInstance:
        view, coms = R1CSInstance(), C.c_void_p()
        _chk(lib().bpg_verifier_instance(self._h, C.byref(view), C.byref(coms)))
        return FlatInstance(view, commitments=C.string_at(coms, 32 * view.m) if view.m else b"")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().bpg_verifier_free(self._h)
                self._h = None
        except Exception:       # interpreter shutdown: the module globals may be gone
            pass


class ConstraintBuffer:
    """ProverBuffer / VerifierBuffer of the reference (src/cs_buffer.rs): records a clause's operations for an OR block."""

    def __init__(self, parent, prover_side: bool):
        first = parent.next_multiplier() if isinstance(parent, ConstraintBuffer) else \
            (parent.get_num_multiplications() if isinstance(parent, Prover) else parent.get_num_vars())
        self.prover_side = prover_side
        self._h = C.c_void_p()
        _chk(lib().bpg_buffer_new(C.c_uint64(first), C.c_int32(1 if prover_side else 0), C.byref(self._h)))

    def rewind(self):
        _chk(lib().bpg_buffer_rewind(self._h))

    def next_multiplier(self):
        lib().bpg_buffer_next_multiplier.restype = C.c_uint64
        return lib().bpg_buffer_next_multiplier(self._h)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().bpg_buffer_free(self._h)
                self._h = None
        except Exception:       # interpreter shutdown: the module globals may be gone
            pass


def or_conjunction(main, buffer: ConstraintBuffer):
    """or(main, buffer) (src/or/or_conjunction.rs:4-38): main is a Prover, a Verifier or an enclosing ConstraintBuffer."""
    if isinstance(main, ConstraintBuffer):
        _chk(lib().bpg_or_buffer(main._h, buffer._h))
    elif isinstance(main, Prover):
        _chk(lib().bpg_or_prover(main._h, buffer._h))
    else:
        _chk(lib().bpg_or_verifier(main._h, buffer._h))


class PedersenGens:
    """PedersenGens::default() - the bases live in the Context."""
    def __init__(self, ctx: Context): self.ctx = ctx
    def bases(self): return self.ctx.pedersen_bases()


class BulletproofGens:
    """BulletproofGens::new(gens_capacity, 1): derives the tables on the GPU and keeps them in HBM."""
    def __init__(self, ctx: Context, gens_capacity: int, party_capacity: int = 1):
        if party_capacity != 1:
            raise ValueError("only party_capacity = 1 is used by the reference (src/bin/prover.rs:92)")
        self.ctx, self.gens_capacity = ctx, gens_capacity
        ctx.gens_ensure(gens_capacity)


# ------------------------------------------------------------------------------------------------ commitments.rs
def commit_single(prover: Prover, witness: bytes, blinding: bytes):
    """commitments::commit_single (src/commitments.rs:22-30)."""
    assert len(witness) <= 32, "the provided witness is longer than 32 bytes"
    s = be_to_scalar(witness)
    com, var = prover.commit(s, blinding)
    return s, com, var


def commit(prover: Prover, witness: bytes, blindings):
    """commitments::commit (src/commitments.rs:34-43): splits into 32-byte scalars."""
    scalars = be_to_scalars(witness)
    coms, vars_ = prover.commit_many(scalars, list(blindings)[:len(scalars)])
    return scalars, coms, vars_


def commit_all_single(prover: Prover, witnesses, blindings):
    """commitments::commit_all_single (src/commitments.rs:8-19), batched into one kernel launch."""
    scalars = [be_to_scalar(w) for w in witnesses]
    coms, vars_ = prover.commit_many(scalars, list(blindings)[:len(scalars)])
    return scalars, coms, vars_


def verifier_commit(verifier: Verifier, commitments):
    return [verifier.commit(c) for c in commitments]


# ------------------------------------------------------------------------------------------------ gadgets
class Gadget:
    def __init__(self, handle): self._h = handle

    def setup(self, prover: Prover, witnesses, blindings):
        """Gadget::setup (src/gadget.rs:18-38) -> (commitments, [(scalar, Variable)])."""
        cap = max(8, len(blindings), 2 * len(witnesses) + 2)
        n = C.c_uint64(cap)
        coms, dsc, dvars = _buf(32 * cap), _buf(32 * cap), (C.c_uint32 * cap)()
        _chk(lib().bpg_gadget_setup(self._h, prover._h, b"".join(witnesses), C.c_uint64(len(witnesses)), b"".join(blindings),
                                    C.c_uint64(len(blindings)), coms, dsc, dvars, C.byref(n)))
        k = n.value
        return [coms.raw[32 * i:32 * i + 32] for i in range(k)], [(dsc.raw[32 * i:32 * i + 32], Variable(dvars[i])) for i in range(k)]

    def preprocess(self, witnesses):
        """Gadget::preprocess (src/gadget.rs:8): the derived scalars, for a host that makes the commitments itself."""
        cap = max(8, 2 * len(witnesses) + 2)
        n = C.c_uint64(cap)
        dsc = _buf(32 * cap)
        _chk(lib().bpg_gadget_preprocess(self._h, b"".join(witnesses), C.c_uint64(len(witnesses)), dsc, C.byref(n)))
        return [dsc.raw[32 * i:32 * i + 32] for i in range(n.value)]

    def prove(self, prover, commitment_vars, derived_witnesses):
        """Gadget::prove on a Prover or on a ConstraintBuffer (the dyn ConstraintSystem of the reference)."""
        v = (C.c_uint32 * max(len(commitment_vars), 1))(*[int(x) for x in commitment_vars])
        dv = (C.c_uint32 * max(len(derived_witnesses), 1))(*[int(x[1]) for x in derived_witnesses])
        fn = lib().bpg_gadget_prove_buffered if isinstance(prover, ConstraintBuffer) else lib().bpg_gadget_prove
        _chk(fn(self._h, prover._h, v, C.c_uint64(len(commitment_vars)), b"".join(x[0] for x in derived_witnesses),
                dv, C.c_uint64(len(derived_witnesses))))

    def verify(self, verifier, witnesses, derived):
        v = (C.c_uint32 * max(len(witnesses), 1))(*[int(x) for x in witnesses])
        dv = (C.c_uint32 * max(len(derived), 1))(*[int(x) for x in derived])
        fn = lib().bpg_gadget_verify_buffered if isinstance(verifier, ConstraintBuffer) else lib().bpg_gadget_verify
        _chk(fn(self._h, verifier._h, v, C.c_uint64(len(witnesses)), dv, C.c_uint64(len(derived))))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().bpg_gadget_free(self._h)
                self._h = None
        except Exception:       # interpreter shutdown: the module globals may be gone
            pass


class BoundsCheck(Gadget):
    """BoundsCheck::new(&min, &max) (src/bounds_check/bounds_check_gadget.rs:54-63); big-endian byte vectors."""
    def __init__(self, min_be: bytes, max_be: bytes):
        h = C.c_void_p()
        _chk(lib().bpg_bounds_check_new(bytes(min_be), C.c_uint64(len(min_be)), bytes(max_be), C.c_uint64(len(max_be)), C.byref(h)))
        super().__init__(h)


class MimcHash256(Gadget):
    """MimcHash256::new(image) (src/mimc_hash/mimc_hash_gadget.rs:65-70)."""
    def __init__(self, image):
        h = C.c_void_p()
        lc = LinearCombination.of(image)._c()
        _chk(lib().bpg_mimc_hash256_new(C.byref(lc), C.byref(h)))
        super().__init__(h)


class MerkleTree256(Gadget):
    """MerkleTree256::new(root, instance_vars, witness_vars, pattern) (src/merkle_tree/merkle_tree_gadget.rs:59-73).
    pattern: the tree in the .gadgets syntax with W / I leaves, e.g. "((W W) (I W))"."""
    def __init__(self, root, instance_vars, witness_vars, pattern: str):
        h = C.c_void_p()
        r = LinearCombination.of(root)._c()
        iv, wv = _lc_array(instance_vars), _lc_array(witness_vars)
        _chk(lib().bpg_merkle_tree256_new(C.byref(r), iv, C.c_uint64(len(instance_vars)), wv, C.c_uint64(len(witness_vars)),
                                          pattern.encode(), C.byref(h)))
        super().__init__(h)


class MerklePath256(Gadget):
    """A Merkle path whose leaf index is a public input: ONE circuit (and one template) for every leaf of a tree of depth len(levels).
    levels[j] = (nb_j, b_j, c1_j, c2_j): four Variables from Prover.input / Verifier.input per level, bottom level first; leaf: the leaf's Variable (a
    committed value or a multiplier variable); root: a linear combination (the last input).  With the input values of merkle_path_inputs it is
    MerkleTree256 for that index's pattern with instance siblings, proof for proof.  It makes gates: prove() / verify() on a Prover / Verifier, no buffer.
    A verifier must build the input values with merkle_path_inputs (or MerkleTree.path_inputs) from an index and siblings: arbitrary values state
    something else than membership."""
    def __init__(self, root, leaf, levels):
        h = C.c_void_p()
        r = LinearCombination.of(root)._c()
        flat = [int(v) for lv in levels for v in lv]
        if len(flat) != 4 * len(levels):
            raise ValueError("a level is (nb, b, c1, c2)")
        arr = (C.c_uint32 * max(len(flat), 1))(*flat)
        _chk(lib().bpg_merkle_path256_new(C.byref(r), C.c_uint32(int(leaf)), arr, C.c_uint64(len(levels)), C.byref(h)))
        super().__init__(h)


def merkle_path_inputs(index, siblings, root):
    """bpg_merkle_path_inputs: the 4 * depth + 1 public inputs of MerklePath256 for leaf `index` with `siblings` (bottom level first, as MerkleTree.paths
    gives them) under `root`: per level (1 - b, b, sibling if b else 0, 0 if b else sibling) with b = bit j of the index, then the root."""
    d = len(siblings)
    out = _buf(32 * (4 * d + 1))
    sib = b"".join(_exact("sibling", x, 32) for x in siblings)
    _chk(lib().bpg_merkle_path_inputs(C.c_uint64(index), sib if d else None, C.c_uint64(d), _exact("root", root, 32), out))
    raw = out.raw
    return [raw[32 * k:32 * k + 32] for k in range(4 * d + 1)]


class Equality(Gadget):
    """Equality::new(right_hand) (src/equality/equality_gadget.rs:35-40)."""
    def __init__(self, right_hand):
        h = C.c_void_p()
        arr = _lc_array(right_hand)
        _chk(lib().bpg_equality_new(arr, C.c_uint64(len(right_hand)), C.byref(h)))
        super().__init__(h)


class Inequality(Gadget):
    """Inequality::new(right_hand, right_hand_assignment) (src/inequality/inequality_gadget.rs:95-101)."""
    def __init__(self, right_hand, right_hand_assignment=None):
        h = C.c_void_p()
        arr = _lc_array(right_hand)
        ra = b"".join(right_hand_assignment) if right_hand_assignment is not None else None
        if ra == b"":
            ra = bytes(32)      # non-NULL marker for an empty assignment list
        _chk(lib().bpg_inequality_new(arr, C.c_uint64(len(right_hand)), ra, C.byref(h)))
        super().__init__(h)


class LessThan(Gadget):
    """LessThan::new(left, left_assignment, right, right_assignment) (src/less_than/less_than_gadget.rs:69-86)."""
    def __init__(self, left_hand, left_hand_assignment, right_hand, right_hand_assignment):
        h = C.c_void_p()
        l, r = LinearCombination.of(left_hand)._c(), LinearCombination.of(right_hand)._c()
        _chk(lib().bpg_less_than_new(C.byref(l), left_hand_assignment, C.byref(r), right_hand_assignment, C.byref(h)))
        super().__init__(h)


class SetMembership(Gadget):
    """SetMembership::new(value, value_assignment, instance_vars, instance_vars_assignments) (set_membership_gadget.rs:64-77)."""
    def __init__(self, value, value_assignment, instance_vars, instance_vars_assignments):
        h = C.c_void_p()
        v = LinearCombination.of(value)._c()
        arr = _lc_array(instance_vars)
        ia = b"".join(instance_vars_assignments) if instance_vars_assignments else None
        _chk(lib().bpg_set_membership_new(C.byref(v), value_assignment, arr, C.c_uint64(len(instance_vars)), ia, C.byref(h)))
        super().__init__(h)


def range_proof(cs, x, n_bits, x_assignment=None):
    """utils::range_proof (src/utils.rs:5-35) on a Prover (assignment given) or a Verifier (None)."""
    lc = LinearCombination.of(x)._c()
    if isinstance(cs, Prover):
        if x_assignment is None:
            raise BpgError(5, "missing assignment")
        _chk(lib().bpg_range_proof_prove(cs._h, C.byref(lc), C.c_uint32(n_bits), x_assignment))
    else:
        _chk(lib().bpg_range_proof_verify(cs._h, C.byref(lc), C.c_uint32(n_bits)))


def hash_pattern(left, right):
    """hash!(l, r) macro of the reference (merkle_tree_gadget.rs:7-12) on pattern strings."""
    return "(%s %s)" % (left, right)
