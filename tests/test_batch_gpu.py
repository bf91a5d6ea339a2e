"""N > 1 path on the GPU (run with -m gpu): two fresh processes each own an engine context on cuda:0, prove their share of a batch of
independent circuits with the PRODUCT (ResidentCircuit.prove, chains prefetched on the context's chain worker), all_gather the proof
bytes (gloo: one GPU box has one card; the 8-GPU runs use the same code over RCCL) and every rank checks the whole batch with the GPU
verifier and with the CPU oracle - bytes equal to the oracle prover's.  Also: bench.py --gpus 2 spawns its own ranks."""
import json
import os
import pathlib
import socket
import subprocess
import sys
import textwrap
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


WORKER = textwrap.dedent('''
    import os, sys, traceback
    def _report(t, v, tb):
        sys.stdout.write("WORKER FAILED: " + "".join(traceback.format_exception(t, v, tb))); sys.stdout.flush()
        os._exit(1)
    sys.excepthook = _report
    sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
    import torch, torch.distributed as dist
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    from bulletproofs_gadgets_amd.batch import shard_indices, gather_proofs
    import oracle_lib as O
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    ctx = bpg.Context(0)                      # both ranks share the one card of the box
    NUM = 5                                   # odd on purpose: ragged shards
    def assembled(i):
        # proof 0..3: 64-bit bounds checks with different witnesses, proof 4: a MiMC preimage (N = 1024, grouped-fold-free tail)
        return workloads.mimc_preimage(ctx, nbytes=40, seed=i) if i == 4 else workloads.bounds_check_64(ctx, seed=i)
    seed = lambda i: bytes([i + 1]) * 32
    mine = shard_indices(NUM, rank, world)
    items = []
    for i in mine:
        a = assembled(i)
        inst = a.prover.instance()
        ctx.gens_ensure(a.gens_capacity)
        items.append((i, a, inst, ctx.upload(inst)))
    local = {}
    # chains prefetched one proof ahead on the context's chain worker (bpg_blinding_begin), exactly as bench.py sequences them
    if items:
        i, a, inst, res = items[0]
        ctx.blinding_begin(a.transcript.state, inst.v_blinding, seed(i), inst.n)
    for k, (i, a, inst, res) in enumerate(items):
        if k + 1 < len(items):
            j, a2, inst2, _ = items[k + 1]
            ctx.blinding_begin(a2.transcript.state, inst2.v_blinding, seed(j), inst2.n)
        proof, _ = res.prove(a.transcript.state, inst.v_blinding, seed(i), 0)
        oc = O.FlatCircuit(inst.n, inst.m, inst.aL, inst.aR, inst.aO, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)
        rc, want, _ = O.prove(O.Gens(a.gens_capacity), a.transcript.state, oc, inst.v_blinding, seed(i), O.FLAG_FAST_MSM)
        assert rc == 0 and proof == want, "rank %%d proof %%d differs from the oracle" %% (rank, i)
        local[i] = proof
    sizes = {i: int(bpg.lib().bpg_proof_size(assembled(i).prover.get_num_multiplications(), 0)) for i in range(NUM)}
    plen = max(sizes.values())
    padded = {i: p + bytes(plen - len(p)) for i, p in local.items()}
    proofs = gather_proofs(padded, NUM, plen, dist)
    assert len(proofs) == NUM and all(p is not None for p in proofs)
    # every rank rebuilds every statement on the verifier side and checks every proof on the GPU
    for i in range(NUM):
        a = assembled(i)
        t = bpg.Transcript(a.transcript.label)
        v = bpg.Verifier(t)
        a.replay(v)
        assert v.is_valid(proofs[i][:sizes[i]], ctx, a.gens_capacity), (rank, i)
    a = assembled(0)
    t = bpg.Transcript(a.transcript.label); v = bpg.Verifier(t); a.replay(v)
    assert not v.is_valid(proofs[1][:sizes[1]], ctx, a.gens_capacity)          # a proof in the wrong slot must not verify
    dist.barrier()
    dist.destroy_process_group()
    sys.stdout.write("rank " + str(rank) + " ok\\n"); sys.stdout.flush()
''') % (str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "golden"))


def test_two_processes_one_gpu_gather_real_proofs(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rank 0 ok" in r.stdout and "rank 1 ok" in r.stdout


@pytest.mark.parametrize("leaves,steps", [(8, 2), (512, 4)])
def test_bench_spawns_its_own_ranks(leaves, steps):
    """python bench.py --gpus 2 without torchrun: the launcher starts two fresh ranks (gloo rehearsal on the one card) and relays ONE line - at the
    small size and at the HEADLINE size (512 leaves: two ranks with their own serving tables and proving streams on one card; the line carries
    each rank's view of the card's memory)."""
    env = dict(os.environ, BPG_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--full", "--steps", str(steps), "--warmup", "1", "--leaves", str(leaves), "--batch", "4",
                        "--no-cpu-baseline", "--in-flight", "2", "--in-flight-steps", "4"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == steps and out["scaling"] == "weak"
    assert all(x["hbm_in_use_GB"] and x["hbm_in_use_GB"] > 0 for x in out["ranks_seen"])
    if leaves == 512:
        assert out["config"]["N"] == 1 << 20 and out["config"]["q"] == 1986769
        print("two ranks at 2^20 on one card: %s" % [(x["rank"], x["proving_streams"], round(x["hbm_in_use_GB"], 1)) for x in out["ranks_seen"]])
    assert sorted(x["rank"] for x in out["ranks_seen"]) == [0, 1]
    assert out["batch"]["proofs"] == 4 and out["batch"]["ranks"] == 2 and out["batch"]["proofs_per_rank"] == 2
    assert out["value"] > 0 and out["roofline"]["whole_proof"]["alg_bytes"] > 0 and out["schedule"]["tt_lg"] == 12
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):       # the roofline object of the driver contract
        assert key in out["roofline"], key
    assert out["unit"] == "constraints/s" and out["higher_is_better"] is True and out["vs_baseline"] is None and out["dtype"] == "u32"
    assert "workload" in out["config"] and out["completions"]["last_ms"] > 0 and "cpu_baseline" not in out
    assert out["throughput"]["ranks_failed"] == 0 and out["throughput"]["proofs_in_flight_per_gpu"] == 2 and out["throughput"]["value"] > 0
    lone = out["lone_proof"]                                                   # rank 0's proof alone: the library's phase clock, its kernels' time, its launches
    assert lone["profile"] == "serving" and lone["launches"] > 20 and 0 < lone["kernel_ms_sum"] < lone["wall_ms"] and lone["phase_ms"]["ipa"] > 0
    if leaves == 512:
        assert lone["launches"] <= 200, lone["launches"]                       # the round-4 review's bar for a 2^20 proof alone (198 since round 5)


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """bench.py without --full: set-up, warm-up, exactly --steps timed proofs and the line, no secondary leg.  --dump-outputs writes what the last
    timed step returned (proof bytes, transcript state after the proof): the same on two runs, and the CPU oracle's bytes for that step's seed."""
    import numpy as np
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    import oracle_lib as O
    steps, dumps = 3, []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--leaves", "8", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == steps and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
        assert out["unit"] == "constraints/s" and out["higher_is_better"] is True and out["dtype"] == "u32" and out["metric"]
        assert out["roofline"] is None and out["lone_proof"] is None and out["single_stream"] is None and out["verify"] is None
        for key in ("cpu_baseline", "throughput", "throughput_variants", "batch", "small_configs", "end_to_end", "value_one_shot", "gpu_busy"):
            assert key not in out, key
        got = {name: np.load(d / (name + ".npy")) for name in ("proof", "transcript_state")}
        for v in got.values():
            assert v.dtype == np.float64 and v.min() >= 0 and v.max() <= 255 and np.all(v == np.round(v))
        dumps.append({name: bytes(v.astype(np.uint8)) for name, v in got.items()})
    assert dumps[0] == dumps[1]
    a = workloads.merkle_full_tree(bpg.Context(0), leaves=8)
    inst = a.prover.instance()
    oc = O.FlatCircuit(inst.n, inst.m, inst.aL, inst.aR, inst.aO, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)
    seed = bytes([0, steps - 1, 0]) + bytes(29)                                # bench.py seed_for(steps - 1) on rank 0
    rc, want, state = O.prove(O.Gens(a.gens_capacity), a.transcript.state, oc, inst.v_blinding, seed, O.FLAG_FAST_MSM)
    assert rc == 0 and dumps[0]["proof"] == want and dumps[0]["transcript_state"] == state


def test_plain_bench_at_the_headline_size_spends_little_outside_its_steps():
    """A plain run at 2^20 (20 proving streams, serving tables) in a new process: the whole run from start to exit, less (steps + warmup) x
    ms_per_step, is what set-up, warm-up beyond its steps and tear-down cost - well inside 30 s (about 5 s measured on one MI355X)."""
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == steps and out["config"]["N"] == 1 << 20 and out["value"] > 0
    outside = wall - (steps + warmup) * out["ms_per_step"] * 1e-3
    print("plain run at 2^20: %.1f s in all, %.1f s outside its steps, %.2f ms per step" % (wall, outside, out["ms_per_step"]))
    assert outside < 30.0, outside


RCCL_WORKER = textwrap.dedent('''
    import os, sys, threading, traceback
    def _report(t, v, tb):
        sys.stdout.write("WORKER FAILED: " + "".join(traceback.format_exception(t, v, tb))); sys.stdout.flush()
        os._exit(1)
    sys.excepthook = _report
    sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
    import torch, torch.distributed as dist
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    from bulletproofs_gadgets_amd.batch import gather_proofs
    import oracle_lib as O
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))          # "nccl" is RCCL on ROCm
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    ctx = bpg.Context(0)
    a = workloads.mimc_preimage(ctx, nbytes=40, seed=2)
    inst = a.prover.instance()
    ctx.gens_ensure(a.gens_capacity)
    res = ctx.upload(inst)
    seed = lambda i: bytes([i + 1]) * 32
    NUM = 4
    local, gathered = {}, []
    def prove_all():
        for i in range(NUM):
            local[i] = res.prove(a.transcript.state, inst.v_blinding, seed(i), 0)[0]
    # the engine proves on its own HIP stream while RCCL collectives run on torch's: first side by side, then the real gather
    th = threading.Thread(target=prove_all); th.start()
    for _ in range(8):
        gathered.append(gather_proofs({0: bytes(range(64))}, 1, 64, dist, device="cuda", force_collective=True))
    th.join()
    assert all(g == [bytes(range(64))] for g in gathered)
    plen = len(local[0])
    proofs = gather_proofs(local, NUM, plen, dist, device="cuda", force_collective=True)
    oc = O.FlatCircuit(inst.n, inst.m, inst.aL, inst.aR, inst.aO, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)
    for i in range(NUM):
        rc, want, _ = O.prove(O.Gens(a.gens_capacity), a.transcript.state, oc, inst.v_blinding, seed(i), O.FLAG_FAST_MSM)
        assert rc == 0 and proofs[i] == want, i
    t = torch.ones(4, device="cuda"); dist.all_reduce(t); assert float(t.sum().item()) == 4.0
    dist.barrier(); dist.destroy_process_group()
    sys.stdout.write("rccl ok\\n"); sys.stdout.flush()
''') % (str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "golden"))


def test_rccl_collectives_beside_engine_streams(tmp_path):
    """The collective of the multi-GPU path as the 8-GPU runs issue it - backend "nccl" (RCCL), device tensors, torch's stream - in a world of
    one on the one card of the box, while the engine proves on its own HIP stream; the gathered bytes are the oracle's."""
    script = tmp_path / "rccl_worker.py"
    script.write_text(RCCL_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rccl ok" in r.stdout


@pytest.mark.gpu
def test_plan_only_reads_the_node_from_sysfs_without_touching_the_gpu():
    """`bench.py --gpus N --plan-only` (the 8-GPU readiness check of a node nobody can run the real bench on yet): on a box with a card the topology comes from
    sysfs - the card's PCI address and NUMA node as torch reports them for device 0 - and the plan names cores, chain-pool lanes, expected HBM and pinned host
    memory per rank; the process never loads torch or the library (no HIP call)."""
    import json
    import subprocess
    import sys
    bench = str(pathlib.Path(__file__).resolve().parent.parent / "bench.py")
    r = subprocess.run([sys.executable, "-X", "importtime", bench, "--gpus", "1", "--plan-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "torch" not in r.stderr and "bulletproofs_gadgets_amd" not in r.stderr          # -X importtime lists every module the process imported
    plan = json.loads(r.stdout.strip().splitlines()[-1])
    assert plan["plan_only"] and plan["topology"]["source"] == "sysfs" and len(plan["ranks"]) == 1
    # torch in a process of its own: this one has the library's HIP runtime loaded, and torch's bundled one then sees no device
    q = subprocess.run([sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); "
                        "print('%04x:%02x:%02x.0' % (getattr(p, 'pci_domain_id', 0), p.pci_bus_id, p.pci_device_id))"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0, q.stderr[-2000:]
    assert plan["ranks"][0]["pci"] == q.stdout.strip().splitlines()[-1]
    rank = plan["ranks"][0]
    assert rank["proving_streams"] == 20 and sum(rank["chain_pool_lanes"]) <= 20 and 30 < rank["hbm_expected_GB"] < 288 and plan["fits"]["hbm_per_card"]

