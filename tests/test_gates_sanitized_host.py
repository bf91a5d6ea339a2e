"""tests/hostcheck/template_gates.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program (its own main, no preload) that runs
Prover::gate, the template checks, the schedule, the packer, the derived slots and the host-compiled interpreter on the hand-made gated circuit and on the
depth-2 Merkle path, every buffer a heap block of exactly the size the plan gives."""
import subprocess

import oracle_lib as O


def test_template_gates_program_under_sanitizers(tmp_path):
    src = O.ROOT / "tests" / "hostcheck" / "template_gates.cpp"
    exe = tmp_path / "template_gates"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", (r.stdout[-2000:], r.stderr[-4000:])
