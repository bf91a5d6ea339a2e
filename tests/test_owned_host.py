"""Who frees what is written in the types (csrc/host/owned.hpp: one move-only owning buffer; csrc/hip_handles.hpp: its device and pinned policies, an event and
a stream): the buffer is checked here on the CPU, as a stand-alone program under the sanitizers - no device, no preload - and the engine's source is checked for
the release lists it no longer has."""
import re
import subprocess

import oracle_lib as O

CSRC = O.ROOT / "bulletproofs_gadgets_amd" / "csrc"


def test_owning_buffer_under_the_sanitizers(tmp_path):
    """tests/hostcheck/owned.cpp: ensure within capacity makes no call, growth frees before it allocates, a failed allocation leaves the buffer empty and
    usable, moves (construction, assignment onto a full target, self-move), release twice, a reallocating vector, a map filled by move; nothing alive at exit"""
    exe = tmp_path / "owned"
    src = O.ROOT / "tests" / "hostcheck" / "owned.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr
    assert r.stdout.split()[-1] == "ok"


def test_the_owning_buffer_header_has_no_hip():
    text = (CSRC / "host" / "owned.hpp").read_text()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text


def test_the_engine_keeps_no_release_lists():
    """No array of buffer pointers to walk, and a context's destructor that names no buffer, event or stream: the members free themselves."""
    engine = (CSRC / "engine.hip").read_text()
    assert not re.search(r"DevBuf\s*\*\s*\w+\s*\[", engine) and not re.search(r"PinBuf\s*\*\s*\w+\s*\[", engine)
    start = engine.index("Engine::~Engine()")
    depth, end = 0, None
    for i in range(engine.index("{", start), len(engine)):
        depth += {"{": 1, "}": -1}.get(engine[i], 0)
        if depth == 0:
            end = i
            break
    body = engine[start:end + 1]
    assert "impl_" in body                                      # it is the destructor, and it does delete the context's state
    for word in ("release(", "hipEventDestroy", "hipStreamDestroy", "hipFree", "hipHostFree"):
        assert word not in body, word
    # ... and nowhere else in the engine either: the runtime's create and destroy calls live in the handles
    for word in ("hipEventDestroy", "hipStreamDestroy", "hipEventCreate", "hipStreamCreate", "hipFree(", "hipHostFree(", "hipMalloc(", "hipHostMalloc("):
        assert word not in engine, word


def test_live_resources_is_declared_and_the_abi_version_stays():
    header = (O.ROOT / "include" / "bpg.h").read_text()
    assert re.search(r"bpg_status\s+bpg_test_live_resources\s*\(\s*uint64_t\s+out\[6\]\s*\)\s*;", header)
    assert re.search(r"#define\s+BPG_ABI_VERSION\s+7u\b", header)
