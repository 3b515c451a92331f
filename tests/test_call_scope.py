"""CPU: the call scope of the C entry points (csrc/api/call.hpp) over a fake HIP runtime (tests/emu/emu_call_scope.cpp),
as a stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process: what is
allocated, copied and synchronised on the all-device path, for host buffers, for one pointer passed several times, for
strided lines, for scratch and must_sync; that an exception frees every buffer once and pools none; the checked sizes."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CASES = ["all device pointers", "host input and output", "one host pointer as two inputs and the output", "strided lines",
         "scratch() alone", "a failing copy", "size helpers", "nothing left allocated"]


def test_call_scope_under_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "emu_call_scope")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "emu", "emu_call_scope.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES) and all(line.startswith("ok " + case) for line, case in zip(lines, CASES)), lines
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
