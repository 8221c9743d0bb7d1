"""CPU: stream_keep, the rewrite of the streamed pre-order walk's descriptors that keeps an elided node's stored child in registers
from its parent's op to its own (no GPU, no engine), under AddressSanitizer + UndefinedBehaviorSanitizer.

Plain C++ in phyamd_tree_schedule.h over phyamd_types.h, run here with instrumentation over trees the program generates itself
(tests/cpp/keep_sanitize.cpp).  The program replays the kernel's loop over the descriptors with the switch on and off and holds
that every op finds the same plane in the register set it reads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physher_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_keep_code_under_asan_ubsan(tmp_path):
    exe = tmp_path / "keep_sanitize"
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "keep_sanitize.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "keep_sanitize: ok" in out.stdout
