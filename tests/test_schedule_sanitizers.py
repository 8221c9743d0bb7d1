"""CPU: the host-built tree schedules (no GPU, no engine) under AddressSanitizer + UndefinedBehaviorSanitizer.

The tree check, build_schedule with its chunked walk lists, the streamed walks' tables and the batched walks' op lists are plain
C++ in phyamd_tree_schedule.h over phyamd_types.h: slot recycling, free lists and packed bit fields, run here with instrumentation
over trees the program generates itself (tests/cpp/schedule_sanitize.cpp), under every option set an engine can ask for."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physher_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_schedule_code_under_asan_ubsan(tmp_path):
    exe = tmp_path / "schedule_sanitize"
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "schedule_sanitize.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "schedule_sanitize: ok" in out.stdout
