"""CPU: stream_elide, the rewrite of the streamed walks' tables that stops storing nodes beside a tip or a cherry (no GPU, no
engine), under AddressSanitizer + UndefinedBehaviorSanitizer.

Plain C++ in phyamd_tree_schedule.h over phyamd_types.h: it re-packs mask groups into appended rows and rewrites bit fields of
the op in front of each changed op, run here with instrumentation over trees the program generates itself
(tests/cpp/elide_sanitize.cpp) and checked field by field against tables built with the switch off."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physher_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_elide_code_under_asan_ubsan(tmp_path):
    exe = tmp_path / "elide_sanitize"
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "elide_sanitize.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "elide_sanitize: ok" in out.stdout
