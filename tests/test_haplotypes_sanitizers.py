"""Sanitizer run of the host code of the haplotypes' sequences (the oriented ids of an entry, the checks of the two lists, the walk strings, the lines
of the file: bgreat_amd/csrc/haplotypes_host.h) in a stand-alone program, tests/sanitize_haplotypes.cpp, under ASan+UBSan.  CPU only: nothing here
touches a device or the library."""
import os
import subprocess

from util import ROOT

SRC = os.path.join(ROOT, "bgreat_amd", "csrc")


def test_haplotypes_host_code_is_sanitizer_clean(tmp_path):
    exe = str(tmp_path / "sanitize_haplotypes")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-Wall", "-I" + SRC, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "sanitize_haplotypes.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "haplotypes ok" in p.stdout and "FAIL" not in p.stdout
    assert "ERROR: " not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
