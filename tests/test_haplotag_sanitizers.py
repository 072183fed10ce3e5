"""Sanitizer run of the host code of haplotags (the tag table from structs and from the bytes of a --blocks file with every check -- malformed
files among them: truncated lines, overlong numbers, no trailing newline, an empty file --, the tag of a row, the fields of a GAF line:
bgreat_amd/csrc/haplotag_host.h) in a stand-alone program, tests/sanitize_haplotag.cpp, under ASan+UBSan.  CPU only: nothing here touches a device
or the library."""
import os
import subprocess

from util import ROOT

SRC = os.path.join(ROOT, "bgreat_amd", "csrc")


def test_haplotag_host_code_is_sanitizer_clean(tmp_path):
    exe = str(tmp_path / "sanitize_haplotag")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-Wall", "-I" + SRC, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "sanitize_haplotag.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "haplotag ok" in p.stdout and "FAIL" not in p.stdout
    assert "ERROR: " not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
