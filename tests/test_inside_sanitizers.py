"""Sanitizer run of the host builder and lookup of the inside index (bgreat_amd/csrc/inside_index.cpp) in a stand-alone program,
tests/sanitize_inside.cpp, under ASan+UBSan: graphs at k = 5, 12 (palindromes planted), 31 and 32 and a set that repeats k-mers, each built
with 1, 3 and 8 threads, must hold exactly the entries of the definition (inside_ref.py); k = 33 and a unitig with an N are refused with
nothing left allocated.  CPU only."""
import os
import subprocess

import numpy as np

import inside_ref as R
from jump_ref import kint
from test_inside_host import SEED, _rand, _unitigs
from util import ROOT

SRC = os.path.join(ROOT, "bgreat_amd", "csrc")


def _case(name, k, us, rng, refused=False):
    lines = []
    absent = []
    if not refused:
        idx = R.index(k, us)
        lines = ["%d %d %d %d" % (c, uid, j, int(fc)) for c, (uid, j, fc) in sorted(idx.items())]
        held = {R.canonical(kint(u[j:j + k]), k) for u in us for j in range(len(u) - k + 1)}
        absent = [x for x in (kint(_rand(rng, k)) for _ in range(300)) if R.canonical(x, k) not in held]
    head = "case %s %d %d %d %d" % (name, k, len(us), -1 if refused else len(lines), len(absent))
    return "\n".join([head] + us + lines + [str(x) for x in absent]) + "\n", len(lines)


def test_inside_index_host_code_is_sanitizer_clean_and_builds_the_definitions_table(tmp_path):
    rng = np.random.default_rng(SEED + 77)
    cases, total = [], 0
    for k in (5, 12, 31, 32):
        text, n = _case("k%d" % k, k, _unitigs(k, rng), rng)
        cases.append(text)
        total += n
    core = _rand(rng, 80)
    text, n = _case("repeats", 12, [_rand(rng, 9) + core, core + _rand(rng, 30), R.rc(core), core[10:50] + core[:40]], rng)
    cases.append(text)
    assert total > 1000 and n > 10
    cases.append(_case("wide", 33, [_rand(rng, 70), _rand(rng, 40)], rng, refused=True)[0])
    cases.append(_case("exceptions", 15, [_rand(rng, 30) + "N" + _rand(rng, 30)], rng, refused=True)[0])
    path = tmp_path / "cases.txt"
    path.write_text("".join(cases))
    exe = str(tmp_path / "sanitize_inside")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-Wall", "-Wno-unused-function", "-I" + SRC,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize_inside.cpp")] +
                          [os.path.join(SRC, f) for f in ("inside_index.cpp", "graph_build.cpp", "anchor_index.cpp")] + ["-o", exe, "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "ERROR: " not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.endswith("7 cases\ninside ok\n") and "FAIL" not in p.stdout
