"""Sanitizer run of the host formatter's GAF lines with the cs:Z: field (bgreat_amd/csrc/record_format.h: gaf_line, append_cs_ops,
format_range_ext) in a stand-alone program, tests/sanitize_gaf_cs.cpp, under ASan+UBSan; and its lines against the definition
(gaf_ref.py + gaf_cs_ref.py + haplotag_ref.py), byte for byte: plain, with the field, tagged, tagged with the field.  The rows are the crafted
ones of test_gpu_crafted_rows.py that spell a walk -- both strands, paths of 1 to 48 unitigs, overhangs, offsets at the walk's end (no aligned
character: the empty value), an N --, at a narrow and a wide k; plus a set that ends at a row that spells no walk.  CPU only."""
import os
import random
import re
import subprocess

import gaf_cs_ref as CS
import gaf_ref as G
import haplotag_ref as H
from test_gpu_crafted_rows import crafted
from util import ROOT

SRC = os.path.join(ROOT, "bgreat_amd", "csrc")


def header_of(i):
    name = "" if i % 29 == 7 else "r%d" % i
    rest = ("", " " + "x" * (i % 37), "\tt%d" % i)[i % 3]
    return ">" + name + (rest if name or rest else " -")


def case_of(name, k, us, rows, table):
    """-> (the case's text for the program, the four expected outputs)"""
    heads = [header_of(i) for i in range(len(rows))]
    text = ["case %s %d %d %d" % (name, k, len(us) - 1, len(rows))] + us[1:] + [" ".join(str(x) for x in table)]
    for h, r in zip(heads, rows):
        text += [h, r.read or "-", " ".join(str(x) for x in [r.status, len(r.path)] + r.path)]
    reads, pairs = [r.read for r in rows], [(r.status, r.path) for r in rows]
    tag = lambda line, path: H.tagged_line(line, H.tag_of(table, path))
    plain, bug = G.gaf_of(us, k, heads, reads, pairs)
    tagged = "".join(tag(ln + "\n", p) for ln, p in zip(plain.split("\n")[:-1], [p for _, p in pairs if p]))
    want = {"plain": plain, "cs": CS.gaf_cs_of(us, k, heads, reads, pairs)[0], "tagged": tagged, "tagged+cs": CS.gaf_cs_of(us, k, heads, reads, pairs, tag)[0]}
    return "\n".join(text) + "\n", want, bug is None


def test_gaf_cs_host_code_is_sanitizer_clean_and_writes_the_definitions_bytes(tmp_path):
    cases, wants = [], {}
    for k in (15, 34):
        c = crafted(k)
        us = c["us"]
        rng = random.Random(k)
        table = [0] + [(rng.randrange(1, 7) << 1 | rng.randrange(2)) if rng.random() < 0.5 else 0 for _ in range(len(us) - 1)]
        walks = [r for r in c["rows"] if not r.path or G.walk_of(us, k, r.path) is not G.NO_WALK]
        bad = next(r for r in c["rows"] if r.path and G.walk_of(us, k, r.path) is G.NO_WALK)
        for name, rows in (("walks%d" % k, walks), ("exit%d" % k, walks[:40] + [bad] + walks[40:60])):
            text, want, ok = case_of(name, k, us, rows, table)
            assert ok == name.startswith("walks")
            cases.append(text)
            wants[name] = (want, ok)
        cs = wants["walks%d" % k][0]["cs"]
        assert "\tcs:Z:\n" in cs and re.search(r"\*[acgt][acgt]", cs) and re.search(r"\*[acgt]n", cs)   # the empty value, differences, a character outside ACGT
        assert cs.count("\n") > 200 and wants["walks%d" % k][0]["tagged+cs"].count("PS:i:") > 50
    path = tmp_path / "cases.txt"
    path.write_text("".join(cases))
    exe = str(tmp_path / "sanitize_gaf_cs")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-Wall", "-Wno-unused-function", "-I" + SRC,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize_gaf_cs.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "ERROR: " not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.endswith("gaf cs ok\n") and "FAIL" not in p.stdout
    got = {}
    for block in p.stdout[:-len("gaf cs ok\n")].split("== ")[1:]:
        head, _, body = block.partition("\n")
        name, variant, ok = head.split(" ")
        got[name, variant] = (body, ok == "ok=1")
    assert len(got) == 4 * len(wants)
    for name, (want, ok) in wants.items():
        for variant, text in want.items():
            assert got[name, variant] == (text, ok), (name, variant)
