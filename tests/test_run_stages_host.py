"""The rules by which a whole run walks its counting features (bgreat_amd/csrc/run_stages.h), driven without a device: tools/run_stages_main.cpp
plays them over stages that only record, built on its own under AddressSanitizer + UBSan.  The end of a run -- in which order the stages end,
what a failure among them does to the others, which code is returned -- and the mask that the graph's switches imply."""
import os
import subprocess

import pytest

from util import ROOT

CAPACITY, INTERNAL, NOMEM = -4, -5, -7
BITS = dict(abundance=1, links=2, pileup=4, variants=8, strands=16, bubbles=32, triples=64, phase=128, blocks=256, haplotypes=512)   # run_counts.h
END_ORDER = ["abundance", "links", "triples", "bubbles", "phase", "blocks", "haplotypes", "pileup"]
ALL = sum(BITS[s] for s in END_ORDER)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("run_stages") / "run_stages")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "run_stages_main.cpp"), "-o", path])
    return path


def play(exe, *args):
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "ERROR: " not in p.stderr and "runtime error" not in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout.splitlines()


def ends(exe, what, ok, **fail):
    """-> ([(stage, ok) per call], the code returned)"""
    lines = play(exe, "end", what, int(ok), *[x for kv in fail.items() for x in kv])
    assert lines[-1].startswith("rc ") and all(ln.startswith("end ") for ln in lines[:-1])
    return [(ln.split()[1], ln.split()[2] == "1") for ln in lines[:-1]], int(lines[-1].split()[1])


def test_all_stages_succeed(exe):
    calls, rc = ends(exe, ALL, True)
    assert rc == 0 and calls == [(s, True) for s in END_ORDER]
    calls, rc = ends(exe, BITS["abundance"] | BITS["links"] | BITS["bubbles"], True)   # only the stages of `what`
    assert rc == 0 and calls == [("abundance", True), ("links", True), ("bubbles", True)]


@pytest.mark.parametrize("failing", ["bubbles", "phase", "blocks", "haplotypes"])
def test_a_failed_stage_of_the_chain_takes_every_total_back(exe, failing):
    calls, rc = ends(exe, ALL, True, **{failing: INTERNAL})
    assert rc == INTERNAL
    at = END_ORDER.index(failing)
    first = [c for c in calls if c[1]]
    assert first == [(s, True) for s in END_ORDER[:at + 1]]   # in order with true up to the failure, nothing behind it ever with true
    last = {}
    for stage, ok in calls:
        last[stage] = ok
    assert set(last) == set(END_ORDER) and not any(last.values())   # every stage ends with false as its last call
    assert calls.index((failing, True)) < min(i for i, c in enumerate(calls) if not c[1])   # nothing is taken back before the failure
    for stage in END_ORDER[at + 1:]:
        assert calls.count((stage, False)) == 1


def test_a_run_that_comes_in_failed(exe):
    calls, rc = ends(exe, ALL, False)
    assert rc == 0 and calls == [(s, False) for s in END_ORDER]
    calls, rc = ends(exe, ALL, False, blocks=INTERNAL, pileup=CAPACITY)   # (nothing is asked to make totals: nothing can fail)
    assert rc == 0 and calls == [(s, False) for s in END_ORDER]


def test_the_pileup_fails_alone(exe):
    calls, rc = ends(exe, ALL, True, pileup=CAPACITY)
    assert rc == CAPACITY and calls == [(s, True) for s in END_ORDER]   # its code, and the other totals stay


def test_the_pileup_fails_after_a_chain_failure(exe):
    calls, rc = ends(exe, ALL, True, phase=NOMEM, pileup=CAPACITY)
    assert rc == NOMEM and calls[-1] == ("pileup", False) and ("pileup", True) not in calls
    calls, rc = ends(exe, ALL, True, bubbles=INTERNAL, haplotypes=NOMEM)   # the first failure's code; the later stage is never asked
    assert rc == INTERNAL and ("haplotypes", True) not in calls


def test_the_mask_the_switches_imply(exe):
    """all combinations of the ten switches against the implications written out here: haplotypes => blocks => phase => bubbles + triples, bubbles =>
    links, variants => pileup, strands only next to their own switch, anything => abundance"""
    lines = play(exe, "wanted")
    assert len(lines) == 1024
    names = ["links", "bubbles", "triples", "phase", "blocks", "haplotypes", "pileup", "variants", "pileup_strands", "variants_strands"]
    for m, ln in enumerate(lines):
        s = {n: bool(m >> i & 1) for i, n in enumerate(names)}
        want = set()
        if s["haplotypes"]:
            want |= {"haplotypes", "blocks"}
        if s["blocks"] or "blocks" in want:
            want |= {"blocks", "phase"}
        if s["phase"] or "phase" in want:
            want |= {"phase", "bubbles", "triples"}
        if s["bubbles"] or "bubbles" in want:
            want |= {"bubbles", "links"}
        if s["links"]:
            want.add("links")
        if s["triples"]:
            want.add("triples")
        if s["variants"]:
            want |= {"variants", "pileup"}
        if s["pileup"]:
            want.add("pileup")
        if (s["pileup"] and s["pileup_strands"]) or (s["variants"] and s["variants_strands"]):
            want.add("strands")
        if want:
            want.add("abundance")
        assert ln.split() == [str(m), str(sum(BITS[w] for w in want))], (s, ln)
