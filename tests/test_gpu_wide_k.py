"""Greedy mode on graphs with 32 < k <= 64 (two-word overlap keys, bgr_align_greedy_wide_kernel) on the GPU, checked row for row against the
Python restatement of the reference's greedy path (wide_greedy_ref.py, pinned to the C++ oracle by test_wide_k_host.py); and the wide kernel
at k <= 32 under test.wide_keys against the reference's own goldens and the oracle."""
import os
import random
import subprocess

import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
import wide_greedy_ref as W
from test_wide_k_host import pack, reads_from, strings
from tools.synth import Synth
from util import check_against_golden, golden_cases, parse_counters, resolve_args, run_cli

pytestmark = pytest.mark.gpu


def graph_and_reads(k, seed, exc=False):
    s = Synth(30000, 110, 2, k, seed)
    unitigs = strings(*s.unitigs())
    if exc:  # exception bases: non-ACGT characters inside some unitigs (the graph gets its N planes)
        r = random.Random(seed)
        for i in range(0, len(unitigs), 9):
            u = list(unitigs[i])
            u[r.randrange(len(u))] = r.choice("NRY")
            unitigs[i] = "".join(u)
    reads = []
    for L in (150, 250):
        rb, ro = s.reads(0, 60, L, 3, seed + L)
        fw = strings(rb, ro)
        reads += fw + [W.reverse_complements(x) for x in fw]
    reads += reads_from(unitigs, 60, 150, seed, subs=3)                       # every seventh with an N
    reads += [x[:n] for x in reads_from(unitigs, 12, 3 * k, seed + 1, with_n=False) for n in (k - 2, k - 1, k)]
    return unitigs, reads


@pytest.mark.parametrize("k", [33, 40, 47, 63, 64])
def test_batch_api_matches_the_checker(k):
    unitigs, reads = graph_and_reads(k, 700 + k)
    g = B.Graph.build(k, *pack(unitigs))
    al = B.Aligner(g, 0)
    ref = W.GreedyRef(k, unitigs)
    rseqs, roffs = pack(reads)
    pk = B.pack_reads(rseqs, roffs)
    for lds in (2, 1):   # key table staged in LDS / probed in L2
        al.configure(lds_mphf=lds)
        for m in (0, 2, 5):
            for e in (0, 1, 2, 5):
                want, cnt = ref.align(reads, m, e)
                al.reset_counters()
                got = W.rows_of(*al.align(rseqs, roffs, m=m, effort=e))
                assert got == want, (k, lds, m, e, next(i for i in range(len(got)) if got[i] != want[i]))
                c = al.counters()
                assert {x: c[x] for x in cnt} == cnt, (k, m, e, c, cnt)
                if m == 2 and e == 2:
                    assert W.rows_of(*al.align_packed(pk, m=m, effort=e)) == want
                    assert al.launch_info()["mphf_in_lds"] == (lds == 2)
    names = [n for n, _ in al.kernel_times()[1]]
    assert "bgr_align_greedy_wide_kernel" in names, names


def test_graph_with_exception_bases():
    k = 40
    unitigs, reads = graph_and_reads(k, 77, exc=True)
    g = B.Graph.build(k, *pack(unitigs))
    assert g.info()["has_exceptions"]
    al = B.Aligner(g, 0)
    ref = W.GreedyRef(k, unitigs)
    for m, e in ((0, 1), (2, 2), (5, 5)):
        assert W.rows_of(*al.align(*pack(reads), m=m, effort=e)) == ref.align(reads, m, e)[0]


def test_exhaustive_mode_refused_on_wide_graph():
    s = Synth(20000, 90, 2, 40, 4)
    g = B.Graph.build(40, *s.unitigs())
    al = B.Aligner(g, 0)
    rb, ro = s.reads(0, 10, 150, 2, 5)
    with pytest.raises(B.BgrError, match="k <= 32"):
        al.align(rb, ro, m=2, effort=2, mode=B.MODE_EXHAUSTIVE)


# ---- the wide kernel at k <= 32 (test.wide_keys) against the reference -------------------------------------------------------------
def test_wide_keys_goldens_through_the_cli():
    n = 0
    for case in golden_cases():
        a = case["args"]
        if "-b" in a or "-G" in a:
            continue
        out, paths, na = run_cli(B.CLI_PATH, resolve_args(a) + ["--set", "test.wide_keys=1"])
        check_against_golden(case, out, paths, na)
        n += 1
    assert n > 30


@pytest.mark.parametrize("k", [8, 21, 31, 32])
def test_wide_keys_synth_matches_oracle(k):
    s = Synth(40000, 70, 2, k, 900 + k)
    seqs, offs = s.unitigs()
    with B.options(**{"test.wide_keys": 1}):
        g = B.Graph.build(k, seqs, offs)
    al = B.Aligner(g, 0)
    o = oracle_py.Oracle(k, seqs, offs)
    rb, ro = s.reads(0, 3000, 150, 3, 901 + k)
    for m, e in ((0, 1), (2, 2), (5, 5)):
        p1, po1, st1 = al.align(rb, ro, m=m, effort=e)
        p2, po2, st2 = o.align(rb, ro, m=m, effort=e)
        assert np.array_equal(st1, st2) and np.array_equal(po1, po2) and np.array_equal(p1, p2), (k, m, e)
    names = [n for n, _ in al.kernel_times()[1]]
    assert "bgr_align_greedy_wide_kernel" in names and "bgr_align_greedy_kernel" not in names, names


# ---- the CLI at k = 63 --------------------------------------------------------------------------------------------------------------
def parse_records(text):
    """paths / notAligned.fa as written -> [(header, payload)]"""
    lines = text.decode().split("\n")
    out = []
    for i in range(0, len(lines) - 1, 2):
        out.append((lines[i], lines[i + 1]))
    return out


@pytest.mark.parametrize("fastq", [False, True])
@pytest.mark.parametrize("correct", [False, True])
def test_cli_k63(fastq, correct, tmp_path):
    k = 63
    unitigs, reads = graph_and_reads(k, 6300)
    # (reads of at most k bases are left to the batch tests: a FASTA reader drops them, aligner.cpp:86, and a path [0] -- a read that is one
    # key -- has no unitig for recoverPath, aligner.cpp:276)
    reads = [r for r in reads if len(r) > k]
    with open(tmp_path / "u.fa", "w") as f:
        for i, u in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, u))
    rf = tmp_path / ("r.fq" if fastq else "r.fa")
    with open(rf, "w") as f:
        for i, r in enumerate(reads):
            f.write(("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r))) if fastq else (">r%d\n%s\n" % (i, r)))
    args = ["-r", str(rf), "-k", str(k), "-g", str(tmp_path / "u.fa"), "-m", "2", "-e", "2", "-t", "4"] + (["-q"] if fastq else []) + (["-c"] if correct else [])
    oa, pa, na = run_cli(B.CLI_PATH, args)
    ob, pb, nb = run_cli(B.CLI_PATH, args + ["--host-route"])
    assert pa == pb and na == nb
    ref = W.GreedyRef(k, unitigs)
    rows, cnt = ref.align(reads, 2, 2)
    want_p, want_n = [], []
    for i, (st, path) in enumerate(rows):
        hdr = ("@r%d" if fastq else ">r%d") % i
        if path:
            want_p.append((hdr, ref.corrected(reads[i], st, path) if correct else "".join("%d." % x for x in path)))
        else:
            want_n.append((hdr, reads[i]))
    assert parse_records(pa) == want_p  # (without -c the second line is printPath's: ints and dots)
    got_n = parse_records(na)
    if fastq:  # (here the FASTQ reader hands on one more record, without a header line, on both routes alike: compared by route above only)
        got_n = [r for r in got_n if r[0]]
    assert got_n == want_n
    c = parse_counters(oa)
    assert fastq or (c["reads"], c["no_overlap"], c["aligned"], c["not_aligned"]) == (cnt["reads"], cnt["no_overlap"], cnt["aligned"], cnt["not_aligned"])
    if not fastq and not correct:  # two lanes on this device, one output pair each: together the single run's files
        d = tmp_path / "split"
        d.mkdir()
        pr = subprocess.run([B.CLI_PATH] + args + ["--gpus", "2", "--split-output", "--set", "test.lanes_on_one_device=1"], cwd=d, capture_output=True,
                            text=True, timeout=600)
        assert pr.returncode == 0, pr.stderr[-2000:]
        assert b"".join(open(d / ("paths.%d" % i), "rb").read() for i in range(2)) == pa
        assert b"".join(open(d / ("notAligned.fa.%d" % i), "rb").read() for i in range(2)) == na


@pytest.mark.parametrize("extra,msg", [(["-b", "-k", "40"], "k <= 32"), (["-G", "-k", "40"], "k <= 32"), (["-k", "65"], "[2,64]")])
def test_cli_refusals(extra, msg, tmp_path):
    s = Synth(20000, 90, 2, 40, 8)
    s.write_unitigs(str(tmp_path / "u.fa"))
    s.write_reads(str(tmp_path / "r.fa"), 0, 50, 150, 2, 9)
    pr = subprocess.run([B.CLI_PATH, "-r", str(tmp_path / "r.fa"), "-g", str(tmp_path / "u.fa")] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 2 and msg in pr.stderr + pr.stdout, (pr.returncode, pr.stderr[-500:])
