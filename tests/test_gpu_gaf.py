"""GAF output on the GPU: `--gaf` through the CLI on both routes, bgr_align_fasta_text(want_output = 3) and bgr_aligner_path_stats, byte for byte /
row for row against gaf_ref.py (the definition in plain Python, pinned to the reference's -c bytes by test_gaf_host.py) over rows of the oracle
(k <= 32), of wide_greedy_ref (k > 32) or of the batch API (itself pinned to both elsewhere)."""
import os
import random
import subprocess

import numpy as np
import pytest

import bgreat_amd as B
import gaf_ref as G
import wide_greedy_ref as W
from test_gaf_host import case_args, check_lines, gaf_cases, golden_rows
from test_gpu_wide_k import graph_and_reads
from test_wide_k_host import pack, strings
from tools.synth import Synth
from util import GOLD, parse_counters, resolve_args, run_cli, sha

pytestmark = pytest.mark.gpu

CASES = gaf_cases()


@pytest.mark.parametrize("case", CASES, ids=["%02d-%s" % (c["id"], c["group"]) for c in CASES])
def test_cli_gaf_on_the_goldens(case):
    """paths = gaf_ref's lines over the oracle's rows; notAligned.fa and the counters are the golden's (the flag changes neither).  Default route,
    host route, tiny batches and chunks (irregular pieces and the host formatter mixed into one file), and the _wide kernels (test.wide_keys)."""
    a, us, H, R, rows = golden_rows(case)
    want, bug = G.gaf_of(us, a["k"], H, R, rows)
    assert bug is None
    want = want.encode("latin-1")
    variants = [[], ["--host-route"], ["-t", "5", "--batch", "37", "--chunk-bytes", "600"]]
    if not a["anchors"]:
        variants.append(["--set", "test.wide_keys=1"])
    for extra in variants:
        out, paths, na = run_cli(B.CLI_PATH, resolve_args(case["args"]) + ["--gaf"] + extra)
        assert paths == want, (case["args"], extra)
        assert parse_counters(out) == case["counters"], (case["args"], extra)
        assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"], (case["args"], extra)


def test_cli_gaf_with_no_overlap_file(tmp_path):
    """--no-overlap (host route) moves the reads without any anchor out of notAligned.fa; the GAF stream is the same"""
    n = 0
    for case in CASES:
        if case["group"] not in ("edge", "long", "dog") or "-q" in case["args"]:
            continue
        a, us, H, R, rows = golden_rows(case)
        want, _ = G.gaf_of(us, a["k"], H, R, rows)
        nov = str(tmp_path / ("nov%d.fa" % case["id"]))
        out, paths, na = run_cli(B.CLI_PATH, resolve_args(case["args"]) + ["--gaf", "--no-overlap", nov, "-t", "3"])
        novb = open(nov, "rb").read()
        assert paths == want.encode("latin-1"), case["args"]
        recs = lambda b: list(zip(b.split(b"\n")[0::2], b.split(b"\n")[1::2]))
        if "notaligned" in case:   # (the larger goldens keep a digest only)
            assert sorted(recs(case["notaligned"].encode("latin-1"))) == sorted(recs(na) + recs(novb)), case["args"]
        assert len(na) + len(novb) == case["notaligned_len"], case["args"]
        assert len(recs(novb)) == case["counters"]["no_overlap"]
        n += 1
    assert n >= 10


def test_the_goldens_cover_what_they_should():
    assert len(CASES) >= 60 and sum(c["counters"]["aligned"] for c in CASES) >= 7000


@pytest.mark.parametrize("fastq", [False, True])
@pytest.mark.parametrize("k", [33, 47, 63, 64])
def test_cli_gaf_wide_k(k, fastq, tmp_path):
    unitigs, reads = graph_and_reads(k, 100 * k)
    reads = [r for r in reads if len(r) > k]   # (as test_gpu_wide_k.test_cli_k63: a FASTA reader drops the others)
    with open(tmp_path / "u.fa", "w") as f:
        for i, u in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, u))
    rf = tmp_path / ("r.fq" if fastq else "r.fa")
    heads = [("@r%d" if fastq else ">r%d") % i + (" pair/1" if i % 3 == 0 else "\tx" if i % 5 == 0 else "") for i in range(len(reads))]
    with open(rf, "w") as f:
        for h, r in zip(heads, reads):
            f.write(("%s\n%s\n+\n%s\n" % (h, r, "I" * len(r))) if fastq else ("%s\n%s\n" % (h, r)))
    args = ["-r", str(rf), "-k", str(k), "-g", str(tmp_path / "u.fa"), "-m", "2", "-e", "2", "-t", "4", "--gaf"] + (["-q"] if fastq else [])
    _, pa, na = run_cli(B.CLI_PATH, args)
    _, pb, nb = run_cli(B.CLI_PATH, args + ["--host-route"])
    ref = W.GreedyRef(k, unitigs)
    rows, cnt = ref.align(reads, 2, 2)
    want, bug = G.gaf_of([""] + unitigs, k, heads, reads, rows)
    assert bug is None and cnt["aligned"] > 50 and any(st & W.ST_RC for st, p in rows if p)
    assert pa == want.encode() and pb == pa and nb == na
    assert check_lines([""] + unitigs, k, 2, heads, reads, rows, pa.decode()) == cnt["aligned"]


def _piece(k, n, L, seed, n_frac=0.05, long_every=0):
    """-> (graph, unitigs with "" in front, text, headers, reads): n reads of L bases, some with an N, some headers with a description"""
    s = Synth(150000, 90, 2, k, seed)
    seqs, offs = s.unitigs()
    rb, ro = s.reads(0, n, L, 3, seed + 1)
    rng = np.random.default_rng(seed)
    rb = rb.copy()
    for i in np.nonzero(rng.random(n) < n_frac)[0]:
        rb[int(ro[i]) + int(rng.integers(0, L))] = ord("N")
    reads = strings(rb, ro)
    if long_every:   # reads of 20 kb: far more than one pass of the 16 lanes
        lb, lo = s.reads(0, max(1, n // long_every), 20000, 4, seed + 2)
        longs = strings(lb, lo)
        for j, r in enumerate(longs):
            if j % 2:
                r = W.reverse_complements(r)
            reads[j * long_every] = r
    heads = [">r%d" % i + (" some text > inside %d" % i if i % 7 == 0 else "") for i in range(n)]
    text = "".join("%s\n%s\n" % (h, r) for h, r in zip(heads, reads)).encode()
    return B.Graph.build(k, seqs, offs), [""] + strings(seqs, offs), text, heads, reads


def test_text_call_equals_the_host_route_on_a_large_piece(tmp_path):
    k, n = 31, 210000
    g, us, text, heads, reads = _piece(k, n, 150, 77)
    f = str(tmp_path / "r.fa")
    open(f, "wb").write(text)
    B.align_all(g, f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2, threads=8, route=1, gaf=True)
    want_p, want_n = open(tmp_path / "p", "rb").read(), open(tmp_path / "n", "rb").read()
    al = B.Aligner(g, 0)
    p, na, info = al.align_fasta_text(text, m=2, effort=2, want_output=3, paths_cap=len(text))
    assert not info["irregular"] and info["n_accepted"] == n
    assert p == want_p and na == want_n and p.count(b"\n") > n // 2
    # a paths buffer that is too small: BGR_E_CAPACITY, then the same bytes through bgr_aligner_fetch_text
    p2, na2, _ = al.align_fasta_text(text, m=2, effort=2, want_output=3, paths_cap=1000)
    assert p2 == want_p and na2 == want_n
    # the first lines against the definition itself
    pth, po, st = al.align(*pack(reads[:3000]), m=2, effort=2)
    want, bug = G.gaf_of(us, k, heads[:3000], reads[:3000], W.rows_of(pth, po, st))
    assert bug is None and p.startswith(want.encode())


@pytest.mark.parametrize("k", [21, 40])
def test_text_call_long_reads_and_n(k):
    g, us, text, heads, reads = _piece(k, 4000, 150, 500 + k, n_frac=0.2, long_every=400)
    al = B.Aligner(g, 0)
    for m in (0, 2, 5):
        p, na, info = al.align_fasta_text(text, m=m, effort=2, want_output=3)
        assert not info["irregular"]
        pth, po, st = al.align(*pack(reads), m=m, effort=2)
        rows = W.rows_of(pth, po, st)
        want, bug = G.gaf_of(us, k, heads, reads, rows)
        assert bug is None and p == want.encode(), (k, m)
        assert na == "".join("%s\n%s\n" % (heads[i], reads[i]) for i in range(len(reads)) if not rows[i][1]).encode()
    assert any(len(reads[i]) == 20000 and rows[i][1] for i in range(len(reads)))
    check_lines(us, k, 5, heads, reads, rows, p.decode())


@pytest.mark.parametrize("k", [8, 15, 31, 32, 33, 48, 64])
def test_path_stats_rows(k):
    rnd = random.Random(k)
    s = Synth(60000, max(40, 2 * k), 2, k, 900 + k)
    seqs, offs = s.unitigs()
    us = [""] + strings(seqs, offs)
    g = B.Graph.build(k, seqs, offs)
    al = B.Aligner(g, 0)
    reads = []
    for L, n in ((k + 1, 40), (2 * k + 3, 100), (150, 300), (251, 100), (1000, 20), (20000, 4)):
        rb, ro = s.reads(0, n, L, 3, 31 * k + L)
        reads += strings(rb, ro)
    reads = [W.reverse_complements(r) if i % 2 else r for i, r in enumerate(reads)]
    for i in range(0, len(reads), 6):   # N reads
        r = list(reads[i])
        r[rnd.randrange(len(r))] = "N"
        reads[i] = "".join(r)
    rnd.shuffle(reads)
    n_mapped = n_rc = 0
    for lo, hi in ((0, 1), (1, 18), (18, 277), (277, len(reads))):   # ragged batches
        batch = reads[lo:hi]
        rb, ro = pack(batch)
        d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
        for m, e in ((0, 0), (2, 2), (5, 5), (2, 1), (5, 3)):
            al.align_device(d_r.data_ptr(), d_o.data_ptr(), len(batch), int(ro[-1]), max(len(x) for x in batch), m=m, effort=e)
            got = al.path_stats(d_r.data_ptr(), d_o.data_ptr(), len(batch))
            rows = W.rows_of(*al.fetch(len(batch), int(ro[-1]) + 8 * len(batch) + 8))
            for i, (st, path) in enumerate(rows):
                want = G.path_stat_row(us, k, batch[i], st, path)
                assert tuple(int(x) for x in got[i]) == want, (k, lo, m, e, i, path, st)
                n_mapped += bool(path)
                n_rc += bool(path) and bool(st & W.ST_RC)
        d_r.free()
        d_o.free()
    assert n_mapped > 500 and n_rc > 0   # (BGR_ST_RC only marks reads whose first try failed and whose retry mapped: few, but the branch must be walked)


def test_path_stats_refusals():
    ge = B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig_exc.fa"), 5)
    al = B.Aligner(ge, 0)
    with pytest.raises(B.BgrError, match="ACGT"):
        al.path_stats(1, 1, 1)
    s = Synth(20000, 75, 2, 31, 5)
    g = B.Graph.build(31, *s.unitigs())
    al = B.Aligner(g, 0)
    rb, ro = s.reads(0, 50, 150, 2, 6)
    d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), 50, int(ro[-1]), 150, mode=B.MODE_EXHAUSTIVE)
    with pytest.raises(B.BgrError, match="exhaustive"):
        al.path_stats(d_r.data_ptr(), d_o.data_ptr(), 50)
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), 50, int(ro[-1]), 150)
    with pytest.raises(B.BgrError, match="n_reads"):
        al.path_stats(d_r.data_ptr(), d_o.data_ptr(), 49)
    assert int(al.path_stats(d_r.data_ptr(), d_o.data_ptr(), 50)["aligned"].sum()) > 0


@pytest.mark.parametrize("extra,graph,msg", [(["-b"], "deg_unitig.fa", "-b"), (["-c"], "deg_unitig.fa", "-c"), ([], "deg_unitig_exc.fa", "ACGT")])
def test_cli_refusals(extra, graph, msg, tmp_path):
    pr = subprocess.run([B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5", "-g", os.path.join(GOLD, graph), "--gaf"] + extra, cwd=tmp_path,
                        capture_output=True, text=True, timeout=300)
    assert pr.returncode == 2 and "--gaf" in pr.stderr and msg in pr.stderr, (pr.returncode, pr.stderr[-500:])


def test_text_call_refusals():
    text = open(os.path.join(GOLD, "deg_reads.fa"), "rb").read()
    al = B.Aligner(B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig.fa"), 5), 0)
    with pytest.raises(B.BgrError, match="error -1.*want_output"):
        al.align_fasta_text(text, want_output=4)
    with pytest.raises(B.BgrError, match="error -1.*greedy"):
        al.align_fasta_text(text, want_output=3, mode=B.MODE_EXHAUSTIVE)
    with pytest.raises(B.BgrError, match="error -1.*record_info_out"):
        al.align_fasta_text(text, want_output=3, record_info=True)
    ale = B.Aligner(B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig_exc.fa"), 5), 0)
    with pytest.raises(B.BgrError, match="error -1.*ACGT"):
        ale.align_fasta_text(text, want_output=3)
