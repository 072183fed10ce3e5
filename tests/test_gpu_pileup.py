"""Per-base depth and mismatches on the GPU: `--pileup` / `--depth` through the CLI on every route, bgr_aligner_pileup behind the batch, packed,
text and device-resident calls -- against pileup_ref.py (the definition in plain Python, pinned by test_pileup_host.py) over rows of the oracle
(goldens), of wide_greedy_ref (k > 32) or of the batch API itself (pinned to both elsewhere).

Not covered here, because no ACGT-only input is known to make the mapper write such a row -- test_gpu_crafted_rows.py writes them into the result
buffers itself and covers them on the GPU: a unitig glued on in the strand its sign does not name, a read that overhangs its walk's end, a path
that spells no walk (skipped > 0), ids outside the graph.  Still not covered on the GPU: a row that does not lie wholly inside the arena (the
kernel skips it), and such crafted rows with the read characters taken from the 2-bit planes or from a text (there they come as ASCII reads)."""
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import abundance_ref as A
import bgreat_amd as B
import gaf_ref as G
import links_ref as K
import pileup_ref as P
import wide_greedy_ref as W
from test_abundance_host import paths_bytes
from test_gaf_host import gaf_cases, golden_rows
from test_gpu_abundance import _mixed_reads
from test_gpu_wide_k import graph_and_reads
from test_wide_k_host import pack, strings
from tools.synth import Synth
from util import GOLD, parse_counters, resolve_args, sha

pytestmark = pytest.mark.gpu

CASES = gaf_cases()
FILES = {"pileup": "pile.tsv", "depth": "depth.bed", "abundance": "ab.tsv", "gfa": "g.gfa"}


def run(args, flags=("pileup", "depth"), timeout=600):
    """the CLI in a scratch directory, with a file for each of `flags` -> (stdout, paths bytes -- the pairs of a split run concatenated --,
    notAligned bytes, {flag: bytes or None}, the names in the directory)"""
    d = tempfile.mkdtemp()
    try:
        more = [x for f in flags for x in ("--" + f, os.path.join(d, FILES[f]))]
        p = subprocess.run([B.CLI_PATH] + list(args) + more, cwd=d, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:
            raise RuntimeError("%s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
        def cat(name):
            if os.path.exists(os.path.join(d, name + ".0")):
                return b"".join(open(os.path.join(d, "%s.%d" % (name, i)), "rb").read() for i in range(8) if os.path.exists(os.path.join(d, "%s.%d" % (name, i))))
            return open(os.path.join(d, name), "rb").read() if os.path.exists(os.path.join(d, name)) else None
        return p.stdout, cat("paths") or b"", cat("notAligned.fa") or b"", {f: cat(FILES[f]) for f in FILES}, sorted(os.listdir(d))
    finally:
        shutil.rmtree(d)


def flat_of(arr):
    """array of B.PILEUP_DTYPE -> (n, 6) int64, as Pileup.flat()"""
    return np.stack([arr[f] for f in B.PILEUP_DTYPE.names], axis=1).astype(np.int64)


@pytest.mark.parametrize("case", CASES, ids=["%02d-%s" % (c["id"], c["group"]) for c in CASES])
def test_cli_pileup_on_the_goldens(case):
    """both files = pileup_ref over the oracle's rows, whatever the route, the batching, the key layout, the number of lanes and the other outputs
    asked for; paths, notAligned.fa and the counters stay the golden's"""
    a, us, H, R, rows = golden_rows(case)
    p = P.pileup_of(us, a["k"], R, rows)
    assert p.skipped == 0
    want_sites, want_depth = P.sites_text_of(us, p), P.depth_text_of(us, p)
    lanes = ["--gpus", "2", "--set", "test.lanes_on_one_device=1"]
    variants = [[], ["--host-route"], ["-t", "5", "--batch", "37", "--chunk-bytes", "600"], lanes, lanes + ["--split-output"]]
    if not a["anchors"]:
        variants.append(["--set", "test.wide_keys=1"])
    for extra in variants:
        out, paths, na, f, names = run(resolve_args(case["args"]) + extra)
        assert f["pileup"] == want_sites and f["depth"] == want_depth, (case["args"], extra)
        assert parse_counters(out) == case["counters"], (case["args"], extra)
        assert len(paths) == case["paths_len"] and sha(paths) == case["paths_sha256"], (case["args"], extra)
        assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"], (case["args"], extra)
    # once each together with the other outputs: they are what they are without the pileup
    lens = A.unitig_lens(us)
    table = A.abundance_of(lens, a["k"], [len(r) for r in R], rows)
    gaf, bug = G.gaf_of(us, a["k"], H, R, rows)
    assert bug is None
    out, paths, na, f, _ = run(resolve_args(case["args"]) + ["--gaf"])
    assert f["pileup"] == want_sites and f["depth"] == want_depth and paths == gaf.encode("latin-1") and parse_counters(out) == case["counters"], case["args"]
    out, paths, na, f, _ = run(resolve_args(case["args"]) + ["-c"], flags=("depth",))   # (one flag alone switches the counting on)
    assert f["depth"] == want_depth and f["pileup"] is None and parse_counters(out) == case["counters"], case["args"]
    assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"], case["args"]
    out, paths, na, f, _ = run(resolve_args(case["args"]), flags=("pileup", "abundance"))
    assert f["pileup"] == want_sites and f["depth"] is None and f["abundance"] == A.text_of(lens, table), case["args"]
    assert sha(paths) == case["paths_sha256"] and sha(na) == case["notaligned_sha256"] and parse_counters(out) == case["counters"], case["args"]
    out, paths, na, f, _ = run(resolve_args(case["args"]), flags=("pileup", "depth", "gfa"))
    assert f["pileup"] == want_sites and f["depth"] == want_depth and f["gfa"] == K.gfa_text(us, a["k"], table, K.links_of(rows, len(us) - 1)), case["args"]
    assert sha(paths) == case["paths_sha256"] and sha(na) == case["notaligned_sha256"] and parse_counters(out) == case["counters"], case["args"]
    # the identity with the abundance file's bases column
    assert [int(d.sum()) for d in p.depth] == [t[1] for t in table]


def test_the_goldens_cover_what_they_should():
    """every class of rows the test above is meant to pin occurs in the oracle's rows (paths of more than 10 unitigs do not: test_batch_api_long_paths)"""
    n_mapped = n_nm = n_rc = n_n = n_twice = 0
    for case in CASES:
        a, us, H, R, rows = golden_rows(case)
        for r, (st, path) in zip(R, rows):
            if not path:
                continue
            ids = [abs(x) for x in path[1:]]
            n_mapped += 1
            n_nm += G.stats(us, a["k"], r, st, path)["nm"] > 0
            n_rc += bool(st & W.ST_RC)
            n_n += "N" in r
            n_twice += len(set(ids)) < len(ids)
    assert len(CASES) >= 60 and n_mapped > 7000 and n_nm > 0 and n_rc > 0 and n_n > 0 and n_twice > 0, (len(CASES), n_mapped, n_nm, n_rc, n_n, n_twice)


def test_cli_output_without_the_flags_is_unchanged():
    """stdout too: the flags add their files and nothing else"""
    case = next(c for c in CASES if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    out, paths, na, f, names = run(resolve_args(case["args"]))
    out0, paths0, na0, f0, names0 = run(resolve_args(case["args"]), flags=())
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
    assert strip(out0) == strip(out) and paths0 == paths and na0 == na
    assert names0 == ["notAligned.fa", "paths"] and names == ["depth.bed", "notAligned.fa", "paths", "pile.tsv"]
    assert f["pileup"].startswith(b"#unitig\tpos\tref\tdepth\tA\tC\tG\tT\tN\n") and b"\n363\t" in f["pileup"] and b"\n363\t" in f["depth"]   # (r0 of the file lies on 363 364 366 367)


@pytest.mark.parametrize("k", [8, 15, 31, 32, 33, 48, 64])
def test_batch_api_long_paths(k):
    """after every launch, through every entry point, the table has grown by pileup_ref over the rows that launch returned: paths of more than
    sixteen and of more than thirty-two unitigs (the carry across the kernel's passes), reads on both strands, with Ns, of k + 1 to 20 000 bases"""
    rnd = random.Random(k)
    s = Synth(60000, max(40, 2 * k), 2, k, 900 + k)
    seqs, offs = s.unitigs()
    us = [""] + strings(seqs, offs)
    g = B.Graph.build(k, seqs, offs)
    al = B.Aligner(g, 0)
    with pytest.raises(B.BgrError, match="error -1.*never enabled"):
        al.pileup()
    al.pileup_enable()
    got, skipped = al.pileup()
    assert not flat_of(got).any() and skipped == 0 and len(got) == sum(len(u) for u in us)
    reads = _mixed_reads(s, k, rnd)
    total = P.Pileup(us)
    n_mapped = n_rc = n_n = n_16 = n_32 = 0

    def check(rows, batch, where):
        nonlocal total
        total.add(P.pileup_of(us, k, batch, rows))
        got, skipped = al.pileup()
        want = total.flat()
        bad = np.nonzero((flat_of(got) != want).any(axis=1))[0]
        assert len(bad) == 0 and skipped == total.skipped == 0, (k, where, bad[:5], flat_of(got)[bad[:5]], want[bad[:5]])

    for lo, hi in ((0, 1), (1, 18), (18, 277), (277, len(reads))):   # ragged batches
        batch = reads[lo:hi]
        rb, ro = pack(batch)
        d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
        text = "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(batch)).encode()
        for m, e in ((0, 0), (2, 2), (5, 5)):
            rows = W.rows_of(*al.align(rb, ro, m=m, effort=e))
            check(rows, batch, (lo, m, e, "align"))
            al.align_device(d_r.data_ptr(), d_o.data_ptr(), len(batch), int(ro[-1]), max(len(x) for x in batch), m=m, effort=e)
            assert W.rows_of(*al.fetch(len(batch), int(ro[-1]) + 8 * len(batch) + 8)) == rows
            check(rows, batch, (lo, m, e, "align_device"))
            assert W.rows_of(*al.align_packed(B.pack_reads(rb, ro), m=m, effort=e)) == rows
            check(rows, batch, (lo, m, e, "align_packed"))
            pt, na, info = al.align_fasta_text(text, m=m, effort=e)
            assert not info["irregular"] and pt == paths_bytes([">r%d" % i for i in range(len(batch))], rows)
            check(rows, batch, (lo, m, e, "align_fasta_text"))
            n_mapped += sum(1 for _, p in rows if p)
            n_rc += sum(1 for st, p in rows if p and st & W.ST_RC)
            n_n += sum(1 for r, (_, p) in zip(batch, rows) if p and "N" in r)
            n_16 += sum(1 for _, p in rows if len(p) > 17)
            n_32 += sum(1 for _, p in rows if len(p) > 33)
        d_r.free()
        d_o.free()
    print("k", k, "mapped", n_mapped, "rc", n_rc, "with N", n_n, "paths > 16", n_16, "paths > 32", n_32)
    # (at k = 8 the 60 kb genome holds most 8-mers more than once: its unitigs are a few bases long, as in test_gpu_gaf.test_path_stats_rows)
    assert n_mapped > 500 and n_rc > 0 and n_n > 0 and n_16 > 0 and n_32 > 0
    assert "bgr_pileup_kernel" in [n for n, _ in al.kernel_times()[1]]
    # the identity with the abundance table the same launches filled
    ab = al.abundance()
    assert [int(d.sum()) for d in total.depth[1:]] == [int(x) for x in ab[:, 1]]
    # disabled launches add nothing; the table stays; reset zeroes
    rb, ro = pack(reads[18:277])
    al.pileup_enable(False)
    rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
    assert (flat_of(al.pileup()[0]) == total.flat()).all()
    al.pileup_enable(True)
    al.reset_pileup()
    assert not flat_of(al.pileup()[0]).any()
    al.align(rb, ro, m=2, effort=2)
    assert (flat_of(al.pileup()[0]) == P.pileup_of(us, k, reads[18:277], rows).flat()).all()


def test_overlapped_batch():
    """one bgr_align_batch of >= 512 k reads runs in pieces on four streams (the aligner and its twins, which add to one table): the table is the
    sum of two half-size calls', which run on one stream each"""
    k = 31
    s = Synth(150000, 90, 2, k, 5)
    seqs, offs = s.unitigs()
    us = [""] + strings(seqs, offs)
    g = B.Graph.build(k, seqs, offs)
    n = 540000
    rb, ro = s.reads(0, n, k + 20, 2, 6, threads=8)
    al = B.Aligner(g, 0)
    al.pileup_enable()
    rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
    whole, skipped = al.pileup()
    assert skipped == 0 and al.counters()["reads"] == n
    h = n // 2
    al2 = B.Aligner(g, 0)
    al2.pileup_enable()
    r1 = W.rows_of(*al2.align(rb[: int(ro[h])], ro[: h + 1], m=2, effort=2))
    first = flat_of(al2.pileup()[0])
    r2 = W.rows_of(*al2.align(rb[int(ro[h]):], ro[h:] - ro[h], m=2, effort=2))
    assert r1 + r2 == rows
    both = flat_of(al2.pileup()[0])
    assert (flat_of(whole) == both).all() and first.any() and (both - first).any()
    mapped = sum(1 for _, p in rows if p)
    assert mapped > 100000 and int(both[:, 0].sum()) == int(al2.abundance()[:, 1].sum()) > mapped   # (every mapped read covers at least a base)
    # a sample of the rows against the definition
    sample = list(range(0, 2000))
    reads = strings(rb[: int(ro[2000])], ro[:2001])
    al3 = B.Aligner(g, 0)
    al3.pileup_enable()
    assert W.rows_of(*al3.align(rb[: int(ro[2000])], ro[:2001], m=2, effort=2)) == rows[:2000]
    assert (flat_of(al3.pileup()[0]) == P.pileup_of(us, k, reads, [rows[i] for i in sample]).flat()).all()


@pytest.mark.parametrize("fastq", [False, True])
@pytest.mark.parametrize("k", [33, 63])
def test_cli_pileup_wide_k(k, fastq, tmp_path):
    unitigs, reads = graph_and_reads(k, 100 * k)
    reads = [r for r in reads if len(r) > k]   # (as test_gpu_wide_k.test_cli_k63: a FASTA reader drops the others)
    with open(tmp_path / "u.fa", "w") as f:
        for i, u in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, u))
    rf = tmp_path / ("r.fq" if fastq else "r.fa")
    heads = [("@r%d" if fastq else ">r%d") % i for i in range(len(reads))]
    with open(rf, "w") as f:
        for h, r in zip(heads, reads):
            f.write(("%s\n%s\n+\n%s\n" % (h, r, "I" * len(r))) if fastq else ("%s\n%s\n" % (h, r)))
    args = ["-r", str(rf), "-k", str(k), "-g", str(tmp_path / "u.fa"), "-m", "2", "-e", "2", "-t", "4"] + (["-q"] if fastq else [])
    ref = W.GreedyRef(k, unitigs)
    rows, cnt = ref.align(reads, 2, 2)
    us = [""] + unitigs
    p = P.pileup_of(us, k, reads, rows)
    assert cnt["aligned"] > 50 and p.skipped == 0 and sum(int(x.sum()) for x in p.alt) > 0
    _, pa, na, fa, _ = run(args)
    _, pb, nb, fb, _ = run(args + ["--host-route"])
    for f in (fa, fb):
        assert f["pileup"] == P.sites_text_of(us, p) and f["depth"] == P.depth_text_of(us, p)
    assert pa == pb == paths_bytes(heads, rows) and na == nb


def test_refusals(tmp_path):
    s = Synth(20000, 75, 2, 31, 5)
    g = B.Graph.build(31, *s.unitigs())
    al = B.Aligner(g, 0)
    rb, ro = s.reads(0, 50, 150, 2, 6)
    with pytest.raises(B.BgrError, match="error -1.*never enabled"):
        al.pileup()
    al.pileup_enable()
    with pytest.raises(B.BgrError, match="error -1.*exhaustive"):
        al.align(rb, ro, mode=B.MODE_EXHAUSTIVE)
    assert not flat_of(al.pileup()[0]).any()
    al.pileup_enable(False)
    al.abundance_enable(False)
    al.align(rb, ro, mode=B.MODE_EXHAUSTIVE)   # (not counting: exhaustive launches are welcome again)
    out = np.zeros(3, dtype=B.PILEUP_DTYPE)
    assert B.lib().bgr_aligner_pileup(al.h, out.ctypes.data, 3, None) == -1 and b"n_bases" in B.lib().bgr_last_error()
    ge = B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig_exc.fa"), 5)
    with pytest.raises(B.BgrError, match="error -1.*ACGT"):
        B.Aligner(ge, 0).pileup_enable()
    for graph, extra, word in (("deg_unitig.fa", ["-b"], "-b"), ("deg_unitig_exc.fa", [], "ACGT")):
        for flag in ("--pileup", "--depth"):
            pr = subprocess.run([B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5", "-g", os.path.join(GOLD, graph), flag, str(tmp_path / "x")] + extra,
                                cwd=tmp_path, capture_output=True, text=True, timeout=300)
            assert pr.returncode == 2 and flag in pr.stderr and word in pr.stderr and not os.path.exists(tmp_path / "x"), (graph, flag, pr.returncode, pr.stderr[-500:])


def test_align_all_keeps_the_totals_in_the_graph(tmp_path):
    case = next(c for c in CASES if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    a, us, H, R, rows = golden_rows(case)
    want = P.pileup_of(us, 31, R, rows)
    g = B.Graph.from_fasta(os.path.join(GOLD, "syn_unitig.fa"), 31)
    f = os.path.join(GOLD, "syn_r150.fa")
    with pytest.raises(B.BgrError):
        g.pileup()
    B.align_all(g, f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2, threads=2, pileup=True)
    got, skipped = g.pileup()
    assert (flat_of(got) == want.flat()).all() and skipped == 0 and not g.pileup_enabled()
    B.align_all(g, f + "," + f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2, threads=2, route=1, pileup=True)   # the next such run replaces them
    assert (flat_of(g.pileup()[0]) == 2 * want.flat()).all()
    B.align_all(g, f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2)   # a run without the switch leaves them
    assert (flat_of(g.pileup()[0]) == 2 * want.flat()).all()
    g.write_pileup(str(tmp_path / "s"))
    g.write_depth(str(tmp_path / "d"))
    want.add(P.pileup_of(us, 31, R, rows))
    assert open(tmp_path / "s", "rb").read() == P.sites_text_of(us, want) and open(tmp_path / "d", "rb").read() == P.depth_text_of(us, want)
    with pytest.raises(B.BgrError):   # a run that fails leaves none
        B.align_all(g, str(tmp_path / "missing.fa"), str(tmp_path / "p"), str(tmp_path / "n"), pileup=True)
    with pytest.raises(B.BgrError):
        g.pileup()
