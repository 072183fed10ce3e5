"""`bgreat --inside`: whole runs with the inside pass (bgr_graph_inside_enable) against the definition, byte for byte.

The rows a run must write: those of an aligner without the switch (the mapping passes as they are) with inside_ref.apply() on top.  From them
the records of `paths` and `notAligned.fa` (text route and --host-route, FASTA and -q), the --no-overlap file, the pair of files per lane of a
split run, the GAF lines with cs:Z: (gaf_ref.py, gaf_cs_ref.py), the abundance, pileup and depth files (abundance_ref.py, pileup_ref.py); with -c
a read mapped inside is written as its unitig's stretch.  Graph 1 is test_gpu_inside.py's hand-made graph, graph 2 its Synth graph at k = 31.
Error-free reads at every offset of the 400-base unitig give every base the depth of the reads that cover it -- and a hole without the flag."""
import os
import subprocess

import numpy as np
import pytest

import abundance_ref as A
import bgreat_amd as B
import gaf_cs_ref as CS
import gaf_ref as G
import inside_ref as R
import pileup_ref as P
from test_gpu_inside import K1, SEED, _pack, _synth_case, graph1, rc, reads1
from test_gpu_wide_k import parse_records
from wide_greedy_ref import rows_of

M = 2


class _Run:
    """a graph and reads on disk, the reference's rows, and the CLI in a directory of its own per call"""

    def __init__(self, tmp, k, us, reads):
        self.k, self.us, self.reads, self.tmp = k, us, reads, tmp
        self.us1 = [""] + us   # (the reference's vector: ids from 1)
        self.heads = [">r%d" % i for i in range(len(reads))]
        with open(tmp / "u.fa", "w") as f:
            for i, u in enumerate(us):
                f.write(">%d\n%s\n" % (i, u))
        with open(tmp / "r.fa", "w") as f:
            for h, r in zip(self.heads, reads):
                f.write("%s\n%s\n" % (h, r))
        with open(tmp / "r.fq", "w") as f:
            for i, r in enumerate(reads):
                f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
        g = B.Graph.build(k, *_pack(us))
        self.rows0 = rows_of(*B.Aligner(g, 0).align(*_pack(reads), m=M, effort=2))
        self.rows, self.n_in = R.apply(k, us, R.index(k, us), reads, self.rows0, M)
        self.n = 0

    def cli(self, extra, fastq=False, ok=True):
        """-> (stdout, directory the run wrote into)"""
        d = self.tmp / ("run%d" % self.n)
        self.n += 1
        d.mkdir()
        args = [B.CLI_PATH, "-r", str(self.tmp / ("r.fq" if fastq else "r.fa")), "-k", str(self.k), "-g", str(self.tmp / "u.fa"), "-m", str(M), "-e", "2", "-t", "4"]
        p = subprocess.run(args + (["-q"] if fastq else []) + extra, cwd=d, capture_output=True, text=True, timeout=300)
        assert (p.returncode == 0) == ok, p.stderr[-2000:]
        return p, d

    def records(self, rows, at=">"):
        heads = [at + h[1:] for h in self.heads]
        paths = "".join(h + "\n" + "".join("%d." % v for v in path) + "\n" for h, (_, path) in zip(heads, rows) if path)
        rest = "".join(h + "\n" + r + "\n" for h, r, (_, path) in zip(heads, self.reads, rows) if not path)
        return paths.encode(), rest.encode()


def _read(d, name):
    return open(d / name, "rb").read()


def _make(tmp_path_factory, which):
    tmp = tmp_path_factory.mktemp("inside_" + which)
    if which == "g1":
        us = graph1()
        reads = [r for _, r in reads1(us, M) if len(r) > K1]   # (a FASTA reader drops reads of at most k characters)
        return _Run(tmp, K1, us, reads)
    k, us, reads = _synth_case(31)
    return _Run(tmp, k, us, reads)


@pytest.fixture(scope="module", params=["g1", "g2"])
def run(request, tmp_path_factory):
    return _make(tmp_path_factory, request.param)


@pytest.mark.gpu
def test_paths_and_not_aligned_on_both_routes(run):
    assert run.n_in >= 20 and run.rows != run.rows0
    want_p, want_n = run.records(run.rows)
    for extra in ([], ["--host-route"]):
        p, d = run.cli(["--inside"] + extra)
        assert _read(d, "paths") == want_p and _read(d, "notAligned.fa") == want_n, extra
        lines = p.stdout.split("\n")
        assert lines[-2] == "Mapped inside a unitig : %d" % run.n_in and lines[-1] == ""
        assert lines[-3].startswith("Mapping in seconds : ")
    # without the flag: the bytes and the lines of today
    p, d = run.cli([])
    old_p, old_n = run.records(run.rows0)
    assert _read(d, "paths") == old_p and _read(d, "notAligned.fa") == old_n
    assert "Mapped inside" not in p.stdout and p.stdout.split("\n")[-2].startswith("Mapping in seconds : ")


@pytest.mark.gpu
def test_fastq(run):
    want_p, want_n = run.records(run.rows, at="@")
    for extra in ([], ["--host-route"]):
        _, d = run.cli(["--inside"] + extra, fastq=True)
        # (the FASTQ reader hands on one more record at the end of the file, without a header line, on both routes alike: it maps, or not, like any other)
        named = lambda b: [r for r in parse_records(b) if r[0]]
        assert named(_read(d, "paths")) == parse_records(want_p) and named(_read(d, "notAligned.fa")) == parse_records(want_n), extra


@pytest.mark.gpu
def test_corrected_reads_are_the_unitigs_stretch(run):
    _, d0 = run.cli(["-c"])
    old = dict(parse_records(_read(d0, "paths")))
    for extra in ([], ["--host-route"]):
        _, d = run.cli(["--inside", "-c"] + extra)
        got = parse_records(_read(d, "paths"))
        assert [h for h, _ in got] == [h for h, (_, path) in zip(run.heads, run.rows) if path]
        got = dict(got)
        n = 0
        for h, r, (st0, _), (st, path) in zip(run.heads, run.reads, run.rows0, run.rows):
            if not path:
                continue
            if (st0 & B.ST_MASK) == B.ST_NOANCHOR:   # mapped inside: the oriented unitig's [s, s + L)
                u = run.us[abs(path[1]) - 1]
                assert got[h] == (u if path[1] > 0 else rc(u))[path[0]:path[0] + len(r)], h
                n += 1
            else:
                assert got[h] == old[h], h
        assert n == run.n_in
        want_n = run.records(run.rows)[1]
        assert _read(d, "notAligned.fa") == want_n


@pytest.mark.gpu
def test_no_overlap_file_loses_the_reads_mapped_inside(run):
    _, d = run.cli(["--inside", "--no-overlap", "noov.fa"])
    want_p = run.records(run.rows)[0]
    assert _read(d, "paths") == want_p
    no_anchor = "".join(h + "\n" + r + "\n" for h, r, (st, path) in zip(run.heads, run.reads, run.rows) if not path and (st & B.ST_MASK) == B.ST_NOANCHOR)
    failed = "".join(h + "\n" + r + "\n" for h, r, (st, path) in zip(run.heads, run.reads, run.rows) if not path and (st & B.ST_MASK) != B.ST_NOANCHOR)
    assert _read(d, "noov.fa") == no_anchor.encode() and _read(d, "notAligned.fa") == failed.encode()


@pytest.mark.gpu
def test_split_output_on_two_lanes(run):
    _, d = run.cli(["--inside", "--gpus", "2", "--split-output", "--set", "test.lanes_on_one_device=1"])
    want_p, want_n = run.records(run.rows)
    assert b"".join(_read(d, "paths.%d" % i) for i in range(2)) == want_p
    assert b"".join(_read(d, "notAligned.fa.%d" % i) for i in range(2)) == want_n


@pytest.mark.gpu
def test_gaf_lines_with_cs(run):
    want = CS.gaf_cs_of(run.us1, run.k, run.heads, run.reads, run.rows)[0]
    plain = G.gaf_of(run.us1, run.k, run.heads, run.reads, run.rows)[0]
    assert want.count("\n") == plain.count("\n") == sum(1 for _, path in run.rows if path)
    for extra in ([], ["--host-route"]):
        _, d = run.cli(["--inside", "--gaf", "--cs"] + extra)
        assert _read(d, "paths").decode() == want, extra
    _, d = run.cli(["--inside", "--gaf"])
    assert _read(d, "paths").decode() == plain


@pytest.mark.gpu
def test_counting_flags_count_the_reads_mapped_inside(run):
    _, d = run.cli(["--inside", "--abundance", "ab.tsv", "--pileup", "pile.tsv", "--depth", "depth.tsv"])
    lens = A.unitig_lens(run.us1)
    assert _read(d, "ab.tsv") == A.text_of(lens, A.abundance_of(lens, run.k, [len(r) for r in run.reads], run.rows))
    p = P.pileup_of(run.us1, run.k, run.reads, run.rows)
    assert _read(d, "pile.tsv") == P.sites_text_of(run.us1, p)
    assert _read(d, "depth.tsv") == P.depth_text_of(run.us1, p)
    # and differ from what the same run counts without the flag
    _, d0 = run.cli(["--abundance", "ab.tsv", "--depth", "depth.tsv"])
    p0 = P.pileup_of(run.us1, run.k, run.reads, run.rows0)
    assert _read(d0, "depth.tsv") == P.depth_text_of(run.us1, p0) != _read(d, "depth.tsv")
    assert _read(d0, "ab.tsv") != _read(d, "ab.tsv")


def _depth_of(text, unitig, length):
    d = np.zeros(length, dtype=np.int64)
    for ln in text.decode().split("\n")[:-1]:
        u, a, b, v = (int(x) for x in ln.split("\t"))
        if u == unitig:
            d[a:b] = v
    return d


@pytest.mark.gpu
def test_every_base_of_a_long_unitig_has_the_depth_of_the_reads_that_cover_it(tmp_path_factory):
    us = graph1()
    U, L = us[0], 150
    reads = [U[i:i + L] for i in range(len(U) - L + 1)]   # error-free, at every offset
    run = _Run(tmp_path_factory.mktemp("inside_depth"), K1, us, reads)
    cover = np.zeros(len(U), dtype=np.int64)
    for i in range(len(reads)):
        cover[i:i + L] += 1
    _, d = run.cli(["--inside", "--depth", "depth.tsv"])
    assert np.array_equal(_depth_of(_read(d, "depth.tsv"), 1, len(U)), cover)
    _, d0 = run.cli(["--depth", "depth.tsv"])
    hole = _depth_of(_read(d0, "depth.tsv"), 1, len(U))
    assert hole.max() <= 2 and hole[150:250].max() == 0 and cover[150:250].min() == 150   # only the two reads at the ends hold an overlap (k-1)-mer


@pytest.mark.gpu
def test_refusals(tmp_path):
    rng = np.random.default_rng(SEED + 9)
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))
    u = rnd(300)
    (tmp_path / "u.fa").write_text(">0\n%s\n>1\n%s\n" % (u, rnd(200)))
    (tmp_path / "un.fa").write_text(">0\n%s\n>1\n%s\n" % (u[:100] + "N" + u[101:], rnd(200)))
    (tmp_path / "r.fa").write_text(">r0\n%s\n" % u[50:200])
    base = [B.CLI_PATH, "-r", str(tmp_path / "r.fa"), "-m", "2"]
    for extra, msg in ((["-g", str(tmp_path / "u.fa"), "-k", "31", "-b"], "-b"), (["-g", str(tmp_path / "u.fa"), "-k", "33"], "k <= 32"),
                       (["-g", str(tmp_path / "un.fa"), "-k", "31"], "ACGT")):
        p = subprocess.run(base + extra + ["--inside"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and msg in p.stderr, (extra, p.returncode, p.stderr[-500:])
        p = subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)   # (without the flag the same run is none of its business)
        assert p.returncode == 0, (extra, p.stderr[-500:])
