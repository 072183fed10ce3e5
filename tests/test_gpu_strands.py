"""The pileup per strand on the GPU: the forward table of bgr_aligner_pileup_strands_enable behind every read source, the sites of
bgr_aligner_pileup_strand_sites on graphs whose difference array crosses the tiles of the passes, the add path, and whole runs (bgr_align_all, the
CLI's --strands / --min-alt-strand on both routes and with two lanes) -- against strands_ref.py (the definition in plain Python, pinned by
test_strands_host.py) over rows of the oracle (goldens) or of the batch API itself (pinned to the oracle elsewhere).

The shapes and their helpers are test_gpu_variants.py's (copied: a random genome cut into unitigs that overlap by k - 1, reads that are windows
of the genome with one character substituted).  A unitig is a piece of the genome as it stands, so a read given as a window of the genome is a
forward observation on every unitig it lies on and a read given as the reverse complement of one is not -- whatever strand the mapper reports.

The internal streams of an overlapped batch (twins) are covered by test_overlapped_batch below, as in test_gpu_pileup.py."""
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bgreat_amd as B
import pileup_ref as P
import strands_ref as S
import variants_ref as V
import wide_greedy_ref as W
from test_gaf_host import golden_rows
from test_strands_host import GOLDENS, case_of, rc
from test_wide_k_host import pack, strings
from tools.synth import Synth
from util import GOLD, parse_counters, resolve_args, sha

pytestmark = pytest.mark.gpu

TILE = B.VARIANTS_TILE


def flat_of(arr):
    return np.stack([arr[f] for f in B.PILEUP_DTYPE.names], axis=1).astype(np.int64)


def as_tuples(sites):
    return [tuple(int(v) for v in s)[:14] for s in sites]


def strands_aligner(g):
    al = B.Aligner(g, 0)
    al.pileup_strands_enable()
    return al


# ---- 1. the goldens through the batch API ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reads,graph,k", GOLDENS)
def test_forward_table_on_the_goldens(reads, graph, k):
    a, us, H, R, rows = golden_rows(case_of(reads, graph))
    combos = {}
    want_f, want_p = S.forward_of(us, k, R, rows, combos), P.pileup_of(us, k, R, rows)
    assert all(combos.get((x, y), 0) > 0 for x in (False, True) for y in (False, True)), combos   # (one-strand data could not tell the tables apart)
    g = B.Graph.from_fasta(os.path.join(GOLD, graph), k)
    al = B.Aligner(g, 0)
    with pytest.raises(B.BgrError, match="error -1.*never"):
        al.pileup_forward()
    al.pileup_strands_enable()
    assert not flat_of(al.pileup_forward()).any() and not flat_of(al.pileup()[0]).any()   # (the switch enabled the pileup as well)
    rb, ro = pack(R)
    assert W.rows_of(*al.align(rb, ro, m=2, effort=2)) == rows
    fwd, (tot, skipped) = flat_of(al.pileup_forward()), al.pileup()
    assert (fwd == want_f.flat()).all() and (flat_of(tot) == want_p.flat()).all() and skipped == 0
    assert fwd.any() and (fwd <= flat_of(tot)).all() and (fwd != flat_of(tot)).any()
    # the sites under the strand filter; 0 is bgr_aligner_pileup_sites' set, which the switch leaves as it is
    for prm in ((2, 2, 200000), (1, 1, 0)):
        for strand in (0, 1, 2):
            assert as_tuples(al.pileup_strand_sites(*prm, strand)) == S.sites_of(want_p, want_f, *prm, strand), (prm, strand)
        assert [s[:8] for s in as_tuples(al.pileup_strand_sites(*prm, 0))] == [tuple(int(v) for v in s) for s in al.pileup_sites(*prm)] == V.sites_of(want_p, *prm)
    # switching off keeps the table and leaves the pileup on: the next launch adds to the total alone
    al.pileup_strands_enable(False)
    al.align(rb, ro, m=2, effort=2)
    assert (flat_of(al.pileup_forward()) == want_f.flat()).all() and (flat_of(al.pileup()[0]) == 2 * want_p.flat()).all()
    al.pileup_strands_enable()
    al.reset_pileup()   # clears both
    assert not flat_of(al.pileup_forward()).any() and not flat_of(al.pileup()[0]).any()
    al.align(rb, ro, m=2, effort=2)
    assert (flat_of(al.pileup_forward()) == want_f.flat()).all() and (flat_of(al.pileup()[0]) == want_p.flat()).all()


# ---- the chosen shapes (test_gpu_variants.py's helpers) --------------------------------------------------------------------------------------

def chain(k, lens, seed):
    """a random genome cut into unitigs of the lengths `lens` that overlap by k - 1 -> (unitigs with unitigs[0] == "", genome, the unitigs' first genome positions)"""
    rnd = random.Random(seed)
    assert all(n >= k for n in lens)
    genome = "".join(rnd.choice("ACGT") for _ in range(sum(n - (k - 1) for n in lens) + k - 1))
    starts, at = [0], 0
    for n in lens:
        at += n - (k - 1)
        starts.append(at)
    return [""] + [genome[starts[i]:starts[i] + n] for i, n in enumerate(lens)], genome, [None] + starts[:-1]


def window_read(genome, x, sub=None, half=3500):
    """the genome around position x (long enough to hold a junction of any unitig of the shape below), with `sub` at x"""
    lo, hi = max(0, x - half), min(len(genome), x + half)
    r = genome[lo:hi]
    return r if sub is None else r[:x - lo] + sub + r[x - lo + 1:]


def tiles_shape(k):
    """five unitigs, a difference array of 5 x TILE + 378 words -> (unitig lengths, the genome positions at the places the passes can go wrong:
    position 0 and len - 1 of unitigs, the last word of a tile and the first word of the next)"""
    long = 3 * TILE + 100
    lens = [TILE - 1, long, 5 * TILE - 1 - (TILE + long + 1) - 1, 300, 77]
    starts, at = [], 0
    for n in lens:
        starts.append(at)
        at += n - (k - 1)
    total = at + k - 1
    word0 = [sum(n + 1 for n in lens[:i]) for i in range(len(lens))]
    assert word0[1] == TILE and word0[3] == 5 * TILE - 1 and sum(lens) + len(lens) == 5 * TILE + 378
    edge = lambda u, w: starts[u] + (w - word0[u])   # genome position of the base at word w of unitig u (0-based here)
    places = [0, starts[0] + lens[0] - 1, starts[1], starts[1] + lens[1] - 1, starts[3], total - 1,
              edge(1, 2 * TILE - 1), edge(1, 2 * TILE), edge(1, 3 * TILE - 1), edge(1, 3 * TILE), edge(1, 4 * TILE - 1), edge(1, 4 * TILE)]
    return lens, places, total


def strand_plants(genome, places, seed):
    """at every one of `places` an allele on ONE strand only (three reads; forward at the even places, reverse at the odd ones), and next to each
    an allele on BOTH strands (two reads each); whole-genome reads on both strands and reads with an N on top
    -> (reads as given, one-strand genome positions, both-strand genome positions)"""
    rnd = random.Random(seed)
    taken, both = set(places), []
    for x in places:
        y = next(x + d for d in (1, -1, 2, -2, 3, -3, 4, -4) if 0 <= x + d < len(genome) and x + d not in taken)
        taken.add(y)
        both.append(y)
    reads = []
    sub = lambda x: rnd.choice([c for c in "ACGT" if c != genome[x]])
    for i, x in enumerate(places):
        r = window_read(genome, x, sub(x))
        reads += [r if i % 2 == 0 else rc(r)] * 3
    for y in both:
        r = window_read(genome, y, sub(y))
        reads += [r, r, rc(r), rc(r)]
    reads += [genome, rc(genome), window_read(genome, places[2], "N"), rc(window_read(genome, places[3], "N")), window_read(genome, both[0] + 9, "N")]
    rnd.shuffle(reads)
    return reads, list(places), both


def ref_tables(us, k, reads, rows):
    return P.pileup_of(us, k, reads, rows), S.forward_of(us, k, reads, rows)


@pytest.mark.parametrize("k", [15, 31, 33, 64])
def test_strand_sites_at_the_tile_edges(k):
    lens, places, total = tiles_shape(k)
    us, genome, starts = chain(k, lens, 11 * k + 3)
    assert len(genome) == total
    seqs, offs = pack(us[1:])
    g = B.Graph.build(k, seqs, offs)
    al = B.Aligner(g, 0)
    al.pileup_enable()
    with pytest.raises(B.BgrError, match="error -1.*never"):   # the pileup alone has no forward table
        al.pileup_strand_sites(1, 1, 0, 0)
    al.pileup_strands_enable()
    assert len(al.pileup_strand_sites(1, 1, 0, 0)) == 0   # empty tables
    for prm in ((0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 1000001, 0)):
        with pytest.raises(B.BgrError, match="error -1.*thresholds"):
            al.pileup_strand_sites(*prm)
    reads, one, both = strand_plants(genome, places, k)
    rb, ro = pack(reads)
    rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
    assert all(p for _, p in rows)
    p, f = ref_tables(us, k, reads, rows)
    assert (flat_of(al.pileup_forward()) == f.flat()).all() and (flat_of(al.pileup()[0]) == p.flat()).all()
    gpos = lambda s: starts[s[0]] + s[1]
    got = {}
    for prm in ((1, 2, 0), (2, 2, 200000), (1, 1, 0)):
        for strand in (0, 1, 2):
            want = S.sites_of(p, f, *prm, strand)
            got[prm, strand] = as_tuples(al.pileup_strand_sites(*prm, strand))
            assert got[prm, strand] == want, (k, prm, strand, len(got[prm, strand]), len(want))
        assert [s[:8] for s in got[prm, 0]] == [tuple(int(v) for v in s) for s in al.pileup_sites(*prm)]   # 0 is today's site set, and the plain call is untouched
    # at 1 exactly the one-strand plants disappear; at 2 the both-strand ones (two reads on each strand) are still there, at 3 none is
    assert {gpos(s) for s in got[(1, 2, 0), 0]} == set(one) | set(both)
    assert {gpos(s) for s in got[(1, 2, 0), 1]} == set(both) == {gpos(s) for s in got[(1, 2, 0), 2]}
    assert len(al.pileup_strand_sites(1, 2, 0, 3)) == 0
    for s in got[(1, 2, 0), 0]:
        x = gpos(s)
        if x in both:
            assert sum(s[3:7]) == 4 and sum(s[9:13]) == 2, s
        else:
            assert sum(s[3:7]) == 3 and sum(s[9:13]) == (3 if places.index(x) % 2 == 0 else 0), s
    sites0 = {(s[0], s[1]) for s in got[(1, 2, 0), 0]}
    assert {(1, 0), (1, lens[0] - 1), (2, 0), (2, lens[1] - 1), (4, 0), (5, lens[4] - 1)} <= sites0
    assert {(2, w - TILE) for e in (2, 3, 4) for w in (e * TILE - 1, e * TILE)} <= sites0
    assert any(s[7] for s in got[(1, 1, 0), 0]) and any(s[13] for s in got[(1, 1, 0), 0])   # Ns beside an allele, on the forward strand too
    # a buffer one record too small: BGR_E_CAPACITY with the number, nothing written; then with room
    L = B.lib()
    prm = B.VariantStrandParams(1, 2, 0, 1)
    want = got[(1, 2, 0), 1]
    cnt = B.C.c_uint64(0)
    out = np.zeros(len(want), dtype=B.VARIANT_STRAND_DTYPE)
    assert L.bgr_aligner_pileup_strand_sites(al.h, B.C.byref(prm), out.ctypes.data, len(want) - 1, B.C.byref(cnt)) == -4 and cnt.value == len(want)
    assert b"room for %d" % (len(want) - 1) in L.bgr_last_error() and not out["unitig"].any()
    assert L.bgr_aligner_pileup_strand_sites(al.h, B.C.byref(prm), out.ctypes.data, len(want), B.C.byref(cnt)) == 0 and cnt.value == len(want)
    assert as_tuples(out) == want and not out["reserved0"].any() and not out["reserved1"].any()
    assert all(x > 0 for x in al.pileup_sites_times())


# ---- 2. the three read sources ---------------------------------------------------------------------------------------------------------------

def test_read_sources_agree():
    """the same reads as ASCII (bgr_align_batch), as a FASTA text (the text form) and as 2-bit planes (bgr_align_batch_packed): one forward table"""
    k = 31
    lens, places, total = tiles_shape(k)
    us, genome, starts = chain(k, lens, 5)
    seqs, offs = pack(us[1:])
    g = B.Graph.build(k, seqs, offs)
    reads, one, both = strand_plants(genome, places, 17)
    assert sum("N" in r for r in reads) == 3
    rb, ro = pack(reads)
    a1, a2, a3 = strands_aligner(g), strands_aligner(g), strands_aligner(g)
    rows = W.rows_of(*a1.align(rb, ro, m=2, effort=2))
    text = "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)).encode()
    pt, na, info = a2.align_fasta_text(text, m=2, effort=2)
    assert not info["irregular"]
    assert W.rows_of(*a3.align_packed(B.pack_reads(rb, ro), m=2, effort=2)) == rows
    p, f = ref_tables(us, k, reads, rows)
    for al in (a1, a2, a3):
        assert (flat_of(al.pileup_forward()) == f.flat()).all() and (flat_of(al.pileup()[0]) == p.flat()).all()
    assert f.flat()[:, 5].any() and (p.flat()[:, 5] - f.flat()[:, 5]).any()   # an N on each strand


# ---- 4. batching, streams, adds --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stage", [0, 4096])
def test_split_launches_and_add_path(stage):
    k = 31
    lens, places, total = tiles_shape(k)
    us, genome, starts = chain(k, lens, 99)
    seqs, offs = pack(us[1:])
    g = B.Graph.build(k, seqs, offs)
    reads, one, both = strand_plants(genome, places, 5)
    h = len(reads) // 2
    def mapped(al, batch):
        rb, ro = pack(batch)
        return W.rows_of(*al.align(rb, ro, m=2, effort=2))
    whole, split, a, b = strands_aligner(g), strands_aligner(g), strands_aligner(g), strands_aligner(g)
    rows = mapped(whole, reads)
    assert mapped(split, reads[:h]) + mapped(split, reads[h:]) == rows   # two launches = one
    assert mapped(a, reads[:h]) + mapped(b, reads[h:]) == rows
    fw, tw = flat_of(whole.pileup_forward()), flat_of(whole.pileup()[0])
    assert (flat_of(split.pileup_forward()) == fw).all() and (flat_of(split.pileup()[0]) == tw).all()
    fa, fb = flat_of(a.pileup_forward()), flat_of(b.pileup_forward())
    with B.options(**{"test.variants_stage_bytes": stage}):
        a.pileup_add(b)
    assert (flat_of(a.pileup_forward()) == fa + fb).all() and (fa + fb == fw).all() and fa.any() and fb.any()
    assert (flat_of(b.pileup_forward()) == fb).all() and (flat_of(a.pileup()[0]) == tw).all()
    for strand in (0, 1, 2):
        assert as_tuples(a.pileup_strand_sites(1, 2, 0, strand)) == as_tuples(whole.pileup_strand_sites(1, 2, 0, strand))
    assert as_tuples(b.pileup_strand_sites(1, 2, 0, 1)) != as_tuples(whole.pileup_strand_sites(1, 2, 0, 1))
    # exactly one side with a forward table: refused either way, and nothing is added
    plain = B.Aligner(g, 0)
    plain.pileup_enable()
    mapped(plain, reads[:h])
    before = flat_of(plain.pileup()[0])
    for x, y in ((a, plain), (plain, a)):
        with pytest.raises(B.BgrError, match="error -1.*forward table"):
            x.pileup_add(y)
    assert (flat_of(plain.pileup()[0]) == before).all() and (flat_of(a.pileup()[0]) == tw).all() and (flat_of(a.pileup_forward()) == fw).all()


def test_overlapped_batch():
    """one bgr_align_batch of >= 512 k reads runs in pieces on four streams (the aligner and its twins, which share both tables): the forward
    table is the sum of two half-size calls', which run on one stream each (test_gpu_pileup.test_overlapped_batch's way to force the twins)"""
    k = 31
    s = Synth(150000, 90, 2, k, 5)
    seqs, offs = s.unitigs()
    g = B.Graph.build(k, seqs, offs)
    n = 540000
    rb, ro = s.reads(0, n, k + 20, 2, 6, threads=8)
    al = strands_aligner(g)
    rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
    h = n // 2
    al2 = strands_aligner(g)
    r1 = W.rows_of(*al2.align(rb[: int(ro[h])], ro[: h + 1], m=2, effort=2))
    first = flat_of(al2.pileup_forward())
    r2 = W.rows_of(*al2.align(rb[int(ro[h]):], ro[h:] - ro[h], m=2, effort=2))
    assert r1 + r2 == rows
    both, whole = flat_of(al2.pileup_forward()), flat_of(al.pileup_forward())
    assert (whole == both).all() and first.any() and (both - first).any()
    tot = flat_of(al.pileup()[0])
    assert (tot == flat_of(al2.pileup()[0])).all() and (whole <= tot).all() and 0 < int(whole[:, 0].sum()) < int(tot[:, 0].sum())
    # a sample of the rows against the definition
    us = [""] + strings(seqs, offs)
    reads = strings(rb[: int(ro[2000])], ro[:2001])
    al3 = strands_aligner(g)
    assert W.rows_of(*al3.align(rb[: int(ro[2000])], ro[:2001], m=2, effort=2)) == rows[:2000]
    assert (flat_of(al3.pileup_forward()) == S.forward_of(us, k, reads, rows[:2000]).flat()).all()


# ---- 5. whole runs ---------------------------------------------------------------------------------------------------------------------------

FILES = {"vcf": "sites.vcf", "pileup": "pile.tsv", "depth": "depth.bed"}


def run(args, flags, more=(), timeout=600):
    """the CLI in a scratch directory, with a file for each of `flags` -> (stdout, paths bytes, notAligned bytes, {flag: bytes or None})"""
    d = tempfile.mkdtemp()
    try:
        files = [x for f in flags for x in ("--" + f, os.path.join(d, FILES[f]))]
        p = subprocess.run([B.CLI_PATH] + list(args) + files + list(more), cwd=d, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:
            raise RuntimeError("%s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
        def cat(name):
            if os.path.exists(os.path.join(d, name + ".0")):
                return b"".join(open(os.path.join(d, "%s.%d" % (name, i)), "rb").read() for i in range(8) if os.path.exists(os.path.join(d, "%s.%d" % (name, i))))
            return open(os.path.join(d, name), "rb").read() if os.path.exists(os.path.join(d, name)) else None
        return p.stdout, cat("paths") or b"", cat("notAligned.fa") or b"", {f: cat(FILES[f]) for f in FILES}
    finally:
        shutil.rmtree(d)


@pytest.mark.parametrize("reads,graph,k", GOLDENS)
def test_cli_on_the_goldens(reads, graph, k):
    case = case_of(reads, graph)
    a, us, H, R, rows = golden_rows(case)
    p, f = ref_tables(us, k, R, rows)
    # the default thresholds on the degenerate graph (10 sites, 4 of them read on both strands); on the synthetic one every differing base is a
    # site (478; its alleles are single reads, so none is read on both strands and --min-alt-strand 1 leaves the header alone)
    t = (2, 2, 200000) if graph == "deg_unitig.fa" else (1, 1, 0)
    prm = ["--min-depth", str(t[0]), "--min-alt", str(t[1]), "--min-af", "0.2" if t[2] else "0"]
    want_pile = S.sites_text_of(us, p, f)
    want_vcf = {s: S.vcf_text_of(us, S.sites_of(p, f, *t, s), *t, s) for s in (0, 1)}
    assert b"\t.\tPASS\t" in want_vcf[0] and (b"\t.\tPASS\t" in want_vcf[1]) == (graph == "deg_unitig.fa") and len(want_vcf[1]) < len(want_vcf[0])
    lanes = ["--gpus", "2", "--set", "test.lanes_on_one_device=1"]
    for extra in ([], ["--host-route"], lanes + ["--set", "test.variants_stage_bytes=4096"]):
        args = resolve_args(case["args"]) + extra
        out, paths, na, got = run(args, ("pileup", "vcf", "depth"), prm + ["--min-alt-strand", "1"])   # (--min-alt-strand implies --strands)
        assert got["pileup"] == want_pile and got["vcf"] == want_vcf[1] and got["depth"] == P.depth_text_of(us, p), (reads, extra)
        assert parse_counters(out) == case["counters"] and sha(paths) == case["paths_sha256"] and sha(na) == case["notaligned_sha256"], (reads, extra)
    args = resolve_args(case["args"]) + lanes
    out, paths, na, got = run(args, ("vcf",), prm + ["--strands"])   # --vcf alone: the forward table stays on the devices, added there from the second lane
    assert got["vcf"] == want_vcf[0] and got["pileup"] is None and parse_counters(out) == case["counters"], reads
    out, paths, na, got = run(args, ("pileup",), ["--strands"])
    assert got["pileup"] == want_pile and got["vcf"] is None and sha(paths) == case["paths_sha256"], reads
    # the same run without the new flags: the bytes of today's writers
    out, paths, na, got = run(resolve_args(case["args"]), ("pileup", "vcf"), prm)
    assert got["pileup"] == P.sites_text_of(us, p) and got["vcf"] == V.vcf_text_of(us, V.sites_of(p, *t), *t)


def test_align_all_keeps_both_tables(tmp_path):
    reads, graph, k = GOLDENS[0]   # (the degenerate graph: its sites survive the strand filter)
    a, us, H, R, rows = golden_rows(case_of(reads, graph))
    p, f = ref_tables(us, k, R, rows)
    g = B.Graph.from_fasta(os.path.join(GOLD, graph), k)
    fa = os.path.join(GOLD, reads)
    g.pileup_strands_enable()
    B.align_all(g, fa, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2, threads=2)
    assert (flat_of(g.pileup_forward()) == f.flat()).all() and (flat_of(g.pileup()[0]) == p.flat()).all()
    g.write_pileup_strands(str(tmp_path / "s"))
    g.write_pileup(str(tmp_path / "t"))
    assert open(tmp_path / "s", "rb").read() == S.sites_text_of(us, p, f) and open(tmp_path / "t", "rb").read() == P.sites_text_of(us, p)
    with pytest.raises(B.BgrError, match="no totals"):
        g.variant_strand_sites()
    # both switches, the host route, the file twice: the forward table travels with the run's table and is gathered as well
    g.variants_strands_enable(2, 2, 200000, 1)
    B.align_all(g, fa + "," + fa, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2, threads=2, route=1)
    p2, f2 = ref_tables(us, k, R + R, rows + rows)
    assert as_tuples(g.variant_strand_sites()) == S.sites_of(p2, f2, 2, 2, 200000, 1) and len(g.variant_strand_sites()) > 0
    assert [tuple(int(v) for v in s) for s in g.variants()] == [s[:8] for s in S.sites_of(p2, f2, 2, 2, 200000, 1)]
    assert (flat_of(g.pileup_forward()) == f2.flat()).all() and (flat_of(g.pileup()[0]) == p2.flat()).all()
    g.write_vcf_strands(str(tmp_path / "v"), g.variant_strand_sites(), (2, 2, 200000, 1))
    assert open(tmp_path / "v", "rb").read() == S.vcf_text_of(us, S.sites_of(p2, f2, 2, 2, 200000, 1), 2, 2, 200000, 1)
    # the strands switch off again: the pileup stays on, the forward totals go; the plain variants switch: no strand sites
    g.pileup_strands_enable(False)
    g.variants_enable(2, 2, 200000)
    B.align_all(g, fa, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2)
    assert (flat_of(g.pileup()[0]) == p.flat()).all() and [tuple(int(v) for v in s) for s in g.variants()] == V.sites_of(p, 2, 2, 200000)
    with pytest.raises(B.BgrError, match="no forward totals"):
        g.pileup_forward()
    with pytest.raises(B.BgrError, match="no totals"):
        g.variant_strand_sites()


def test_refusals(tmp_path):
    base = [B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5", "-g", os.path.join(GOLD, "deg_unitig.fa")]
    x = str(tmp_path / "x")
    def cli(*more):
        return subprocess.run(base + list(more), cwd=tmp_path, capture_output=True, text=True, timeout=300)
    for more in (["--strands"], ["--strands", "--depth", x], ["--strands", "--abundance", x]):   # --strands needs --pileup or --vcf
        pr = cli(*more)
        assert pr.returncode == 2 and "--strands" in pr.stderr and "--pileup" in pr.stderr and "--vcf" in pr.stderr and not os.path.exists(x), (more, pr.stderr[-500:])
    for more in (["--min-alt-strand", "1"], ["--min-alt-strand", "1", "--pileup", x], ["--min-alt-strand", "0", "--strands", "--pileup", x]):   # ... --min-alt-strand --vcf
        pr = cli(*more)
        assert pr.returncode == 2 and "--min-alt-strand" in pr.stderr and "--vcf" in pr.stderr and not os.path.exists(x), (more, pr.stderr[-500:])
    for bad in ("-1", "x", "", "1.5", "1000000000", "+1", "0x1"):   # digits only, at most nine
        pr = cli("--vcf", x, "--min-alt-strand", bad)
        assert pr.returncode == 2 and "--min-alt-strand" in pr.stderr and not os.path.exists(x), (bad, pr.stderr[-500:])
    pr = cli("--vcf", x, "--strands", "-b")   # the refusals of --vcf stand
    assert pr.returncode == 2 and "--vcf" in pr.stderr and "-b" in pr.stderr and not os.path.exists(x), pr.stderr[-500:]
    assert B.parse_min_alt_strand("000000007") == 7
