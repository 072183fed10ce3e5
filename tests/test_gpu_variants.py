"""SNV sites on the GPU: `--vcf` through the CLI on every route against variants_ref.py over the oracle's rows (goldens), and
bgr_aligner_pileup_sites / bgr_aligner_pileup_add against variants_ref applied to the same aligner's pileup() -- the host path
test_gpu_pileup.py pins -- on graphs whose difference array ends below, on and just behind a tile of the passes, with a unitig across several
tiles, unitig boundaries on both sides of a tile edge and sites planted at every such place.

The graphs are a random genome cut into unitigs that overlap by k - 1 characters, so the number of words T + n is set exactly; a read is a
window of the genome around a junction (the mapper anchors reads on the overlaps), with one character substituted where a site is planted."""
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
import variants_ref as V
import wide_greedy_ref as W
from test_gaf_host import gaf_cases, golden_rows
from test_wide_k_host import pack
from util import GOLD, parse_counters, resolve_args, sha

pytestmark = pytest.mark.gpu

CASES = gaf_cases()
TILE = B.VARIANTS_TILE
FILES = {"vcf": "sites.vcf", "pileup": "pile.tsv", "depth": "depth.bed", "gfa": "g.gfa"}


def run(args, flags=("vcf",), more=(), timeout=600):
    """the CLI in a scratch directory, with a file for each of `flags` -> (stdout, paths bytes -- the pairs of a split run concatenated --,
    notAligned bytes, {flag: bytes or None}, the names in the directory)"""
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
        return p.stdout, cat("paths") or b"", cat("notAligned.fa") or b"", {f: cat(FILES[f]) for f in FILES}, sorted(os.listdir(d))
    finally:
        shutil.rmtree(d)


ALL = ["--min-depth", "1", "--min-alt", "1", "--min-af", "0"]   # every base with an ACGT disagreement is a site


@pytest.mark.parametrize("case", CASES, ids=["%02d-%s" % (c["id"], c["group"]) for c in CASES])
def test_cli_vcf_on_the_goldens(case):
    """the VCF = variants_ref over the oracle's rows, whatever the route, the batching, the key layout and the number of lanes (the second
    lane's table is added into the first one's on the device); paths, notAligned.fa and the counters stay the golden's"""
    a, us, H, R, rows = golden_rows(case)
    p = P.pileup_of(us, a["k"], R, rows)
    assert p.skipped == 0
    want = V.vcf_text_of(us, V.sites_of(p, 1, 1, 0), 1, 1, 0)
    lanes = ["--gpus", "2", "--set", "test.lanes_on_one_device=1"]
    variants = [[], ["--host-route"], ["-t", "5", "--batch", "37", "--chunk-bytes", "600"], lanes, lanes + ["--split-output"], lanes + ["--set", "test.variants_stage_bytes=4096"]]
    if not a["anchors"]:
        variants.append(["--set", "test.wide_keys=1"])
    for extra in variants:
        out, paths, na, f, names = run(resolve_args(case["args"]) + extra, more=ALL)
        assert f["vcf"] == want, (case["args"], extra)
        assert parse_counters(out) == case["counters"], (case["args"], extra)
        assert len(paths) == case["paths_len"] and sha(paths) == case["paths_sha256"], (case["args"], extra)
        assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"], (case["args"], extra)
        if not extra:
            assert names == ["notAligned.fa", "paths", "sites.vcf"]   # a run with only --vcf: no other file, and no table on the host
    # the default thresholds
    out, paths, na, f, _ = run(resolve_args(case["args"]))
    assert f["vcf"] == V.vcf_text_of(us, V.sites_of(p, 2, 2, 200000), 2, 2, 200000) and parse_counters(out) == case["counters"], case["args"]
    # together with the other outputs: they are what they are without --vcf
    lens = A.unitig_lens(us)
    table = A.abundance_of(lens, a["k"], [len(r) for r in R], rows)
    gaf, bug = G.gaf_of(us, a["k"], H, R, rows)
    assert bug is None
    out, paths, na, f, _ = run(resolve_args(case["args"]) + ["--gaf"], flags=("vcf", "pileup", "depth", "gfa"), more=ALL)
    assert f["vcf"] == want and f["pileup"] == P.sites_text_of(us, p) and f["depth"] == P.depth_text_of(us, p), case["args"]
    assert f["gfa"] == K.gfa_text(us, a["k"], table, K.links_of(rows, len(us) - 1)) and paths == gaf.encode("latin-1"), case["args"]
    assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"] and parse_counters(out) == case["counters"], case["args"]


def test_the_goldens_have_sites():
    """the test above is about something: sites occur under both threshold sets, with several alleles and with Ns beside an allele"""
    n_all = n_default = n_multi = n_with_n = 0
    for case in CASES:
        a, us, H, R, rows = golden_rows(case)
        p = P.pileup_of(us, a["k"], R, rows)
        sites = V.sites_of(p, 1, 1, 0)
        n_all += len(sites)
        n_default += len(V.sites_of(p, 2, 2, 200000))
        n_multi += sum(1 for s in sites if sum(1 for v in s[3:7] if v) > 1)
        n_with_n += sum(1 for s in sites if s[7])
    assert n_all > 1000 and n_default > 0 and n_multi > 0, (n_all, n_default, n_multi, n_with_n)


# ---- the batch API on graphs of exactly chosen size --------------------------------------------------------------------------------------

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


def rc(s):
    """the reverse complement; N stays N"""
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def window_read(genome, x, sub=None, half=3500):
    """the genome around position x (long enough to hold a junction of any unitig of the shapes below), with `sub` at x"""
    lo, hi = max(0, x - half), min(len(genome), x + half)
    r = genome[lo:hi]
    return r if sub is None else r[:x - lo] + sub + r[x - lo + 1:]


def planted_reads(genome, three, two, seed):
    """three reads with the same substitution at every position of `three`, two at every one of `two`; then whole-genome reads on both strands,
    every second read on its reverse complement, and reads with an N -> (reads, {genome position: (letter, copies)})"""
    rnd = random.Random(seed)
    reads, planted = [], {}
    for xs, copies in ((three, 3), (two, 2)):
        for x in xs:
            sub = rnd.choice([c for c in "ACGT" if c != genome[x]])
            planted[x] = (sub, copies)
            reads += [window_read(genome, x, sub)] * copies
    reads += [genome, genome]
    for x in list(three)[:3]:   # an N beside a planted allele, and an N where nothing else differs
        reads.append(window_read(genome, x, "N"))
        reads.append(window_read(genome, min(len(genome) - 1, x + 7), "N"))
    reads = [rc(r) if i % 2 else r for i, r in enumerate(reads)]
    rnd.shuffle(reads)
    return reads, planted


def shape(name, k):
    """-> (unitig lengths, genome positions to plant three reads at, ... two reads at).  Unitig i (1-based) owns the words
    sum(len_j + 1, j < i) .. + len_i of the difference array; position p of it is genome position start_i + p"""
    if name in ("below", "exact", "plus1"):
        words = {"below": TILE - 5, "exact": TILE, "plus1": TILE + 1}[name]
        lens = [700, 900, words - 3 - 1600]
        total = sum(n - (k - 1) for n in lens) + k - 1
        return lens, [0, 699 - (k - 1) + 5, total - 1], [total - 2, 350]   # pos 0, inside, the last base of the last unitig
    assert name == "tiles"
    # unitig 1 ends on the last word of tile 0 (its extra word) and unitig 2 begins on the first word of tile 1 and spans tiles 1 .. 4;
    # unitig 4 begins on the last word of tile 4: its position 0 and its position 1 lie on the two sides of a tile edge
    long = 3 * TILE + 100
    lens = [TILE - 1, long, 5 * TILE - 1 - (TILE + long + 1) - 1, 300, 77]
    starts, at = [], 0
    for n in lens:
        starts.append(at)
        at += n - (k - 1)
    total = at + k - 1
    word0 = [sum(n + 1 for n in lens[:i]) for i in range(len(lens))]
    assert word0[1] == TILE and word0[3] == 5 * TILE - 1 and (word0[4] + lens[4] + 1) % TILE not in (0, 1)
    edge = lambda u, w: starts[u] + (w - word0[u])   # genome position of the base at word w of unitig u (0-based here)
    three = [0, starts[0] + lens[0] - 1, starts[1], starts[1] + lens[1] - 1, starts[3], starts[3] + 1, total - 1,
             edge(1, 2 * TILE - 1), edge(1, 2 * TILE), edge(1, 3 * TILE - 1), edge(1, 3 * TILE), edge(1, 4 * TILE - 1), edge(1, 4 * TILE)]
    two = [edge(1, 2 * TILE + 500), starts[2] + 40, total - 3]
    return lens, three, two


def lens_and_refs(us):
    return [len(u) for u in us], [P.codes_of(u) for u in us]


def flat_of(arr):
    return np.stack([arr[f] for f in B.PILEUP_DTYPE.names], axis=1).astype(np.int64)


def as_tuples(sites):
    return [tuple(int(v) for v in s) for s in sites]


def map_all(g, reads, m=2, effort=2):
    al = B.Aligner(g, 0)
    al.pileup_enable()
    rb, ro = pack(reads)
    rows = W.rows_of(*al.align(rb, ro, m=m, effort=effort))
    return al, rows


SHAPES = [("below", 31), ("exact", 31), ("plus1", 31), ("tiles", 15), ("tiles", 31), ("tiles", 33), ("tiles", 64)]


@pytest.mark.parametrize("name,k", SHAPES, ids=["%s-k%d" % s for s in SHAPES])
def test_batch_api_sites(name, k):
    lens, three, two = shape(name, k)
    us, genome, starts = chain(k, lens, 7 * k + len(name))
    T, n = sum(lens), len(lens)
    assert (T + n) == {"below": TILE - 5, "exact": TILE, "plus1": TILE + 1, "tiles": 5 * TILE + 378}[name]
    seqs, offs = pack(us[1:])
    g = B.Graph.build(k, seqs, offs)
    assert g.info()["total_bases"] // 2 == T and g.info()["n_unitigs"] == n
    al = B.Aligner(g, 0)
    with pytest.raises(B.BgrError, match="error -1.*never enabled"):
        al.pileup_sites(1, 1, 0)
    al.pileup_enable()
    assert len(al.pileup_sites(1, 1, 0)) == 0   # an empty table
    for prm in ((0, 1, 0), (1, 0, 0), (1, 1, 1000001)):
        with pytest.raises(B.BgrError, match="error -1.*thresholds"):
            al.pileup_sites(*prm)
    # a launch with no mismatch at all: depth everywhere, no site
    clean = [genome, rc(genome)] + [window_read(genome, x) for x in three]
    rb, ro = pack(clean)
    rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
    assert all(p for _, p in rows)
    assert len(al.pileup_sites(1, 1, 0)) == 0 and flat_of(al.pileup()[0])[:, 0].min() >= 2
    # the planted reads on top
    reads, planted = planted_reads(genome, three, two, k)
    rb, ro = pack(reads)
    rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
    assert all(p for _, p in rows) and any(p[1] < 0 for _, p in rows) and any(p[1] > 0 for _, p in rows)   # reads on both strands
    table = flat_of(al.pileup()[0])
    ulens, refs = lens_and_refs(us)
    gpos = lambda s: starts[s[0]] + s[1]
    for prm in ((1, 1, 0), (3, 3, 0), (2, 2, 200000), (1, 1, 1000000), (len(clean) + 3, 1, 0), (1, 2, 400000)):
        want = V.sites_of_rows(table, ulens, refs, *prm)
        got = as_tuples(al.pileup_sites(*prm))
        assert got == want, (name, k, prm, len(got), len(want), [x for x in got if x not in want][:3], [x for x in want if x not in got][:3])
        if prm == (1, 1, 0):   # every planted position, on every unitig it lies on (the k - 1 shared characters count on both neighbours)
            assert {gpos(s) for s in got} == set(planted)
            for s in got:
                sub, copies = planted[gpos(s)]
                assert s[3 + "ACGT".index(sub)] == copies and sum(s[3:7]) == copies
            assert any(s[7] for s in got) and len(got) > len(planted)
        if prm == (3, 3, 0):   # min_alt = 3 keeps the sites three reads planted and drops those of two
            assert {gpos(s) for s in got} == {x for x, (_, c) in planted.items() if c == 3}
    # the places the shapes are about
    got = {(s[0], s[1]) for s in as_tuples(al.pileup_sites(3, 3, 0))}
    assert (1, 0) in got and (n, lens[-1] - 1) in got
    if name == "tiles":
        assert {(2, 0), (2, lens[1] - 1), (1, lens[0] - 1), (4, 0), (4, 1)} <= got
        assert {(2, w - TILE) for e in (2, 3, 4) for w in (e * TILE - 1, e * TILE)} <= got
    # a buffer one record too small: BGR_E_CAPACITY with the number, nothing written; then with room
    L = B.lib()
    prm = B.VariantParams(1, 1, 0)
    want = V.sites_of_rows(table, ulens, refs, 1, 1, 0)
    cnt = B.C.c_uint64(0)
    out = np.zeros(len(want), dtype=B.VARIANT_DTYPE)
    assert L.bgr_aligner_pileup_sites(al.h, B.C.byref(prm), out.ctypes.data, len(want) - 1, B.C.byref(cnt)) == -4 and cnt.value == len(want)
    assert b"room for %d" % (len(want) - 1) in L.bgr_last_error() and not out["unitig"].any()
    assert L.bgr_aligner_pileup_sites(al.h, B.C.byref(prm), out.ctypes.data, len(want), B.C.byref(cnt)) == 0 and cnt.value == len(want)
    assert as_tuples(out) == want
    ms = al.pileup_sites_times()
    assert len(ms) == 5 and all(x > 0 for x in ms)


@pytest.mark.parametrize("stage", [0, 4096])
def test_add_path(stage):
    """two aligners on one graph map half the reads each; after a.pileup_add(b) the sites and the table of a are those of one aligner that
    mapped all the reads -- by one kernel, and (the test hook) in pieces through the staging buffer, the way tables cross devices"""
    k = 31
    lens, three, two = shape("tiles", k)
    us, genome, starts = chain(k, lens, 99)
    seqs, offs = pack(us[1:])
    g = B.Graph.build(k, seqs, offs)
    reads, planted = planted_reads(genome, three, two, 5)
    whole, rows = map_all(g, reads)
    h = len(reads) // 2
    a, ra = map_all(g, reads[:h])
    b, rb_ = map_all(g, reads[h:])
    assert ra + rb_ == rows and all(p for _, p in rows)
    ta, tb = flat_of(a.pileup()[0]), flat_of(b.pileup()[0])
    with B.options(**{"test.variants_stage_bytes": stage}):
        a.pileup_add(b)
    assert (flat_of(a.pileup()[0]) == ta + tb).all() and (flat_of(b.pileup()[0]) == tb).all() and ta.any() and tb.any()
    assert (ta + tb == flat_of(whole.pileup()[0])).all()
    for prm in ((1, 1, 0), (3, 3, 0), (2, 2, 200000)):
        got = as_tuples(a.pileup_sites(*prm))
        assert got == as_tuples(whole.pileup_sites(*prm)) and (len(got) > 0 or prm[2]), prm   # (three reads in some thirty: below the default fraction)
    # three reads of a planted site lie in different halves somewhere: neither half alone has the sites of (3, 3, 0)
    assert as_tuples(b.pileup_sites(3, 3, 0)) != as_tuples(whole.pileup_sites(3, 3, 0))
    for x, y in ((a, a), (a, B.Aligner(g, 0))):
        with pytest.raises(B.BgrError, match="error -1"):
            x.pileup_add(y)


def test_align_all_keeps_the_sites_in_the_graph(tmp_path):
    case = next(c for c in CASES if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    a, us, H, R, rows = golden_rows(case)
    p = P.pileup_of(us, 31, R, rows)
    g = B.Graph.from_fasta(os.path.join(GOLD, "syn_unitig.fa"), 31)
    f = os.path.join(GOLD, "syn_r150.fa")
    g.variants_enable(1, 1, 0)
    B.align_all(g, f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2, threads=2)
    assert as_tuples(g.variants()) == V.sites_of(p, 1, 1, 0) and g.variants_params() == (1, 1, 0)
    with pytest.raises(B.BgrError, match="no totals"):   # the table never reached the host
        g.pileup()
    g.write_vcf(str(tmp_path / "v"))
    assert open(tmp_path / "v", "rb").read() == V.vcf_text_of(us, V.sites_of(p, 1, 1, 0), 1, 1, 0)
    g.variants_enable(2, 2, 200000)
    B.align_all(g, f + "," + f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2, threads=2, route=1, pileup=True)   # both switches: the host totals as well
    p.add(P.pileup_of(us, 31, R, rows))
    assert as_tuples(g.variants()) == V.sites_of(p, 2, 2, 200000) and g.variants_params() == (2, 2, 200000)
    assert (flat_of(g.pileup()[0]) == p.flat()).all()
    g.variants_enable(on=False)
    B.align_all(g, f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2)   # a run without the switch leaves them
    assert as_tuples(g.variants()) == V.sites_of(p, 2, 2, 200000)
    g.variants_enable(1, 1, 0)
    with pytest.raises(B.BgrError):   # a run that fails leaves none
        B.align_all(g, str(tmp_path / "missing.fa"), str(tmp_path / "p"), str(tmp_path / "n"))
    with pytest.raises(B.BgrError, match="no totals"):
        g.variants()
    with pytest.raises(B.BgrError, match="error -1.*--vcf"):
        B.align_all(g, f, str(tmp_path / "p"), str(tmp_path / "n"), mode=B.MODE_EXHAUSTIVE)


def test_refusals(tmp_path):
    base = [B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5"]
    vcf = str(tmp_path / "x.vcf")
    def cli(graph, *more):
        return subprocess.run(base + ["-g", os.path.join(GOLD, graph)] + list(more), cwd=tmp_path, capture_output=True, text=True, timeout=300)
    pr = cli("deg_unitig.fa", "--vcf", vcf, "-b")
    assert pr.returncode == 2 and "--vcf" in pr.stderr and "-b" in pr.stderr and not os.path.exists(vcf), pr.stderr[-500:]
    pr = cli("deg_unitig_exc.fa", "--vcf", vcf)
    assert pr.returncode == 2 and "--vcf" in pr.stderr and "ACGT" in pr.stderr and not os.path.exists(vcf), pr.stderr[-500:]
    for bad in ("0.0000001", "1.5", "x", "", ".2", "20%"):
        pr = cli("deg_unitig.fa", "--vcf", vcf, "--min-af", bad)
        assert pr.returncode == 2 and "--min-af" in pr.stderr and not os.path.exists(vcf), (bad, pr.stderr[-500:])
    for flag, bad in (("--min-depth", "0"), ("--min-alt", "0"), ("--min-depth", "x"), ("--min-alt", "-1")):
        pr = cli("deg_unitig.fa", "--vcf", vcf, flag, bad)
        assert pr.returncode == 2 and flag in pr.stderr and not os.path.exists(vcf), (flag, bad, pr.stderr[-500:])
    for more in (["--min-depth", "3"], ["--min-alt", "3"], ["--min-af", "0.5"]):   # thresholds without --vcf
        pr = cli("deg_unitig.fa", *more)
        assert pr.returncode == 2 and "--vcf" in pr.stderr, (more, pr.stderr[-500:])
