"""The per-strand pileup's definition (strands_ref.py) against pileup_ref.py / variants_ref.py on hand-checked rows and over the goldens' oracle
rows, and what of the C-ABI needs no device: the VCF writer's bytes, the refusals and the exported symbols.  The forward table itself, the sites
and bgr_write_pileup_strands' bytes (the graph's totals are set by a run) are checked in test_gpu_strands.py."""
import os

import numpy as np
import pytest

import abundance_ref as A
import bgreat_amd as B
import gaf_ref as G
import pileup_ref as P
import strands_ref as S
import variants_ref as V
from test_gaf_host import _oracle, gaf_cases, golden_rows
from test_wide_k_host import pack
from util import GOLD, ROOT
from wide_greedy_ref import ST_RC

K = 4
US = ["", "AACCGT", "CGTTAG", "ACGACG"]   # test_pileup_host.py's: 1 and 2 share CGT, the walk of [+1, +2] is AACCGTTAG


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def case_of(reads, graph):
    return next(c for c in gaf_cases() if c["args"][:6] == ["-r", reads, "-k", c["args"][3], "-g", graph] and "-G" not in c["args"] and "-m" in c["args"]
                and c["args"][c["args"].index("-m") + 1] == "2" and c["args"][c["args"].index("-e") + 1] == "2")


def flat_sum(p):
    return int(p.flat()[:, 0].sum()), int(p.flat()[:, 1:5].sum())


def test_the_four_combinations_by_hand():
    one = lambda read, st, path: S.forward_of(US, K, [read], [(st, path)])
    tot = lambda read, st, path: P.pileup_of(US, K, [read], [(st, path)])
    # the read as given runs along both unitigs' file strand: everything is forward
    f, p = one("ACCTTTA", 0, [1, 1, 2]), tot("ACCTTTA", 0, [1, 1, 2])
    assert (f.flat() == p.flat()).all() and p.flat().any()
    # the same placement from the reverse complement: nothing is forward
    f = one("TAAAGGT", ST_RC, [1, 1, 2])
    assert not f.flat().any() and (tot("TAAAGGT", ST_RC, [1, 1, 2]).flat() == p.flat()).all()
    # unitig 2 backwards, the read as given: reverse; the same walk from the read's reverse complement: forward
    assert not one("CGAAC", 0, [0, -2]).flat().any()
    f = one(rc("CGAAC"), ST_RC, [0, -2])
    assert (f.flat() == tot("CGAAC", 0, [0, -2]).flat()).all() and int(f.alt[2][4][1]) == 1
    # a unitig glued on in the strand its sign does not name: the walk's orientation decides, not the sign
    assert (one("ACCTTTA", 0, [1, 1, -2]).flat() == tot("ACCTTTA", 0, [1, 1, -2]).flat()).all()
    # no walk: neither table, and skipped is the total's alone
    f, p = one("CGTT", 0, [0, 2, 1]), tot("CGTT", 0, [0, 2, 1])
    assert not f.flat().any() and f.skipped == 0 and p.skipped == 1


GOLDENS = [("deg_reads.fa", "deg_unitig.fa", 5), ("syn_r150.fa", "syn_unitig.fa", 31)]


@pytest.mark.parametrize("reads,graph,k", GOLDENS)
def test_forward_against_total_over_the_goldens(reads, graph, k):
    a, us, H, R, rows = golden_rows(case_of(reads, graph))
    combos = {}
    p, f = P.pileup_of(us, k, R, rows), S.forward_of(us, k, R, rows, combos)
    assert all(combos.get((x, y), 0) > 0 for x in (False, True) for y in (False, True)), combos
    assert f.skipped == 0
    for u in range(1, len(us)):
        assert (f.depth[u] >= 0).all() and (f.depth[u] <= p.depth[u]).all() and (f.alt[u] >= 0).all() and (f.alt[u] <= p.alt[u]).all(), u
    assert [int(d.sum()) for d in f.depth] == S.forward_bases(us, k, R, rows)
    fd, fa = flat_sum(f)
    td, ta = flat_sum(p)
    assert 0 < fd < td and 0 < fa < ta
    if graph == "deg_unitig.fa":   # the figures the definition was checked with
        assert (combos[(False, True)], combos[(False, False)], combos[(True, True)], combos[(True, False)]) == (82, 67, 39, 30) and (fd, td) == (689, 1346)
        assert int(f.flat()[:, 1:].sum()) == 123 and int(p.flat()[:, 1:].sum()) == 259
        n = [len(S.sites_of(p, f, 2, 2, 200000, s)) for s in (0, 1, 2)]
        assert n == [10, 4, 0] and 0 < n[1] < n[0] and n[2] == 0
    else:
        assert (combos[(False, True)], combos[(False, False)], combos[(True, True)], combos[(True, False)]) == (561, 520, 75, 79) and (fd, td) == (37679, 71970)
    # min_alt_strand = 0 is today's site set exactly
    for prm in ((1, 1, 0), (2, 2, 200000), (3, 1, 500000)):
        assert [s[:8] for s in S.sites_of(p, f, *prm, 0)] == V.sites_of(p, *prm)
        s1 = S.sites_of(p, f, *prm, 1)
        assert set(s1) <= set(S.sites_of(p, f, *prm, 0))


@pytest.mark.parametrize("reads,graph,k", GOLDENS)
def test_a_read_and_its_reverse_complement_split_the_total(reads, graph, k):
    """the reverse complement of a read maps on the other strand, by status or by path: where the oracle maps both on the same stretch of the same
    unitigs, forward(read) + forward(rc(read)) = total(read) -- every observation is forward in exactly one of the two"""
    a, us, H, R, rows = golden_rows(case_of(reads, graph))
    R2 = [rc(r) for r in R]
    rb, ro = pack(R2)
    p2, po2, st2 = _oracle(a["graph"], k, False).align(rb, ro, m=a["m"], effort=a["e"], mode=0)
    rows2 = [(int(st2[i]), [int(x) for x in p2[int(po2[i]):int(po2[i + 1])]]) for i in range(len(R2))]
    both = same = 0
    for r, r2, row, row2 in zip(R, R2, rows, rows2):
        if not row[1] or not row2[1]:
            continue
        both += 1
        t, t2 = P.pileup_of(us, k, [r], [row]), P.pileup_of(us, k, [r2], [row2])
        if t.skipped or t2.skipped or not (t.flat() == t2.flat()).all():
            continue   # (the oracle placed the reverse complement elsewhere: another stretch, nothing to compare)
        same += 1
        fw = S.forward_of(us, k, [r], [row]).add(S.forward_of(us, k, [r2], [row2]))
        assert (fw.flat() == t.flat()).all(), (row, row2)
    assert both > 100 and same >= 20, (both, same)   # (on the degenerate graph the oracle places many a reverse complement on another of its repeats)


def golden_graph():
    us = G.load_unitigs(os.path.join(GOLD, "syn_unitig.fa"), 31)
    return us, B.Graph.from_fasta(os.path.join(GOLD, "syn_unitig.fa"), 31)


def sites_array(sites):
    return np.array([tuple(s) + (0, 0) for s in sites], dtype=B.VARIANT_STRAND_DTYPE)


def hand_made_sites(us):
    """on the golden graph: first and last base of unitigs, two ALTs, fn > 0, alleles on one strand only; every record passes 2 / 2 / 200 000 / 0"""
    other = lambda ch, i=0: [x for x in "ACGT" if x != ch][i]
    def rec(u, pos, depth, fdepth, n=(0, 0), **alts):   # alts by position among the three non-reference letters: x0 = (total, forward)
        counts, fcounts = [0, 0, 0, 0], [0, 0, 0, 0]
        for key, (v, fv) in alts.items():
            i = "ACGT".index(other(us[u][pos], int(key[1])))
            counts[i], fcounts[i] = v, fv
        return (u, pos, depth) + tuple(counts) + (n[0], fdepth) + tuple(fcounts) + (n[1],)
    last = len(us) - 1
    return [rec(1, 0, 10, 4, x0=(2, 1)), rec(1, len(us[1]) - 1, 12, 7, x1=(5, 3), x2=(5, 2)), rec(2, 3, 4000000000, 3999999999, n=(7, 7), x0=(3000000000, 2999999999)),
            rec(7, 5, 9, 4, x0=(3, 3), x1=(3, 0), x2=(3, 1)), rec(7, 6, 12, 6, n=(2, 1), x2=(4, 2), x0=(6, 3)), rec(last, len(us[last]) - 1, 2, 0, x1=(2, 0))]


def test_write_vcf_strands_bytes(tmp_path):
    us, g = golden_graph()
    sites = hand_made_sites(us)
    path = str(tmp_path / "x.vcf")
    g.write_vcf_strands(path, sites_array(sites), (2, 2, 200000, 0))
    got = open(path, "rb").read()
    assert got == S.vcf_text_of(us, sites, 2, 2, 200000, 0)
    assert got.startswith(b"##fileformat=VCFv4.2\n##source=bgreat-mi355x\n##bgreat_thresholds=<min_depth=2,min_alt=2,min_af_ppm=200000,min_alt_strand=0>\n")
    assert got.index(b"##INFO=<ID=AD,") < got.index(b"##INFO=<ID=ADF,") < got.index(b"##INFO=<ID=ADR,") < got.index(b"##INFO=<ID=NN,")
    text = got.decode()
    assert "DP=12;AD=2,5,5;ADF=2,3,2;ADR=0,2,3;NN=0\n" in text          # two ALTs
    assert "DP=12;AD=0,6,4;ADF=0,3,2;ADR=0,3,2;NN=2\n" in text          # fn > 0: forward ref = 6 - (3 + 2 + 1)
    assert "DP=4000000000;AD=999999993,3000000000;ADF=999999993,2999999999;ADR=0,1;NN=7\n" in text
    # min_alt_strand 1: the alleles seen on one strand only leave ALT, AD, ADF and ADR; sites without any other are no sites any more
    fewer = [s for s in sites if S.passing("ACGT".index(us[s[0]][s[1]]), s[2], s[3:7], s[9:13], 2, 2, 200000, 1)]
    assert len(fewer) == 5 and sites[-1] not in fewer
    g.write_vcf_strands(path, sites_array(fewer), (2, 2, 200000, 1))
    got = open(path, "rb").read()
    assert got == S.vcf_text_of(us, fewer, 2, 2, 200000, 1) and b"min_alt_strand=1>" in got
    assert b"DP=9;AD=0,3;ADF=0,1;ADR=0,2;NN=0\n" in got   # of three tied alleles the one read on both strands
    g.write_vcf_strands(path, sites_array([]), (1, 1, 0, 3))   # no sites: the header alone
    assert open(path, "rb").read() == S.vcf_text_of(us, [], 1, 1, 0, 3)


def test_write_vcf_strands_refuses_what_is_no_site(tmp_path):
    us, g = golden_graph()
    sites = hand_made_sites(us)
    path = str(tmp_path / "x.vcf")
    z = (0, 0, 0, 0, 0, 0)
    for bad, word in ((sites[::-1], "order"), ([(len(us), 0, 5, 0, 0, 0, 0, 0) + z], "outside"), ([(1, 0, 10, 0, 0, 0, 0, 10) + z], "no passing allele"),
                      ([sites[0][:8] + (11,) + sites[0][9:]], "do not fit"), ([sites[0][:9] + (3, 3, 3, 3, 0)], "do not fit"), ([sites[4][:13] + (3,)], "do not fit")):
        with pytest.raises(B.BgrError, match="error -1.*" + word):
            g.write_vcf_strands(path, sites_array(bad), (2, 2, 200000, 0))
        assert not os.path.exists(path)
    with pytest.raises(B.BgrError, match="error -1.*no passing allele"):   # the last record's allele is never read forward
        g.write_vcf_strands(path, sites_array(sites[-1:]), (2, 2, 200000, 1))
    for prm in ((0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 1000001, 0)):
        with pytest.raises(B.BgrError, match="error -1.*thresholds"):
            g.write_vcf_strands(path, sites_array(sites), prm)
    with pytest.raises(B.BgrError, match="error -3"):
        g.write_vcf_strands(str(tmp_path / "no" / "dir" / "x.vcf"), sites_array(sites), (2, 2, 200000, 0))


def test_pileup_strands_text_by_hand():
    rows = [("ACCTTTA", 0, [1, 1, 2]), ("TAAAGGT", ST_RC, [1, 1, 2]), ("ACCGT", 0, [1, 1])]
    R, rw = [r for r, _, _ in rows], [(st, p) for _, st, p in rows]
    text = S.sites_text_of(US, P.pileup_of(US, K, R, rw), S.forward_of(US, K, R, rw)).decode().split("\n")
    assert text[0] == "#unitig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tdepth+\tA+\tC+\tG+\tT+\tN+"
    assert "1\t4\tG\t3\t0\t0\t0\t2\t0\t2\t0\t0\t0\t1\t0" in text and "2\t1\tG\t2\t0\t0\t0\t2\t0\t1\t0\t0\t0\t1\t0" in text


def test_refusals_without_a_device(tmp_path):
    L = B.lib()
    ge = B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig_exc.fa"), 5)
    with pytest.raises(B.BgrError, match="error -1.*ACGT"):
        ge.pileup_strands_enable()
    with pytest.raises(B.BgrError, match="error -1.*ACGT"):
        ge.variants_strands_enable()
    assert not ge.pileup_strands_enabled() and not ge.pileup_enabled() and not ge.variants_enabled()
    g = B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig.fa"), 5)
    assert not g.pileup_strands_enabled()
    g.pileup_strands_enable()
    assert g.pileup_strands_enabled() and g.pileup_enabled()   # (as the aligner's switch enables the aligner's pileup)
    g.pileup_strands_enable(False)
    assert not g.pileup_strands_enabled() and g.pileup_enabled()
    for prm in ((0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 1000001, 0)):
        with pytest.raises(B.BgrError, match="error -1.*thresholds"):
            g.variants_strands_enable(*prm)
        assert not g.variants_enabled()
    g.variants_strands_enable(1, 1, 0, 2)
    assert g.variants_enabled()
    g.variants_strands_enable(on=False)
    assert not g.variants_enabled()
    for call in (g.pileup_forward, g.variant_strand_sites, lambda: g.write_pileup_strands(str(tmp_path / "x"))):
        with pytest.raises(B.BgrError, match="error -1.*no (forward )?totals"):
            call()
    assert not os.path.exists(tmp_path / "x")
    n = B.C.c_uint64(5)
    prm = B.VariantStrandParams(1, 1, 0, 0)
    assert L.bgr_graph_pileup_strands_enable(None, 1) == -1 and L.bgr_graph_pileup_strands_enabled(None) == 0 and L.bgr_graph_pileup_forward(None, None, 0) == -1
    assert L.bgr_graph_variants_strands_enable(None, B.C.byref(prm)) == -1
    assert L.bgr_graph_variant_strand_sites(None, None, 0, B.C.byref(n)) == -1 and n.value == 0 and L.bgr_graph_variant_strand_sites(g.h, None, 0, None) == -1
    assert L.bgr_write_pileup_strands(None, g.h) == -1 and L.bgr_write_pileup_strands(b"x", None) == -1
    assert L.bgr_write_vcf_strands(None, g.h, B.C.byref(prm), None, 0) == -1 and L.bgr_write_vcf_strands(b"x", None, B.C.byref(prm), None, 0) == -1
    assert L.bgr_write_vcf_strands(b"x", g.h, None, None, 0) == -1 and L.bgr_write_vcf_strands(b"x", g.h, B.C.byref(prm), None, 1) == -1 and not os.path.exists("x")
    n.value = 5
    assert L.bgr_aligner_pileup_strand_sites(None, B.C.byref(prm), None, 0, B.C.byref(n)) == -1 and n.value == 0
    assert L.bgr_aligner_pileup_strands_enable(None, 1) == -1 and L.bgr_aligner_pileup_forward(None, None, 0) == -1


def test_symbols_and_structs():
    L = B.lib()
    for name in ("bgr_aligner_pileup_strands_enable", "bgr_aligner_pileup_forward", "bgr_aligner_pileup_strand_sites", "bgr_graph_pileup_strands_enable",
                 "bgr_graph_pileup_strands_enabled", "bgr_graph_pileup_forward", "bgr_graph_variants_strands_enable", "bgr_graph_variant_strand_sites",
                 "bgr_write_pileup_strands", "bgr_write_vcf_strands"):
        assert hasattr(L, name) and name in B.SYMBOLS, name
    assert B.VARIANT_STRAND_DTYPE.itemsize == 64 and B.VARIANT_STRAND_DTYPE.names[:14] == ("unitig", "pos", "depth", "a", "c", "g", "t", "n", "fdepth", "fa", "fc", "fg", "ft", "fn")
    assert B.C.sizeof(B.VariantStrandParams) == 16
    header = open(os.path.join(ROOT, "include", "bgreat_gpu.h")).read()
    for name in ("bgr_variant_strand_params", "bgr_variant_strand_site", "bgr_write_vcf_strands"):
        assert name in header
