"""SNV calling's definition (variants_ref.py) on hand-written pileups, the identity that lets the device scan the difference array flat, and what
of the C-ABI needs no device: the VCF writer's bytes, the --min-af parser, the refusals and the exported symbols.  The sites themselves are
checked in test_gpu_variants.py."""
import os
import random

import numpy as np
import pytest

import bgreat_amd as B
import gaf_ref as G
import pileup_ref as P
import variants_ref as V
from util import GOLD, ROOT

US = ["", "ACGTACGTAC", "GGGTTT"]


def pile(entries):
    """{(u, pos): (depth, a, c, g, t, n)} -> Pileup over US"""
    p = P.Pileup(US)
    for (u, pos), row in entries.items():
        p.depth[u][pos] = row[0]
        p.alt[u][pos] = row[1:]
    return p


def test_each_threshold_at_its_edge():
    # unitig 1 pos 1 is a C; 10 reads cover it, 3 of them read T
    p = pile({(1, 1): (10, 0, 0, 0, 3, 0)})
    site = [(1, 1, 10, 0, 0, 0, 3, 0)]
    for min_depth, want in ((9, site), (10, site), (11, [])):
        assert V.sites_of(p, min_depth, 1, 0) == want
    for min_alt, want in ((2, site), (3, site), (4, [])):
        assert V.sites_of(p, 1, min_alt, 0) == want
    # 3 / 10 = 300 000 ppm: the tie passes, one part per million more does not
    for ppm, want in ((299999, site), (300000, site), (300001, [])):
        assert V.sites_of(p, 1, 1, ppm) == want


def test_ppm_tie_needs_64_bits():
    # c * 1e6 == ppm * depth with both sides beyond 2^32: 3 000 000 of 4 000 000 000 reads is 750 ppm exactly
    p = pile({(2, 0): (4000000000, 3000000, 0, 0, 0, 0)})
    assert len(V.sites_of(p, 1, 1, 750)) == 1 and V.sites_of(p, 1, 1, 751) == []


def test_ppm_extremes():
    p = pile({(1, 0): (7, 0, 1, 0, 0, 0), (1, 2): (5, 0, 5, 0, 0, 0), (1, 4): (5, 0, 4, 0, 0, 1)})
    assert [s[:2] for s in V.sites_of(p, 1, 1, 0)] == [(1, 0), (1, 2), (1, 4)]
    assert [s[:2] for s in V.sites_of(p, 1, 1, 1000000)] == [(1, 2)]   # every covering read has the allele


def test_several_alleles_and_count_ties():
    # pos 3 of unitig 1 is a T: A and G tie at 4, C has 5 -- C first, then A before G
    p = pile({(1, 3): (20, 4, 5, 4, 0, 2), (2, 1): (9, 3, 3, 0, 3, 0)})
    assert V.passing(3, 20, (4, 5, 4, 0), 1, 1, 0) == [1, 0, 2]
    assert V.passing(3, 20, (4, 5, 4, 0), 1, 5, 0) == [1]
    assert V.passing(2, 9, (3, 3, 0, 3), 1, 1, 0) == [0, 1, 3]   # unitig 2 pos 1 is a G: three alleles, all tied
    text = V.vcf_text_of(US, V.sites_of(p, 1, 1, 0), 1, 1, 0).decode()
    assert "1\t4\t.\tT\tC,A,G\t.\tPASS\tDP=20;AD=5,5,4,4;NN=2\n" in text
    assert "2\t2\t.\tG\tA,C,T\t.\tPASS\tDP=9;AD=0,3,3,3;NN=0\n" in text
    assert text.index("##contig=<ID=1,length=10>") < text.index("##contig=<ID=2,length=6>") < text.index("#CHROM")


def test_n_is_never_an_allele():
    p = pile({(1, 5): (8, 0, 0, 0, 0, 8), (1, 6): (8, 0, 0, 0, 1, 7)})
    assert V.sites_of(p, 1, 1, 0) == [(1, 6, 8, 0, 0, 0, 1, 7)]


def test_the_unitigs_own_letter_is_no_allele():
    # a count on the base's own letter cannot come from the kernel; the definition ignores it all the same
    assert V.passing(0, 10, (9, 0, 0, 0), 1, 1, 0) == []


def random_pileup(rnd, n_unitigs, max_len):
    us = [""] + ["".join(rnd.choice("ACGT") for _ in range(rnd.randint(1, max_len))) for _ in range(n_unitigs)]
    p = P.Pileup(us)
    for u in range(1, len(us)):
        L = len(us[u])
        for _ in range(rnd.randint(0, 6)):   # covered stretches, as reads leave them
            a = rnd.randrange(L)
            b = rnd.randint(a + 1, L)
            p.depth[u][a:b] += rnd.choice([1, 1, 2, 0xFFFFFFF0])   # (sums beyond 2^32 too: the device counts mod 2^32)
        p.depth[u] %= 1 << 32
        for pos in range(L):
            if p.depth[u][pos] and rnd.random() < 0.3:
                c = rnd.randrange(5)
                if c != p.ref[u][pos]:
                    p.alt[u][pos][c] = rnd.randint(1, 5)
    return us, p


@pytest.mark.parametrize("seed", range(6))
def test_flat_scan_identity(seed):
    """every unitig's len + 1 difference words sum to 0 mod 2^32, so ONE running sum over all T + n words equals the per-unitig depths -- what
    the device's passes rely on (variants_kernels.h) and what bgr_aligner_pileup computes unitig by unitig on the host"""
    rnd = random.Random(seed)
    us, p = random_pileup(rnd, rnd.randint(1, 40), rnd.choice([3, 40, 700]))
    alt, delta, base_offs = V.table_words(p)
    n = len(us) - 1
    assert len(delta) == int(base_offs[n + 1]) + n and len(alt) == 4 * int(base_offs[n + 1])
    flat = np.cumsum(delta.astype(np.uint64)) % (1 << 32)
    for u in range(1, n + 1):
        d0 = int(base_offs[u]) + u - 1
        assert int(delta[d0:d0 + len(us[u]) + 1].astype(np.uint64).sum()) % (1 << 32) == 0
        assert (flat[d0:d0 + len(us[u])] == p.depth[u].astype(np.uint64)).all(), u
        assert flat[d0 + len(us[u])] == 0   # the extra word: back to 0
        # and the layout of the alt words: N lies in the word of the base's own letter
        for pos in range(len(us[u])):
            w = alt[4 * (int(base_offs[u]) + pos):][:4]
            ref = int(p.ref[u][pos])
            assert int(w[ref]) == int(p.alt[u][pos][4]) and all(int(w[c]) == int(p.alt[u][pos][c]) for c in range(4) if c != ref)


def golden_graph():
    us = G.load_unitigs(os.path.join(GOLD, "syn_unitig.fa"), 31)
    return us, B.Graph.from_fasta(os.path.join(GOLD, "syn_unitig.fa"), 31)


def sites_array(sites):
    return np.array(sites, dtype=B.VARIANT_DTYPE)


def hand_made_sites(us):
    """on the golden graph: first and last base of unitigs, several alleles, ties, Ns; every record passes 2 / 2 / 200 000"""
    other = lambda ch, i=0: [x for x in "ACGT" if x != ch][i]
    def rec(u, pos, depth, n=0, **alts):   # alts by LETTER position among the three non-reference letters: x0, x1, x2
        counts = [0, 0, 0, 0]
        for key, v in alts.items():
            counts["ACGT".index(other(us[u][pos], int(key[1])))] = v
        return (u, pos, depth) + tuple(counts) + (n,)
    last = len(us) - 1
    return [rec(1, 0, 10, x0=2), rec(1, len(us[1]) - 1, 10, x1=5, x2=5, n=0), rec(2, 3, 4000000000, x0=3000000000, n=7), rec(7, 5, 9, x0=3, x1=3, x2=3),
            rec(7, 6, 12, x2=4, x0=6, n=2), rec(last, len(us[last]) - 1, 2, x1=2)]


def test_write_vcf_bytes(tmp_path):
    us, g = golden_graph()
    sites = hand_made_sites(us)
    path = str(tmp_path / "x.vcf")
    g.write_vcf(path, sites_array(sites), (2, 2, 200000))
    got = open(path, "rb").read()
    assert got == V.vcf_text_of(us, sites, 2, 2, 200000)
    assert got.count(b"##contig=") == 4 and got.startswith(b"##fileformat=VCFv4.2\n##source=bgreat-mi355x\n##bgreat_thresholds=<min_depth=2,min_alt=2,min_af_ppm=200000>\n")
    g.write_vcf(path, sites_array([]), (1, 1, 0))   # no sites: the header alone
    assert open(path, "rb").read() == V.vcf_text_of(us, [], 1, 1, 0)
    # under stricter thresholds fewer alleles pass: ALT and AD follow
    fewer = [sites[1], sites[2], sites[4]]
    g.write_vcf(path, sites_array(fewer), (2, 5, 0))
    assert open(path, "rb").read() == V.vcf_text_of(us, fewer, 2, 5, 0) and len(open(path, "rb").read().split(b"#CHROM")[1].split(b"\n")[3].split(b"\t")[4]) == 1


def test_write_vcf_refuses_what_is_no_site(tmp_path):
    us, g = golden_graph()
    sites = hand_made_sites(us)
    path = str(tmp_path / "x.vcf")
    for bad, word in ((sites[::-1], "order"), ([sites[0], sites[0]], "order"), ([(len(us), 0, 5, 0, 0, 0, 0, 0)], "outside"), ([(1, len(us[1]), 5, 0, 0, 0, 0, 0)], "outside"),
                      ([(0, 0, 5, 0, 0, 0, 0, 0)], "outside"), ([(1, 0, 10, 0, 0, 0, 0, 10)], "no passing allele")):
        with pytest.raises(B.BgrError, match="error -1.*" + word):
            g.write_vcf(path, sites_array(bad), (2, 2, 200000))
        assert not os.path.exists(path)
    with pytest.raises(B.BgrError, match="error -1.*no passing allele"):   # sites[0] has 2 of 10: 200 000 ppm exactly
        g.write_vcf(path, sites_array(sites[:1]), (2, 2, 200001))
    for prm in ((0, 1, 0), (1, 0, 0), (1, 1, 1000001)):
        with pytest.raises(B.BgrError, match="error -1.*thresholds"):
            g.write_vcf(path, sites_array(sites), prm)
    with pytest.raises(B.BgrError, match="error -3"):
        g.write_vcf(str(tmp_path / "no" / "dir" / "x.vcf"), sites_array(sites), (2, 2, 200000))


def test_min_af_parser():
    for text, ppm in (("0", 0), ("1", 1000000), ("0.2", 200000), ("0.000001", 1), ("1.0", 1000000), ("1.000000", 1000000), ("0.5", 500000), ("0.123456", 123456),
                      ("00.25", 250000), ("0.999999", 999999)):
        assert B.parse_af_ppm(text) == ppm, text
    for text in ("", ".", ".5", "0.", "1.1", "2", "1.000001", "0.0000001", "0.2x", " 0.2", "0.2 ", "-0.2", "+0.2", "1e-3", "0,2", "0x1", "nan", "10"):
        with pytest.raises(B.BgrError, match="error -1"):
            B.parse_af_ppm(text)


def test_refusals_without_a_device():
    L = B.lib()
    ge = B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig_exc.fa"), 5)
    with pytest.raises(B.BgrError, match="error -1.*ACGT"):
        ge.variants_enable()
    assert not ge.variants_enabled()
    g = B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig.fa"), 5)
    assert not g.variants_enabled()
    for prm in ((0, 1, 0), (1, 0, 0), (1, 1, 1000001)):
        with pytest.raises(B.BgrError, match="error -1.*thresholds"):
            g.variants_enable(*prm)
        assert not g.variants_enabled()
    g.variants_enable(1, 1, 0)
    assert g.variants_enabled() and not g.pileup_enabled()
    g.variants_enable(on=False)
    assert not g.variants_enabled()
    for call in (g.variants, g.variants_params, lambda: g.write_vcf("x")):
        with pytest.raises(B.BgrError, match="error -1.*no totals"):
            call()
    n = B.C.c_uint64(5)
    prm = B.VariantParams(1, 1, 0)
    assert L.bgr_graph_variants_enable(None, B.C.byref(prm)) == -1 and L.bgr_graph_variants_enabled(None) == 0
    assert L.bgr_graph_variants(None, None, 0, B.C.byref(n)) == -1 and n.value == 0 and L.bgr_graph_variants(g.h, None, 0, None) == -1
    assert L.bgr_graph_variants_params(None, B.C.byref(prm)) == -1 and L.bgr_graph_variants_params(g.h, None) == -1
    assert L.bgr_write_vcf(None, g.h, B.C.byref(prm), None, 0) == -1 and L.bgr_write_vcf(b"x", None, B.C.byref(prm), None, 0) == -1
    assert L.bgr_write_vcf(b"x", g.h, None, None, 0) == -1 and L.bgr_write_vcf(b"x", g.h, B.C.byref(prm), None, 1) == -1 and not os.path.exists("x")
    n.value = 5
    assert L.bgr_aligner_pileup_sites(None, B.C.byref(prm), None, 0, B.C.byref(n)) == -1 and n.value == 0
    assert L.bgr_aligner_pileup_sites_times(None, None) == -1 and L.bgr_aligner_pileup_add(None, None) == -1
    assert L.bgr_parse_af_ppm(None, None) == -1 and L.bgr_parse_af_ppm(b"0.2", None) == -1


def test_symbols_and_struct():
    L = B.lib()
    for name in ("bgr_aligner_pileup_sites", "bgr_aligner_pileup_sites_times", "bgr_aligner_pileup_add", "bgr_graph_variants_enable", "bgr_graph_variants_enabled",
                 "bgr_graph_variants", "bgr_graph_variants_params", "bgr_write_vcf", "bgr_parse_af_ppm"):
        assert hasattr(L, name) and name in B.SYMBOLS, name
    assert B.VARIANT_DTYPE.itemsize == 32 and B.VARIANT_DTYPE.names == ("unitig", "pos", "depth", "a", "c", "g", "t", "n")
    assert B.C.sizeof(B.VariantParams) == 12
    header = open(os.path.join(ROOT, "include", "bgreat_gpu.h")).read()
    assert "#define BGR_VARIANTS_TILE %du" % B.VARIANTS_TILE in header
    assert "test.variants_stage_bytes" in dict(B.option_names())
