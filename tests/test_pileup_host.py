"""The pileup's definition (pileup_ref.py) on hand-checked rows and over the goldens' oracle rows, and what of the C-ABI needs no device: the
refusals and the exported symbols.  The writers' bytes are checked in test_gpu_pileup.py: the graph's totals are set by a run, and a run needs
a device.

Flipped orientation -- a unitig glued on in the strand its sign does not name (compactionEnd's second try) -- occurs in none of the goldens' rows
and no ACGT-only input is known to produce it: the kernel takes the strand from the walk's state, as gaf_stat does, and the definition is
tested for it here, on the CPU, only."""
import os

import pytest

import abundance_ref as A
import bgreat_amd as B
import gaf_ref as G
import pileup_ref as P
from test_gaf_host import gaf_cases, golden_rows
from util import GOLD
from wide_greedy_ref import ST_RC

K = 4
US = ["", "AACCGT", "CGTTAG", "ACGACG"]   # 1 and 2 share CGT: the walk of [+1, +2] is AACCGTTAG; 3 glues on itself


def table(rows):
    """[(read, status, path)] -> Pileup"""
    return P.pileup_of(US, K, [r for r, _, _ in rows], [(st, p) for _, st, p in rows])


def nonzero_alt(p):
    return {(u, pos, P.LETTERS[c]): int(p.alt[u][pos][c]) for u in range(1, len(US)) for pos in range(len(US[u])) for c in range(5) if p.alt[u][pos][c]}


def test_mismatch_inside_the_overlap_counts_on_both_unitigs():
    # walk AACCGTTAG, extents [0, 6) and [3, 9); the read covers [1, 8) and has T for the G at walk position 4: position 4 of unitig 1, 1 of unitig 2
    p = table([("ACCTTTA", 0, [1, 1, 2])])
    assert p.depth[1].tolist() == [0, 1, 1, 1, 1, 1] and p.depth[2].tolist() == [1, 1, 1, 1, 1, 0]
    assert nonzero_alt(p) == {(1, 4, "T"): 1, (2, 1, "T"): 1} and p.skipped == 0


def test_read_on_its_reverse_complement():
    # TAAAGGT is the reverse complement of ACCTTTA: the same counts
    p = table([("TAAAGGT", ST_RC, [1, 1, 2])])
    assert p.depth[1].tolist() == [0, 1, 1, 1, 1, 1] and p.depth[2].tolist() == [1, 1, 1, 1, 1, 0]
    assert nonzero_alt(p) == {(1, 4, "T"): 1, (2, 1, "T"): 1}


def test_negative_id():
    # the walk is CTAACG, unitig 2 backwards; the read CGAAC has G at x = 1, which is position 6 - 1 - 1 = 4 (an A) of the unitig, read as the complement C
    p = table([("CGAAC", 0, [0, -2])])
    assert p.depth[2].tolist() == [0, 1, 1, 1, 1, 1] and not p.depth[1].any()
    assert nonzero_alt(p) == {(2, 4, "C"): 1}


def test_unitig_glued_on_the_strand_its_sign_does_not_name():
    # -2 spells CTAACG, which does not continue AACCGT; its reverse complement does: the unitig lies forward in the walk whatever its sign says
    assert G.walk_of(US, K, [1, 1, -2]) == ("AACCGTTAG", [True, True])
    p = table([("ACCTTTA", 0, [1, 1, -2])])
    assert p.depth[2].tolist() == [1, 1, 1, 1, 1, 0] and nonzero_alt(p) == {(1, 4, "T"): 1, (2, 1, "T"): 1}


def test_n_and_other_characters():
    # walk position 3 (C) lies on both unitigs; N stays N on a reversed unitig and on a reverse-complemented read; a lower-case letter is an N
    assert nonzero_alt(table([("ACNGTTA", 0, [1, 1, 2])])) == {(1, 3, "N"): 1, (2, 0, "N"): 1}
    assert nonzero_alt(table([("TAACNGT", ST_RC, [1, 1, 2])])) == {(1, 3, "N"): 1, (2, 0, "N"): 1}
    assert nonzero_alt(table([("CNAAC", 0, [0, -2])])) == {(2, 4, "N"): 1}
    assert nonzero_alt(table([("ACcGTTA", 0, [1, 1, 2])])) == {(1, 3, "N"): 1, (2, 0, "N"): 1}


def test_unitig_twice_in_one_path():
    # walk ACGACGACG, extents [0, 6) and [3, 9); T for the C at walk position 4: position 4 of the first occurrence, 1 of the second
    p = table([("ACGATGACG", 0, [0, 3, 3])])
    assert p.depth[3].tolist() == [2, 2, 2, 2, 2, 2] and nonzero_alt(p) == {(3, 4, "T"): 1, (3, 1, "T"): 1}


def test_unmapped_overhang_and_no_walk():
    p = table([("ACCGTTA", 0, []), ("TAGGG", 0, [6, 1, 2]), ("CGTT", 0, [0, 2, 1]), ("ACCG", 0, [0, 1, 9]), ("ACCG", 0, [10, 1, 2])])
    # the second read overhangs the walk's end: cl = 3, on unitig 2 only; the last three spell no walk
    assert p.depth[2].tolist() == [0, 0, 0, 1, 1, 1] and not p.depth[1].any() and not nonzero_alt(p) and p.skipped == 3


def test_texts():
    p = table([("ACCTTTA", 0, [1, 1, 2]), ("ACCGT", 0, [1, 1])])
    assert P.sites_text_of(US, p) == (b"#unitig\tpos\tref\tdepth\tA\tC\tG\tT\tN\n1\t1\tA\t2\t0\t0\t0\t0\t0\n1\t2\tC\t2\t0\t0\t0\t0\t0\n1\t3\tC\t2\t0\t0\t0\t0\t0\n"
                                      b"1\t4\tG\t2\t0\t0\t0\t1\t0\n1\t5\tT\t2\t0\t0\t0\t0\t0\n2\t0\tC\t1\t0\t0\t0\t0\t0\n2\t1\tG\t1\t0\t0\t0\t1\t0\n"
                                      b"2\t2\tT\t1\t0\t0\t0\t0\t0\n2\t3\tT\t1\t0\t0\t0\t0\t0\n2\t4\tA\t1\t0\t0\t0\t0\t0\n")
    assert P.depth_text_of(US, p) == b"1\t1\t6\t2\n2\t0\t5\t1\n"
    assert p.flat().shape == (18, 6) and p.flat()[4].tolist() == [2, 0, 0, 0, 1, 0]


def test_over_the_goldens():
    """sum(depth[u]) == abundance_ref's bases[u]; a read on one unitig adds as many alts as gaf_ref counts mismatches; every class of rows the
    GPU tests rely on occurs"""
    n_mapped = n_nm = n_rc = n_n = n_twice = 0
    for case in gaf_cases():
        a, us, H, R, rows = golden_rows(case)
        k, lens = a["k"], A.unitig_lens(us)
        p = P.Pileup(us)
        for r, (st, path) in zip(R, rows):
            if not path:
                continue
            adds = P.add_read(p, us, k, r, st, path)
            s = G.stats(us, k, r, st, path)
            assert s is not G.NO_WALK
            if len(path) == 2:
                assert adds == s["nm"], (case["args"], path)
            else:
                assert adds >= s["nm"]
            ids = [abs(x) for x in path[1:]]
            n_mapped += 1
            n_nm += s["nm"] > 0
            n_rc += bool(st & ST_RC)
            n_n += "N" in r
            n_twice += len(set(ids)) < len(ids)
        ab = A.abundance_of(lens, k, [len(r) for r in R], rows)
        assert p.skipped == 0 and [int(d.sum()) for d in p.depth] == [t[1] for t in ab], case["args"]
    assert n_mapped > 7000 and n_nm > 0 and n_rc > 0 and n_n > 0 and n_twice > 0, (n_mapped, n_nm, n_rc, n_n, n_twice)


def test_refusals_without_a_device(tmp_path):
    L = B.lib()
    ge = B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig_exc.fa"), 5)
    with pytest.raises(B.BgrError, match="error -1.*--pileup.*ACGT"):
        ge.pileup_enable()
    assert not ge.pileup_enabled()
    g = B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig.fa"), 5)
    assert not g.pileup_enabled()
    g.pileup_enable()
    assert g.pileup_enabled()
    g.pileup_enable(False)
    assert not g.pileup_enabled()
    with pytest.raises(B.BgrError, match="error -1.*no totals"):
        g.pileup()
    for write in (g.write_pileup, g.write_depth):
        with pytest.raises(B.BgrError, match="error -1.*no totals"):
            write(str(tmp_path / "x"))
        assert not os.path.exists(tmp_path / "x")
    assert L.bgr_graph_pileup_enable(None, 1) == -1 and L.bgr_graph_pileup_enabled(None) == 0
    assert L.bgr_graph_pileup(None, None, 0, None) == -1 and L.bgr_write_pileup(None, g.h) == -1 and L.bgr_write_depth(b"x", None) == -1
    assert L.bgr_aligner_pileup_enable(None, 1) == -1 and L.bgr_aligner_pileup(None, None, 0, None) == -1 and L.bgr_aligner_reset_pileup(None) == -1


def test_symbols_and_struct():
    L = B.lib()
    for name in ("bgr_aligner_pileup_enable", "bgr_aligner_pileup", "bgr_aligner_reset_pileup", "bgr_graph_pileup_enable", "bgr_graph_pileup_enabled",
                 "bgr_graph_pileup", "bgr_write_pileup", "bgr_write_depth"):
        assert hasattr(L, name), name
    assert B.PILEUP_DTYPE.itemsize == 24 and B.PILEUP_DTYPE.names == ("depth", "a", "c", "g", "t", "n")
