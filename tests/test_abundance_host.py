"""The checker of the abundance output (abundance_ref.py) pinned without the product: over the oracle's rows of every greedy and -G golden
(the exception-plane graphs and the -c runs included) the counts must satisfy three invariants that do not go through the definition's own
code path -- the ids of the golden paths bytes, the k-mers of each read's covered stretch, the bases counted position by position -- plus
hand-checked rows.  And the C-ABI's new surface as far as a machine without a device gets."""
import ctypes as C
import os

import numpy as np

import abundance_ref as A
import bgreat_amd as B
import gaf_ref as G
from test_gaf_host import EXC_GRAPHS, case_args, golden_rows
from util import GOLD, golden_cases, sha


def abundance_cases():
    """every golden of the greedy modes (no -b): -G, -q, -c and the graphs with exception planes too"""
    return [c for c in golden_cases() if not case_args(c)["brute"]]


def paths_bytes(H, rows):
    """the paths file printPath writes for rows (aligner.cpp:600-609): header line, then every int followed by '.'"""
    return "".join("%s\n%s\n" % (H[i], "".join("%d." % x for x in p)) for i, (_, p) in enumerate(rows) if p).encode("latin-1")


def test_invariants_on_every_greedy_golden():
    n_cases = n_mapped = n_exc = n_dog = n_partial = 0
    for case in abundance_cases():
        a, us, H, R, rows = golden_rows(case)
        k, K1 = a["k"], a["k"] - 1
        lens = A.unitig_lens(us)
        table = A.abundance_of(lens, k, [len(r) for r in R], rows)
        assert all(t == [0, 0, 0] for t in table[:1])
        # a. the reads column = the ids of the paths file the reference wrote (a -c run wrote corrected reads instead: no ids there)
        if not a["correct"]:
            pb = paths_bytes(H, rows)
            assert len(pb) == case["paths_len"] and sha(pb) == case["paths_sha256"], case["args"]   # (the rows are the golden's)
            if "paths" in case:
                pb = case["paths"].encode("latin-1")
            assert [t[0] for t in table] == A.ids_in_paths(pb, len(lens) - 1), case["args"]
        assert sum(t[0] for t in table) == sum(len(p) - 1 for _, p in rows if p)
        for i, (st, path) in enumerate(rows):
            if not path:
                continue
            L = len(R[i])
            occ = A.occurrences(lens, k, L, path)
            off, cl = A.covered(lens, k, L, path)
            # b. every k-mer of the covered stretch lies in exactly one unitig (cl from the GAF checker, which spells the walk, where it applies)
            if a["graph"] not in EXC_GRAPHS:
                s = G.stats(us, k, R[i], st, path)
                assert s is not G.NO_WALK and s["cl"] == cl and s["plen"] == A.extents(lens, k, path)[-1][1], (case["args"], i)
            assert sum(max(0, o - K1) for _, o in occ) == max(0, cl - K1), (case["args"], i, path)
            # c. bases, position by position: a walk position counts once per unitig that lies over it -- and that is cl plus what of every
            # junction's k-1 shared positions lies inside the covered stretch
            ext = A.extents(lens, k, path)
            by_pos = sum(sum(1 for s_, e_ in ext if s_ <= p < e_) for p in range(off, off + cl))
            shared = [max(0, min(off + cl, ext[j][1]) - max(off, ext[j + 1][0])) for j in range(len(ext) - 1)]
            assert all(ext[j][1] - ext[j + 1][0] == K1 for j in range(len(ext) - 1))
            assert sum(o for _, o in occ) == by_pos == cl + sum(shared), (case["args"], i, path)
            n_partial += sum(1 for x in shared if 0 < x < K1)
            assert sum(o for _, o in occ) == cl + K1 * sum(1 for x in shared if x == K1) + sum(x for x in shared if x < K1)
            n_mapped += 1
        n_cases += 1
        n_exc += a["graph"] in EXC_GRAPHS
        n_dog += a["anchors"]
    assert n_cases >= 70 and n_mapped >= 8000 and n_exc >= 1 and n_dog >= 1, (n_cases, n_mapped, n_exc, n_dog)


def test_hand_checked_rows():
    """r0 and r2 of syn_r150.fa (the rows test_gaf_host.py pins), worked by hand from the unitig lengths"""
    us = G.load_unitigs(os.path.join(GOLD, "syn_unitig.fa"), 31)
    lens = A.unitig_lens(us)
    assert [lens[i] for i in (363, 364, 366, 367)] == [61, 87, 61, 43]
    # extents (0, 61) (31, 118) (88, 149) (119, 162): plen 162, the read covers [8, 158)
    assert A.occurrences(lens, 31, 150, [8, 363, 364, -366, 367]) == [(363, 53), (364, 87), (366, 61), (367, 39)]
    t = A.abundance_of(lens, 31, [150], [(2, [8, 363, 364, -366, 367])])
    assert t[363] == [1, 53, 23] and t[364] == [1, 87, 57] and t[366] == [1, 61, 31] and t[367] == [1, 39, 9] and sum(x[0] for x in t) == 4
    # mapped on the reverse complement: the strand does not enter.  lengths 87 61 89 61, extents (0, 87) (57, 118) (88, 177) (147, 208), covers [32, 182)
    assert A.occurrences(lens, 31, 150, [32, -1009, -1008, -1006, 1005]) == [(1009, 55), (1008, 61), (1006, 89), (1005, 35)]
    # a read that ends in front of the walk's last unitigs still counts them as reads, with no bases; twice the same unitig counts twice
    lens2 = [0, 40, 35, 50]
    t = A.abundance_of(lens2, 31, [20, 100], [(2, [5, 1, -2, 3]), (6, [0, 2, 2])])
    # first: extents (0, 40) (10, 45) (15, 65), covers [5, 25): o = 20, 15, 10.  second: extents (0, 35) (5, 40), plen 40, cl = 40: o = 35, 35
    assert t == [[0, 0, 0], [1, 20, 0], [3, 85, 10], [1, 10, 0]]
    assert A.abundance_of(lens2, 31, [20], [(0, [])]) == [[0, 0, 0]] * 4
    # an offset behind the walk's end covers nothing
    assert A.occurrences(lens2, 31, 20, [60, 1, 2]) == [(1, 0), (2, 0)]


def test_text_round_trip():
    lens, table = [0, 31, 45], [[0, 0, 0], [2, 50, 0], [0, 0, 0]]
    b = A.text_of(lens, table)
    assert b == b"#unitig\tlength\treads\tbases\tkmers\n1\t31\t2\t50\t0\n2\t45\t0\t0\t0\n"
    assert A.parse_text(b) == (lens, table)
    assert A.ids_in_paths(b">a\n3.1.-2.1.\n>b x\n0.2.\n", 2) == [0, 2, 2]


def test_write_abundance_bytes(tmp_path):
    """bgr_write_abundance is host code: header line, one line per unitig in order, zero rows included, 64-bit values in full"""
    g = B.Graph.from_fasta(os.path.join(GOLD, "syn_unitig.fa"), 31)
    us = G.load_unitigs(os.path.join(GOLD, "syn_unitig.fa"), 31)
    lens = A.unitig_lens(us)
    n = g.info()["n_unitigs"]
    assert n == len(lens) - 1
    rows = np.zeros((n, 3), dtype=np.uint64)
    rows[0] = (1, 2, 3)
    rows[6] = (2 ** 64 - 1, 2 ** 40 + 7, 10 ** 19)
    rows[n - 1] = (5, 0, 9)
    f = str(tmp_path / "ab.tsv")
    B.write_abundance(f, g, rows)
    table = [[0, 0, 0]] + [[int(x) for x in r] for r in rows]
    got = open(f, "rb").read()
    assert got == A.text_of(lens, table) and got.count(b"\n") == n + 1
    assert b"\n7\t%d\t18446744073709551615\t1099511627783\t10000000000000000000\n" % lens[7] in got
    L = B.lib()
    assert L.bgr_write_abundance(f.encode(), g.h, rows.ctypes.data, n - 1) == -1 and b"n_rows" in L.bgr_last_error()
    assert L.bgr_write_abundance(str(tmp_path / "no" / "dir").encode(), g.h, rows.ctypes.data, n) == -3


def test_cabi_surface(tmp_path):
    L = B.lib()
    for name in ("bgr_aligner_abundance_enable", "bgr_aligner_abundance", "bgr_aligner_reset_abundance", "bgr_graph_abundance", "bgr_write_abundance"):
        assert hasattr(L, name) and name in B.SYMBOLS
    # the new field took the struct's tail padding
    assert C.sizeof(B.RunOptions) == 80 and B.RunOptions.abundance.offset == 76 and B.RunOptions.gaf.offset == 72
    assert C.sizeof(B.UnitigAbundance) == 24 and B.KNOB_ABUNDANCE_FORM == 12
    g = B.Graph.from_fasta(os.path.join(GOLD, "toy_unitig.fa"), 4)
    n = g.info()["n_unitigs"]
    out = np.zeros((n, 3), dtype=np.uint64)
    # no run yet: no totals
    assert L.bgr_graph_abundance(g.h, out.ctypes.data, n) == -1 and b"bgr_align_all" in L.bgr_last_error()
    try:
        g.abundance()
        assert False
    except B.BgrError as e:
        assert "error -1" in str(e)
    # exhaustive mode is refused before any device work, and names -b
    cnt = (C.c_uint64 * 5)()
    secs = C.c_double(0)
    o = B.RunOptions(C.sizeof(B.RunOptions), 1, 1)
    assert o.abundance == 0
    o.abundance = 1
    pb = B.Params(B.MODE_EXHAUSTIVE, 2, 2, 0)
    assert L.bgr_align_all(g.h, C.byref(pb), C.byref(o), b"x.fa", str(tmp_path / "p").encode(), str(tmp_path / "n").encode(), cnt, C.byref(secs)) == -1
    assert b"-b" in L.bgr_last_error() and b"--abundance" in L.bgr_last_error()
    assert not os.path.exists(tmp_path / "p")
    assert L.bgr_graph_abundance(g.h, out.ctypes.data, n) == -1
    try:
        B.align_all(g, "x.fa", str(tmp_path / "p"), str(tmp_path / "n"), mode=B.MODE_EXHAUSTIVE, abundance=True)
        assert False
    except B.BgrError as e:
        assert "-b" in str(e)


def test_plan_chooses_the_form_from_the_numbers():
    """bgr_plan_abundance, no device: form B (2) needs its table of 12 x (n_unitigs + 1) bytes in a workgroup's LDS and k x total_bases < 2^32
    (a walk position lies on at most k occurrences, so no 32-bit counter of such a launch wraps); the automatic choice takes it from one read per
    sixteen unitigs and workgroup on"""
    P = B.plan_abundance
    R, L = 262144, 150
    assert P(6388, 31, R, R * L) == {"form": 2, "blocks": 512, "threads": 1024, "lds_bytes": 12 * 6389}   # two tables per CU
    assert P(6388, 31, R, R * L, form=1)["form"] == 1 and P(6388, 31, R, R * L, form=1)["lds_bytes"] == 0
    assert P(6, 31, R, R * 100) == {"form": 2, "blocks": 512, "threads": 1024, "lds_bytes": 84}
    # the table must fit: 160 KB less the slack = 13 647 unitigs on an MI355X, 64 KB on a device that reports no more
    assert P(13647, 31, R, R * L, form=2) == {"form": 2, "blocks": 256, "threads": 1024, "lds_bytes": 12 * 13648} and P(13647, 31, R, R * L)["form"] == 2
    assert P(13648, 31, R, R * L, form=2)["form"] == 1
    assert P(6388, 31, R, R * L, lds_per_cu=65536, form=2)["form"] == 1 and P(5000, 31, R, R * L, lds_per_cu=65536, form=2)["form"] == 2
    assert P(98866, 31, R, R * L, form=2) == {"form": 1, "blocks": 16384, "threads": 256, "lds_bytes": 0}
    # no counter may wrap: k x total_bases < 2^32, whatever the knob says
    for k in (8, 31, 64):
        edge = (1 << 32) // k
        assert P(6, k, 1000, edge - 1, form=2)["form"] == 2 and P(6, k, 1000, edge, form=2)["form"] == 1 and P(6, k, 1000, edge, form=0)["form"] == 1
    assert P(6388, 31, 5_000_000, 750_000_000, form=2)["form"] == 1
    # automatic: few reads on a table of thousands of counters stay with form A; a workgroup per 64 reads at most
    assert P(6388, 31, 64, 64 * L)["form"] == 1 and P(6388, 31, 64, 64 * L, form=2) == {"form": 2, "blocks": 1, "threads": 1024, "lds_bytes": 12 * 6389}
    assert P(1000, 31, 64, 64 * L)["form"] == 2 and P(1100, 31, 64, 64 * L)["form"] == 1
    assert P(6388, 31, 0, 0)["blocks"] == 0
    out = (C.c_uint32 * 4)()
    assert B.lib().bgr_plan_abundance(6, 31, 1, 1, 0, 0, 3, out) == -1


def test_ids_outside_the_graph_add_nothing_and_have_length_0():
    """rows the mapper never writes (somebody else's: tests/test_gpu_crafted_rows.py): an occurrence whose id is 0 or beyond the graph's adds nothing
    and has length 0 in the walk -- the next unitig still steps back by k - 1 -- by hand, k = 4"""
    lens, k = [0, 10, 12, 9], 4
    for bad in (0, 4, -4, 2000, -(2 ** 31)):
        # extents (0, 10), (7, 7), (4, 16): the read covers [2, 10) = 8 bases of unitig 1 and [4, 10) = 6 of unitig 2
        path = [2, 1, bad, 2]
        assert A.extents(lens, k, path) == [(0, 10), (7, 7), (4, 16)] and A.covered(lens, k, 8, path) == (2, 8)
        assert A.occurrences(lens, k, 8, path) == [(1, 8), (2, 6)]
        assert A.abundance_of(lens, k, [8], [(2, path)]) == [[0, 0, 0], [1, 8, 5], [1, 6, 3], [0, 0, 0]]
        # in front: extents (0, 0), (-3, 7); the read covers [0, 5), all of it on unitig 1
        assert A.extents(lens, k, [0, bad, 1]) == [(0, 0), (-3, 7)] and A.occurrences(lens, k, 5, [0, bad, 1]) == [(1, 5)]
        # behind: extents (0, 10), (7, 7) -- the walk's size is the largest e, 10, so a read of 9 covers [0, 9) of unitig 1
        assert A.extents(lens, k, [0, 1, bad]) == [(0, 10), (7, 7)] and A.covered(lens, k, 9, [0, 1, bad]) == (0, 9) and A.occurrences(lens, k, 9, [0, 1, bad]) == [(1, 9)]
        assert A.covered(lens, k, 20, [2, 1, bad]) == (2, 8) and A.covered(lens, k, 20, [11, 1, bad]) == (11, 0)
        # nothing else in the row: no walk at all
        assert A.abundance_of(lens, k, [8, 8], [(2, [0, bad]), (2, [3, bad, bad])]) == [[0, 0, 0]] * 4
    assert A.valid_id(lens, 3) and A.valid_id(lens, -3) and not A.valid_id(lens, 0) and not A.valid_id(lens, 4)
