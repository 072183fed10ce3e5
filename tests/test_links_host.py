"""The checker of the link counts and the GFA bytes (links_ref.py) pinned by hand-checked rows; bgr_write_gfa (host code) against it byte for
byte; the bound the table of links is sized by against the oracle's rows of every greedy golden; the choice between the kernel's forms from
plain numbers; and the C-ABI's new surface as far as a machine without a device gets."""
import ctypes as C
import os

import numpy as np

import abundance_ref as A
import bgreat_amd as B
import gaf_ref as G
import links_ref as K
from test_abundance_host import abundance_cases
from test_gaf_host import EXC_GRAPHS, golden_rows
from util import GOLD


def test_hand_checked_rows():
    # (a, b) and (-b, -a) are one link, kept under the smaller key: |a| first, then '+' before '-'
    assert K.canonical(3, 5) == (3, 5) and K.canonical(-5, -3) == (3, 5)
    assert K.canonical(5, 3) == (-3, -5) and K.canonical(-3, -5) == (-3, -5)
    assert K.canonical(3, -5) == (3, -5) and K.canonical(5, -3) == (3, -5)      # its mate is (3, -5) -> itself by the other name
    assert K.canonical(-3, 5) == (-3, 5) and K.canonical(-5, 3) == (-3, 5)
    # (a, -a) is its own mate; (a, a) and (-a, -a) are one link, kept as (a, a)
    assert K.canonical(4, -4) == (4, -4) and K.canonical(-4, 4) == (-4, 4)
    assert K.canonical(4, 4) == (4, 4) and K.canonical(-4, -4) == (4, 4)
    rows = [(2, [8, 363, 364, -366, 367]),        # three links
            (6, [0, -367, 366, -364, -363]),      # the same three from the other strand: neither the status nor path[0] enters
            (2, [5, 7]), (0, []),                 # a path of one unitig and an unmapped read add nothing
            (2, [0, 4, -4, 4, 4, 4, -4]),         # (4, -4) twice, (-4, 4) once, (4, 4) twice
            (2, [0, 9, 0, 9, 2000, 9, 9])]        # ids that are 0 or beyond n_unitigs are skipped with their pairs
    c = K.links_of(rows, 1009)
    assert c == {(363, 364): 2, (364, -366): 2, (-366, 367): 2, (4, -4): 2, (-4, 4): 1, (4, 4): 2, (9, 9): 1}
    # sorted by key = (|a|, a < 0, |b|, b < 0)
    assert K.sorted_links(c) == [(4, 4, 2), (4, -4, 2), (-4, 4, 1), (9, 9, 1), (363, 364, 2), (364, -366, 2), (-366, 367, 2)]
    assert K.sorted_links({(2, 3): 1, (2, -3): 1, (-2, 3): 1, (-2, -1): 1, (2, 10): 0, (1, 7): 5}) == [(1, 7, 5), (2, 3, 1), (2, -3, 1), (-2, -1, 1), (-2, 3, 1)]
    # ... on either side of a pair, the first place and INT32_MIN (whose magnitude no int32 holds) included
    assert K.links_of([(2, [0, 0, 5, 6, 1010, 6, 7, -(2 ** 31), 7, 8]), (2, [0, -(2 ** 31), 1, 2]), (2, [0, 1, -1010])], 1009) == {(5, 6): 1, (6, 7): 1, (7, 8): 1, (1, 2): 1}
    assert K.add_counts({(1, 2): 1}, {(1, 2): 2, (3, 4): 1}) == {(1, 2): 3, (3, 4): 1}
    assert K.gaf_pairs([(False, 1005), (True, 1006), (True, 1008)]) == [(-1005, 1006), (1006, 1008)]
    text = K.gfa_text(["", "ACGTA", "CGTAN"], 4, [[0, 0, 0], [2, 9, 3], [0, 0, 0]], {(1, -2): 2 ** 64 - 1, (1, 2): 0})
    assert text == b"H\tVN:Z:1.0\nS\t1\tACGTA\tLN:i:5\tRC:i:2\tKC:i:3\nS\t2\tCGTAN\tLN:i:5\tRC:i:0\tKC:i:0\nL\t1\t+\t2\t-\t3M\tRC:i:18446744073709551615\n"
    assert K.parse_gfa(text) == (3, [(1, "ACGTA", 5, 2, 3), (2, "CGTAN", 5, 0, 0)], {(1, -2): 2 ** 64 - 1})


def test_the_kernels_canonical_form_is_the_checkers():
    """bgr_link_canonical runs the inline code the kernel runs: the same canonical form as links_ref on every sign and order of small ids (where
    |a| == |b| and the ties live), on random ones up to 2^30 - 1, and a 64-bit key whose integer order is the order of the key tuples"""
    rng = np.random.default_rng(11)
    pairs = [(a, b) for a in range(-4, 5) for b in range(-4, 5) if a and b]
    pairs += [(int(a) * int(sa), int(b) * int(sb)) for a, b, sa, sb in zip(rng.integers(1, 2 ** 30, 2000), rng.integers(1, 2 ** 30, 2000), rng.choice([-1, 1], 2000), rng.choice([-1, 1], 2000))]
    pairs += [(2 ** 30 - 1, -(2 ** 30 - 1)), (-(2 ** 30 - 1), -(2 ** 30 - 1)), (1, 2 ** 30 - 1)]
    keyed = []
    for a, b in pairs:
        c, key = B.link_canonical(a, b)
        assert c == K.canonical(a, b) and B.link_canonical(-b, -a) == (c, key), (a, b)
        assert key == (abs(c[0]) << 33) | ((c[0] < 0) << 32) | (abs(c[1]) << 1) | (c[1] < 0) and 0 < key < 2 ** 63
        keyed.append((key, c))
    keyed = sorted(set(keyed))
    assert [c for _, c in keyed] == sorted({c for _, c in keyed}, key=lambda l: K.key(*l)) and len({k for k, _ in keyed}) == len(keyed)
    L = B.lib()
    out = B.Link()
    for a, b in ((0, 1), (1, 0), (2 ** 30, 1), (1, -2 ** 31)):
        assert L.bgr_link_canonical(a, b, C.byref(out), None) == -1


def _made_up(n):
    rng = np.random.default_rng(n)
    rows = rng.integers(0, 1000, size=(n, 3)).astype(np.uint64)
    rows[0] = (2 ** 64 - 1, 5, 2 ** 64 - 1)
    rows[n - 1] = (0, 0, 0)
    counts = {}
    for _ in range(40):
        a, b = (int(x) * (1 if rng.integers(0, 2) else -1) for x in rng.integers(1, n + 1, size=2))
        counts[K.canonical(a, b)] = int(rng.integers(1, 100))
    counts.update({K.canonical(1, 1): 2 ** 64 - 1, K.canonical(1, -1): 3, K.canonical(-1, 1): 1, K.canonical(n, -2): 7, K.canonical(-n, -(n - 1)): 2 ** 40 + 1, K.canonical(2, 3): 0})
    return rows, counts


def test_write_gfa_bytes(tmp_path):
    """bgr_write_gfa is host code: H line, an S line per unitig in order with zero rows included, L lines sorted by key, 64-bit values in full; a graph
    with non-ACGT unitig characters keeps them"""
    for graph, k in (("syn_unitig.fa", 31), (EXC_GRAPHS[0], 5)):
        g = B.Graph.from_fasta(os.path.join(GOLD, graph), k)
        us = G.load_unitigs(os.path.join(GOLD, graph), k)
        n = g.info()["n_unitigs"]
        assert n == len(us) - 1 and n >= 3 and (graph not in EXC_GRAPHS or (g.info()["has_exceptions"] and any(set(u) - set("ACGT") for u in us)))
        rows, counts = _made_up(n)
        f = str(tmp_path / "g.gfa")
        B.write_gfa(f, g, rows, K.sorted_links(counts))
        table = [[0, 0, 0]] + [[int(x) for x in r] for r in rows]
        got = open(f, "rb").read()
        assert got == K.gfa_text(us, k, table, counts), graph
        assert got.count(b"\nS\t") == n and b"\tRC:i:18446744073709551615\tKC:i:18446744073709551615\n" in got
        assert b"L\t1\t+\t1\t+\t%dM\tRC:i:18446744073709551615\n" % (k - 1) in got and b"L\t2\t+\t3\t+" not in got   # (a zero count writes no line)
        k1, segs, links = K.parse_gfa(got)
        assert k1 == k - 1 and [s[1] for s in segs] == us[1:] and links == {l: c for l, c in counts.items() if c}
        L = B.lib()
        arr = np.array(K.sorted_links(counts), dtype=B.LINK_DTYPE)
        assert L.bgr_write_gfa(f.encode(), g.h, rows.ctypes.data, n - 1, arr.ctypes.data, len(arr)) == -1 and b"n_rows" in L.bgr_last_error()
        assert L.bgr_write_gfa(str(tmp_path / "no" / "dir").encode(), g.h, rows.ctypes.data, n, arr.ctypes.data, len(arr)) == -3
        bad = arr.copy()
        bad[0]["to"] = n + 1
        assert L.bgr_write_gfa(f.encode(), g.h, rows.ctypes.data, n, bad.ctypes.data, len(bad)) == -1
        assert L.bgr_write_gfa(f.encode(), g.h, rows.ctypes.data, n, arr[::-1].copy().ctypes.data, len(arr)) == -1 and b"sorted" in L.bgr_last_error()
        assert open(f, "rb").read() == got   # (a refused call leaves the file alone)


def test_cabi_surface(tmp_path):
    L = B.lib()
    for name in ("bgr_aligner_links_enable", "bgr_aligner_links", "bgr_aligner_reset_links", "bgr_aligner_links_plan", "bgr_aligner_links_info", "bgr_plan_links",
                 "bgr_graph_links_enable", "bgr_graph_links", "bgr_graph_links_bound", "bgr_write_gfa", "bgr_link_canonical", "bgr_graph_links_enabled"):
        assert hasattr(L, name) and name in B.SYMBOLS
    # the run's switch is the graph's: bgr_run_options did not grow
    assert C.sizeof(B.RunOptions) == 80 and B.RunOptions.abundance.offset == 76 and B.RunOptions.gaf.offset == 72
    assert C.sizeof(B.Link) == 16 and B.LINK_DTYPE.itemsize == 16 and B.Link.count.offset == 8 and B.KNOB_LINKS_FORM == 13
    assert "test.links_capacity" in dict(B.option_names())
    g = B.Graph.from_fasta(os.path.join(GOLD, "toy_unitig.fa"), 4)
    n = C.c_uint64(7)
    # no run yet: no totals
    assert L.bgr_graph_links(g.h, None, 0, C.byref(n)) == -1 and b"bgr_align_all" in L.bgr_last_error() and n.value == 0
    try:
        g.links()
        assert False
    except B.BgrError as e:
        assert "error -1" in str(e)
    # exhaustive mode with the switch on is refused before any device work, and names -b and --gfa
    cnt = (C.c_uint64 * 5)()
    secs = C.c_double(0)
    o = B.RunOptions(C.sizeof(B.RunOptions), 1, 1)
    pb = B.Params(B.MODE_EXHAUSTIVE, 2, 2, 0)
    g.links_enable()
    assert L.bgr_align_all(g.h, C.byref(pb), C.byref(o), b"x.fa", str(tmp_path / "p").encode(), str(tmp_path / "n").encode(), cnt, C.byref(secs)) == -1
    assert b"-b" in L.bgr_last_error() and b"--gfa" in L.bgr_last_error()
    assert not os.path.exists(tmp_path / "p") and not os.path.exists(tmp_path / "n")
    assert L.bgr_graph_links(g.h, None, 0, C.byref(n)) == -1
    g.links_enable(False)
    try:   # the keyword sets the switch for the call ...
        B.align_all(g, "x.fa", str(tmp_path / "p"), str(tmp_path / "n"), mode=B.MODE_EXHAUSTIVE, links=True)
        assert False
    except B.BgrError as e:
        assert "-b" in str(e) and "--gfa" in str(e)
    assert not os.path.exists(tmp_path / "p")
    assert not g.links_enabled()
    assert L.bgr_graph_links_enable(g.h, 1) == 0 and g.links_enabled()   # (set through the C-ABI: the keyword puts back what the library says, not a shadow of it)
    try:
        B.align_all(g, str(tmp_path / "missing.fa"), str(tmp_path / "p2"), str(tmp_path / "n2"), links=False)
        assert False
    except B.BgrError as e:
        assert "--gfa" not in str(e)
    assert g.links_enabled()
    g.links_enable(False)
    # ... and puts it back: with the switch off the same call gets as far as the missing file
    try:
        B.align_all(g, str(tmp_path / "x.fa"), str(tmp_path / "p"), str(tmp_path / "n"), mode=B.MODE_EXHAUSTIVE)
        assert False
    except B.BgrError as e:
        assert "--gfa" not in str(e)


def test_the_bound_holds_on_every_greedy_golden():
    """the table of links has at least twice Graph.links_bound() slots: no rows the oracle returns on a golden graph hold more distinct links than the
    bound says -- every graph of the goldens, those with exception planes and the -G runs included"""
    graphs, n_cases, n_links = {}, 0, 0
    for case in abundance_cases():
        a, us, H, R, rows = golden_rows(case)
        gk = (a["graph"], a["k"], a["anchors"])
        if gk not in graphs:
            g = B.Graph.from_fasta(os.path.join(GOLD, a["graph"]), a["k"], anchors=a["anchors"]) if a["anchors"] else B.Graph.from_fasta(os.path.join(GOLD, a["graph"]), a["k"])
            graphs[gk] = (g.links_bound(), {})
        bound, seen = graphs[gk]
        c = K.links_of(rows, len(us) - 1)
        assert sum(c.values()) == sum(len(p) - 2 for _, p in rows if len(p) > 2), case["args"]
        assert len(c) <= bound, (case["args"], len(c), bound)
        seen.update(c)   # ... and neither do the rows of all its cases together
        assert len(seen) <= bound, (case["args"], len(seen), bound)
        n_cases += 1
        n_links += len(c)
    assert n_cases >= 70 and n_links >= 5000 and any(k[0] in EXC_GRAPHS for k in graphs), (n_cases, n_links)
    # the bound is the graph's, whatever the key layout
    with B.options(**{"test.wide_keys": 1}):
        gw = B.Graph.from_fasta(os.path.join(GOLD, "syn_unitig.fa"), 31)
    assert gw.links_bound() == graphs[("syn_unitig.fa", 31, False)][0] > 0


def test_plan_chooses_the_form_from_the_numbers():
    """bgr_plan_links, no device: form B (2) by default exactly where the graph's bound of distinct links is at most half of the 2 048 slots of a
    workgroup's LDS table -- it can never fall through there; the knob forces either form on any graph"""
    P = B.plan_links
    R = 262144
    assert P(48, R) == {"form": 2, "blocks": 512, "threads": 1024, "lds_bytes": 2048 * 12 + 8}
    assert P(1024, R)["form"] == 2 and P(1025, R)["form"] == 1
    assert P(30000, R) == {"form": 1, "blocks": 16384, "threads": 256, "lds_bytes": 0}
    assert P(30000, R, form=2) == {"form": 2, "blocks": 512, "threads": 1024, "lds_bytes": 2048 * 12 + 8}
    assert P(48, R, form=1) == {"form": 1, "blocks": 16384, "threads": 256, "lds_bytes": 0}
    # a workgroup per 64 reads (form B) or 16 reads (form A) at most; the device's CUs bound the grid
    assert P(48, 64)["blocks"] == 1 and P(48, 65)["blocks"] == 2 and P(30000, 17)["blocks"] == 2 and P(30000, 16)["blocks"] == 1
    assert P(48, R, num_cus=8)["blocks"] == 16 and P(30000, R, num_cus=8)["blocks"] == 512
    assert P(48, 0)["blocks"] == 0 and P(30000, 0)["blocks"] == 0
    out = (C.c_uint32 * 4)()
    assert B.lib().bgr_plan_links(6, 1, 0, 3, out) == -1
