"""The checker of the bubbles and of the file's bytes (bubbles_ref.py) checks itself on seeded random link sets; bgr_write_bubbles (host code)
against it byte for byte; the argument errors of the writer and of the calls that are refused before any device work.  No GPU."""
import ctypes as C
import os
import random

import numpy as np

import bgreat_amd as B
import bubbles_ref as BR
import links_ref as K
from test_gaf_host import EXC_GRAPHS
from test_wide_k_host import pack
from util import GOLD


def planted(seed, n=150, n_bubbles=8, n_noise=20, max_count=4):
    """links_ref counts over n unitigs: bubbles on four random unitigs each in random orientations (they may share unitigs and spoil each other),
    and random links on top"""
    rnd = random.Random(seed)
    sid = lambda: rnd.choice((1, -1)) * rnd.randint(1, n)
    counts = {}
    for _ in range(n_bubbles):
        s, b, c, t = (x * rnd.choice((1, -1)) for x in rnd.sample(range(1, n + 1), 4))
        for l in ((s, b), (s, c), (b, t), (c, t)):
            counts[K.canonical(*l)] = rnd.randint(1, max_count)
    for _ in range(n_noise):
        counts[K.canonical(sid(), sid())] = rnd.randint(1, max_count)
    return counts


def test_the_reference_is_closed_under_the_strand_mate():
    """without the canonical filter every bubble is there on both strands, and the filter keeps exactly one of the two"""
    n_found = {1: 0, 2: 0, 3: 0}   # (per threshold: the property is not checked on empty sets)
    for seed in range(300):
        counts = planted(seed)
        for min_link in (1, 2, 3):
            both = BR.all_oriented(counts, min_link)
            recs = BR.bubbles_of(counts, min_link)
            assert len(set(both)) == len(both) == 2 * len(recs), (seed, min_link)
            assert {BR.mate(q) for q in both} == set(both), (seed, min_link)
            assert [(s, t, b, c) for s, t, (b, c), _ in recs] == sorted((q for q in both if abs(q[0]) < abs(q[1])), key=lambda q: BR.okey(q[0])), (seed, min_link)
            assert len({s for s, _, _, _ in recs}) == len(recs)   # an oriented id opens at most one
            n_found[min_link] += len(recs)
    assert min(n_found.values()) >= 50, n_found


def test_hand_checked_bubbles():
    c = {(1, 2): 7, (1, 3): 2, (2, 4): 6, (3, 4): 1}
    assert BR.bubbles_of(c) == [(1, 4, (2, 3), (7, 6, 2, 1))]
    assert BR.bubbles_of(c, 2) == [] and BR.bubbles_of(c, 1) == BR.bubbles_of({K.canonical(-b, -a): n for (a, b), n in c.items()})
    assert BR.bubbles_of({**c, (1, 5): 1}) == [] and BR.bubbles_of({**c, (1, 5): 1}, 2) == []   # three ways out; at 2 the branch 3 is gone as well
    assert BR.bubbles_of({**c, (1, 5): 1, (1, 3): 2, (3, 4): 2}, 2) == [(1, 4, (2, 3), (7, 6, 2, 2))]   # min_link prunes the third way
    assert BR.bubbles_of({**c, K.canonical(5, 2): 1}) == [] and BR.bubbles_of({**c, K.canonical(5, 4): 1}) == []
    assert BR.bubbles_of({(1, 2): 1, (1, 3): 1, (2, 4): 1, (3, -4): 1}) == []
    # walked against its unitigs: the record keeps the orientation of the smaller (s, t)
    assert BR.bubbles_of({K.canonical(-3, -2): 2, K.canonical(-3, 1): 3, K.canonical(-2, 4): 4, K.canonical(1, 4): 5}) == [(-3, 4, (1, -2), (3, 5, 2, 4))]


def _hand_graph():
    """twelve unitigs, k = 5: 2 / 3 differ in one letter, 5 / 6 in two, 8 / 9 in length, 11 / 12 in one letter (read backwards in the fourth bubble)"""
    rnd = random.Random(11)
    rs = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    sub = lambda s, i: s[:i] + {"A": "C", "C": "G", "G": "T", "T": "A"}[s[i]] + s[i + 1:]
    u = [""] + [rs(rnd.randint(9, 30)) for _ in range(12)]
    u[3] = sub(u[2], 4)
    u[6] = sub(sub(u[5], 0), len(u[5]) - 1)
    u[9] = u[8][:3] + "GT" + u[8][3:]
    u[12] = sub(u[11], 2)
    recs = [(1, 4, (2, 3), (7, 6, 2 ** 40 + 1, 1)), (-7, 4, (5, 6), (1, 2, 3, 4)), (7, 10, (8, 9), (2 ** 64 - 1, 0, 5, 5)), (-10, 1, (-11, -12), (9, 8, 7, 6))]
    return u, recs


def test_write_bubbles_bytes(tmp_path):
    u, recs = _hand_graph()
    g = B.Graph.build(5, *pack(u[1:]))
    f = str(tmp_path / "b.tsv")
    arr = np.array(recs, dtype=B.BUBBLE_DTYPE)
    assert BR.as_tuples(arr) == recs
    B.write_bubbles(f, g, arr)
    got = open(f, "rb").read()
    assert got == BR.bubbles_text(u, recs)
    lines = got.decode().split("\n")
    assert lines[0] == "#source\tsink\tbranch1\tbranch2\tlen1\tlen2\tin1\tout1\tin2\tout2\tkind\tdiff" and lines[-1] == "" and len(lines) == 6
    cols = [ln.split("\t") for ln in lines[1:-1]]
    assert [c[10] for c in cols] == ["snv", "mnv", "indel", "snv"]
    assert cols[0][11] == "4:%s>%s" % (u[2][4], u[3][4]) and cols[1][11] == "." and cols[2][4:6] == [str(len(u[8])), str(len(u[8]) + 2)]
    at = len(u[11]) - 1 - 2   # the branches of the fourth are walked reversed: position and letters are those of the reverse complements
    assert cols[3][:4] == ["-10", "1", "-11", "-12"] and cols[3][11] == "%d:%s>%s" % (at, BR.oriented(u, -11)[at], BR.oriented(u, -12)[at])
    assert cols[2][6] == "18446744073709551615" and cols[0][8] == str(2 ** 40 + 1)
    B.write_bubbles(f, g, arr[:0])   # no bubble: the header alone
    assert open(f, "rb").read() == BR.bubbles_text(u, [])
    # the argument errors
    L = B.lib()
    B.write_bubbles(f, g, arr)
    assert L.bgr_write_bubbles(None, g.h, arr.ctypes.data, len(arr)) == -1 and L.bgr_write_bubbles(f.encode(), None, arr.ctypes.data, len(arr)) == -1
    assert L.bgr_write_bubbles(f.encode(), g.h, None, 1) == -1
    assert L.bgr_write_bubbles(str(tmp_path / "no" / "dir").encode(), g.h, arr.ctypes.data, len(arr)) == -3
    for field, idx, v in (("source", None, 0), ("sink", None, 13), ("branch", 0, -13), ("branch", 1, -2 ** 31)):
        bad = arr.copy()
        if idx is None:
            bad[2][field] = v
        else:
            bad[2][field][idx] = v
        assert L.bgr_write_bubbles(f.encode(), g.h, bad.ctypes.data, len(bad)) == -1 and b"record 2" in L.bgr_last_error(), (field, v)
    assert open(f, "rb").read() == got   # (a refused call leaves the file alone)
    blob = B.Graph.from_blob(g.blob())   # a graph created from a blob carries no unitig characters
    assert L.bgr_write_bubbles(f.encode(), blob.h, arr.ctypes.data, len(arr)) == -1 and b"blob" in L.bgr_last_error()
    assert open(f, "rb").read() == got


def test_links_bubbles_refuses_before_any_device_work():
    L = B.lib()
    n = C.c_uint64(7)
    good = np.array([(1, 2, 3), (1, 3, 3), (2, 4, 3), (3, 4, 3)], dtype=B.LINK_DTYPE)
    out = np.zeros(4, dtype=B.BUBBLE_DTYPE)
    call = lambda links, nl, nu, ml, o=out, cap=4, pn=C.byref(n): L.bgr_links_bubbles(0, None if links is None else links.ctypes.data, nl, nu, ml, None if o is None else o.ctypes.data, cap, pn)
    assert call(good, 4, 4, 1, pn=None) == -1
    for what, rc_msg in ((lambda: call(None, 4, 4, 1), b"null"), (lambda: call(good, 4, 4, 1, o=None), b"null"), (lambda: call(good, 4, 4, 0), b"min_link"),
                         (lambda: call(good, 4, 3, 1), b"1 .. n_unitigs"), (lambda: call(good, 4, 2 ** 30, 1), b"2^30"), (lambda: call(good[::-1].copy(), 4, 4, 1), b"ascending"),
                         (lambda: call(good[[0, 0, 1, 2]].copy(), 4, 4, 1), b"ascending")):
        n.value = 7
        assert what() == -1 and rc_msg in L.bgr_last_error() and n.value == 0, rc_msg
    for a, b, msg in ((0, 2, b"1 .. n_unitigs"), (1, 0, b"1 .. n_unitigs"), (-2 ** 31, 1, b"1 .. n_unitigs"), (5, 1, b"1 .. n_unitigs"),
                      (2, 1, b"canonical"), (-2, -1, b"canonical"), (2, -1, b"canonical")):   # an id that is none; links that are not canonical
        bad = np.array([(a, b, 1)], dtype=B.LINK_DTYPE)
        assert call(bad, 1, 4, 1) == -1 and msg in L.bgr_last_error(), (a, b)
    # no link, no bubble -- and no device either
    n.value = 7
    assert call(None, 0, 4, 1, o=None, cap=0) == 0 and n.value == 0 and call(None, 0, 0, 1, o=None, cap=0) == 0
    assert len(B.links_bubbles([], 10)) == 0


def test_cabi_surface(tmp_path):
    L = B.lib()
    for name in ("bgr_links_bubbles", "bgr_aligner_bubbles", "bgr_aligner_bubbles_times", "bgr_graph_bubbles_enable", "bgr_graph_bubbles_enabled", "bgr_graph_bubbles", "bgr_write_bubbles"):
        assert hasattr(L, name) and name in B.SYMBOLS
    assert C.sizeof(B.Bubble) == 48 and B.BUBBLE_DTYPE.itemsize == 48 and B.Bubble.count.offset == 16 and B.BUBBLE_DTYPE.fields["count"][1] == 16 and B.BUBBLES_TILE == 1024
    n = C.c_uint64(7)
    assert L.bgr_aligner_bubbles(None, 1, None, 0, C.byref(n)) == -1 and n.value == 0
    g = B.Graph.from_fasta(os.path.join(GOLD, "toy_unitig.fa"), 4)
    n.value = 7
    assert L.bgr_graph_bubbles(g.h, None, 0, C.byref(n)) == -1 and b"bgr_align_all" in L.bgr_last_error() and n.value == 0   # no run yet: no totals
    assert not g.bubbles_enabled() and L.bgr_graph_bubbles_enable(g.h, 1, 0) == -1 and b"min_link" in L.bgr_last_error() and not g.bubbles_enabled()
    assert L.bgr_graph_bubbles_enable(None, 1, 1) == -1
    # the switch implies link counting for the run, and exhaustive mode is refused before any device work
    g.bubbles_enable(min_link=2)
    assert g.bubbles_enabled() and not g.links_enabled()
    cnt = (C.c_uint64 * 5)()
    secs = C.c_double(0)
    o = B.RunOptions(C.sizeof(B.RunOptions), 1, 1)
    pb = B.Params(B.MODE_EXHAUSTIVE, 2, 2, 0)
    assert L.bgr_align_all(g.h, C.byref(pb), C.byref(o), b"x.fa", str(tmp_path / "p").encode(), str(tmp_path / "n").encode(), cnt, C.byref(secs)) == -1
    assert b"-b" in L.bgr_last_error() and b"--bubbles" in L.bgr_last_error() and not os.path.exists(tmp_path / "p")
    g.bubbles_enable(False)
    assert not g.bubbles_enabled()
    assert L.bgr_align_all(g.h, C.byref(pb), C.byref(o), b"x.fa", str(tmp_path / "p").encode(), str(tmp_path / "n").encode(), cnt, C.byref(secs)) != 0 and b"--bubbles" not in L.bgr_last_error()
    # a graph with characters other than ACGT: a branch read backwards would not spell the reverse complement
    ge = B.Graph.from_fasta(os.path.join(GOLD, EXC_GRAPHS[0]), 5)
    assert ge.info()["has_exceptions"] and L.bgr_graph_bubbles_enable(ge.h, 1, 1) == -1 and b"ACGT" in L.bgr_last_error() and not ge.bubbles_enabled()
