"""The checkers of the triples and of the phase records (triples_ref.py, phase_ref.py) check themselves; the graph's bound on distinct triples
against the rows the oracle returns; bgr_triple_canonical, bgr_bubbles_phase and the two writers (host code) against the checkers, through the
library.  No GPU."""
import ctypes as C
import os
import random

import numpy as np

import bgreat_amd as B
import bubbles_ref as BR
import links_ref as K
import oracle_py
import phase_ref as P
import triples_ref as T
from test_abundance_host import abundance_cases
from test_bubbles_host import planted
from test_gaf_host import EXC_GRAPHS, golden_rows
from test_wide_k_host import pack
from util import GOLD


def random_rows(seed, n=40, n_rows=60):
    rnd = random.Random(seed)
    sid = lambda: rnd.choice((1, -1)) * rnd.randint(1, n)
    rows = []
    for _ in range(n_rows):
        ln = rnd.choice((0, 1, 2, 3, 4, 5, 9, 17, 18, 19))
        rows.append((rnd.randint(0, 3), ([rnd.randint(0, 50)] + [sid() for _ in range(ln)]) if ln else []))
    return rows


def flip(rows):
    """every path read from the other strand"""
    return [(st, p[:1] + [-x for x in reversed(p[1:])]) for st, p in rows]


def test_hand_checked_rows():
    assert T.canonical(1, 2, 3) == (1, 2, 3) == T.canonical(-3, -2, -1)
    assert T.canonical(3, -2, 1) == (-1, 2, -3) and T.canonical(2, -1, -2) == (2, 1, -2) == T.canonical(2, 1, -2) and T.canonical(1, 1, 1) == (1, 1, 1) == T.canonical(-1, -1, -1)
    assert T.canonical(-1, 1, -1) == (1, -1, 1) and T.canonical(5, -7, -5) == (5, 7, -5)   # (a == -c: the sign of the middle id decides)
    rows = [(1, [0, 1, 2, 3, 4]), (3, [9, -4, -3, -2]), (1, [0, 1, 2]), (0, []), (1, [3, 7]), (1, [0, 1, 0, 3, 4, 5]), (1, [0, 1, 6, 3]), (1, [0, 1, -2 ** 31, 3, 2, 1])]
    c = T.triples_of(rows, 5)
    assert c == {(1, 2, 3): 1, (2, 3, 4): 2, (3, 4, 5): 1, (-1, -2, -3): 1}   # (0, 6 > n and INT32_MIN are skipped triple by triple; (3, 2, 1) is no mate of (1, 2, 3))
    assert T.sorted_triples(c) == [(1, 2, 3, 1), (-1, -2, -3, 1), (2, 3, 4, 2), (3, 4, 5, 1)]
    assert T.triples_text(c) == b"#from\tvia\tto\tcount\n1\t2\t3\t1\n-1\t-2\t-3\t1\n2\t3\t4\t2\n3\t4\t5\t1\n"
    assert T.sorted_triples({(1, 2, 3): 0}) == [] and T.parse_text(T.triples_text({})) == {}


def test_the_checker_of_the_triples_checks_itself():
    n_triples = 0
    for seed in range(200):
        rows = random_rows(seed)
        c = T.triples_of(rows, 40)
        assert sum(c.values()) == sum(max(0, len(p) - 3) for _, p in rows), seed   # a row of n ids gives n - 2
        assert all(T.canonical(*t) == t and T.canonical(-t[2], -t[1], -t[0]) == t for t in c)   # strand mates collapse
        assert T.triples_of(flip(rows), 40) == c, seed   # flipping every path leaves the counts alone
        assert T.parse_text(T.triples_text(c)) == c, seed   # the text round-trips
        s = T.sorted_triples(c)
        assert [T.key(*t[:3]) for t in s] == sorted(T.key(*t[:3]) for t in s) and len(s) == len(c)
        small = T.triples_of(rows, 20)   # ids beyond n_unitigs are skipped, triple by triple
        assert all(max(abs(x) for x in t) <= 20 for t in small) and all(small.get(t, 0) == n for t, n in c.items() if max(abs(x) for x in t) <= 20)
        n_triples += len(c)
    assert n_triples > 10000


def negated(counts):
    """every link / triple read from the other strand and made canonical again: the same set"""
    return {(K.canonical(*(-x for x in reversed(t))) if len(t) == 2 else T.canonical(*(-x for x in reversed(t)))): n for t, n in counts.items()}


def planted_triples(seed, bubbles, n=150):
    """triple counts that thread some of the neighbour pairs of `bubbles`, and noise"""
    rnd = random.Random(seed)
    out = {}
    for s, m, ins in P.orientations(bubbles):
        for i in ins:
            for j in rnd.sample(range(-n, n + 1), 3) + [x for q in P.orientations(bubbles) if q[0] == m for x in q[2]]:
                if j != 0 and rnd.random() < 0.7:
                    out[T.canonical(i, m, j)] = rnd.randint(1, 9)
    return out


def chain(n_sites, rnd):
    """links of n_sites bubbles in a row, each sharing its sink with the next one's source, ids and orientations shuffled"""
    ids = list(range(1, 3 * n_sites + 2))
    rnd.shuffle(ids)
    o = [x * rnd.choice((1, -1)) for x in ids]
    links = {}
    for i in range(n_sites):
        s, b, c, t = o[3 * i], o[3 * i + 1], o[3 * i + 2], o[3 * i + 3]
        for l in ((s, b), (s, c), (b, t), (c, t)):
            links[K.canonical(*l)] = rnd.randint(1, 5)
    return links, o


def test_the_checker_of_the_phase_checks_itself():
    n_recs = n_called = 0
    for seed in range(120):
        rnd = random.Random(seed)
        links, o = chain(rnd.randint(1, 6), rnd)
        links.update({l: v for l, v in planted(seed, n=len(o) + 40, n_bubbles=3, n_noise=4).items() if min(abs(x) for x in l) > len(o) or rnd.random() < 0.05})   # (bubbles and noise beside the chain, now and then into it)
        bubbles = BR.bubbles_of(links)
        triples = planted_triples(seed, bubbles)
        recs = P.phase_of(bubbles, triples)
        assert P.phase_of(BR.bubbles_of(negated(links)), negated(triples)) == recs, seed   # every link and triple negated and reversed: the same records
        assert P.parse_text(P.phase_text(recs)) == recs
        spelled = {(s, t, b, c) for s, t, (b, c), _ in bubbles}
        for r in recs:
            x, y = P.bubbles_of_record(r)
            assert r[0] > 0 and x in spelled and y in spelled and x != y, (seed, r)
        n_recs += len(recs)
        n_called += sum(P.call(r[5]) != "." for r in recs)
    assert n_recs >= 150 and n_called >= 80, (n_recs, n_called)
    # by hand: 1 -> {2, 3} -> 4 -> {5, 6} -> 7
    links = {(1, 2): 3, (1, 3): 3, (2, 4): 3, (3, 4): 3, (4, 5): 2, (4, 6): 2, (5, 7): 2, (6, 7): 2}
    tr = {(2, 4, 5): 4, (3, 4, 6): 5, (2, 4, 6): 1}
    assert P.phase_of(BR.bubbles_of(links), tr) == [(4, 1, (2, 3), (5, 6), 7, (4, 1, 0, 5))]
    assert P.phase_text(P.phase_of(BR.bubbles_of(links), tr)) == b"#via\tsource\tin1\tin2\tout1\tout2\tsink\tn11\tn12\tn21\tn22\tphase\n4\t1\t2\t3\t5\t6\t7\t4\t1\t0\t5\tcis\n"
    assert P.call((1, 5, 5, 0)) == "trans" and P.call((0, 0, 0, 0)) == "." and P.call((2, 1, 3, 2)) == "."
    # the second bubble stored against its unitigs: via stays 4 (the reading with m > 0), the out branches are read as that reading orients them
    links2 = {K.canonical(*l): n for l, n in {(1, 2): 3, (1, 3): 3, (2, 4): 3, (3, 4): 3, (4, -6): 2, (4, -5): 2, (-6, -7): 2, (-5, -7): 2}.items()}
    assert P.phase_of(BR.bubbles_of(links2), {T.canonical(2, 4, -5): 7}) == [(4, 1, (2, 3), (-5, -6), -7, (7, 0, 0, 0))]


def test_the_kernels_canonical_form_is_the_checkers():
    rnd = random.Random(3)
    ids = [1, -1, 2, -2, 2 ** 30 - 1, -(2 ** 30 - 1)] + [rnd.choice((1, -1)) * rnd.randint(1, 2 ** 30 - 1) for _ in range(30)]
    for a in ids[:12]:
        for b in ids[:12]:
            for c in ids:
                assert B.triple_canonical(a, b, c) == T.canonical(a, b, c), (a, b, c)
    L = B.lib()
    out = B.Triple()
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (2 ** 30, 1, 1), (1, -2 ** 30, 1), (1, 1, -2 ** 31)):
        assert L.bgr_triple_canonical(*bad, C.byref(out)) == -1, bad
    assert L.bgr_triple_canonical(1, 2, 3, None) == -1


def soup(seed, k):
    """a small unitig set that duplicates its own k-mers: pieces of one sequence cut at random with k-1 overlaps, some stored reverse complemented,
    some twice, fans on shared overlaps, a homopolymer of two lengths"""
    rnd = random.Random(seed)
    rs = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    rc = lambda s: "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[ch] for ch in reversed(s))
    G = rs(rnd.randint(8 * k, 20 * k))
    us, p = [], 0
    while p + k <= len(G):
        u = G[p:p + rnd.randint(k, 2 * k)]
        us.append(rc(u) if rnd.random() < 0.4 else u)
        p += len(u) - (k - 1)
    for _ in range(rnd.randint(2, 8)):
        u = rnd.choice(us)
        ov = u[-(k - 1):] if rnd.random() < 0.5 else u[:k - 1]
        for _ in range(rnd.randint(1, 6)):
            v = ov + rs(rnd.randint(1, k)) if rnd.random() < 0.5 else rs(rnd.randint(1, k)) + ov
            us.append(rc(v) if rnd.random() < 0.3 else v)
    us += ["A" * k, "A" * (k + 2), rnd.choice(us), rc(rnd.choice(us))]
    if (k - 1) % 2 == 0:
        h = rs((k - 1) // 2)
        us += [h + rc(h) + rs(3), rs(3) + h + rc(h)]
    rnd.shuffle(us)
    reads = []
    for _ in range(300):
        L = rnd.randint(k + 1, min(len(G), 8 * k))
        at = rnd.randint(0, len(G) - L)
        r = G[at:at + L]
        reads.append(rc(r) if rnd.random() < 0.5 else r)
    for _ in range(60):
        a, b = rnd.choice(us), rnd.choice(us)
        reads.append((a + b[k - 1:] + "A" * k)[:rnd.randint(k + 1, 5 * k)])
    return us, reads


def test_the_bound_holds_on_every_greedy_golden_and_on_degenerate_graphs():
    """the table of triples has at least twice Graph.triples_bound() slots: no rows the oracle returns hold more distinct triples than the bound says --
    every graph of the goldens, those with exception planes and the -G runs included, and small unitig sets that duplicate their own k-mers"""
    graphs, n_cases, n_triples = {}, 0, 0
    for case in abundance_cases():
        a, us, H, R, rows = golden_rows(case)
        gk = (a["graph"], a["k"], a["anchors"])
        if gk not in graphs:
            g = B.Graph.from_fasta(os.path.join(GOLD, a["graph"]), a["k"], anchors=a["anchors"]) if a["anchors"] else B.Graph.from_fasta(os.path.join(GOLD, a["graph"]), a["k"])
            graphs[gk] = (g.triples_bound(), {})
        bound, seen = graphs[gk]
        c = T.triples_of(rows, len(us) - 1)
        assert sum(c.values()) == sum(len(p) - 3 for _, p in rows if len(p) > 3), case["args"]
        seen.update(c)   # the rows of all the graph's cases together
        assert len(seen) <= bound, (case["args"], len(seen), bound)
        n_cases += 1
        n_triples += len(c)
    assert n_cases >= 70 and n_triples >= 3000 and any(k[0] in EXC_GRAPHS for k in graphs), (n_cases, n_triples)
    with B.options(**{"test.wide_keys": 1}):   # the bound is the graph's, whatever the key layout
        gw = B.Graph.from_fasta(os.path.join(GOLD, "syn_unitig.fa"), 31)
    assert gw.triples_bound() == graphs[("syn_unitig.fa", 31, False)][0] > 0
    n_met = 0
    for seed in range(12):
        k = (5, 7, 9, 12, 15, 31)[seed % 6]
        us, reads = soup(seed, k)
        seqs, offs = pack(us)
        g = B.Graph.build(k, seqs, offs)
        rseq, roffs = pack(reads)
        for m, e in ((0, 2), (3, 8)):
            p, po, st = oracle_py.Oracle(k, seqs, offs).align(rseq, roffs, m=m, effort=e)
            rows = [(int(st[i]), [int(x) for x in p[int(po[i]):int(po[i + 1])]]) for i in range(len(reads))]
            c = T.triples_of(rows, len(us))
            assert len(c) <= g.triples_bound(), (seed, k, len(c), g.triples_bound())
            n_met += len(c)
    assert n_met >= 200, n_met


def _hand():
    rnd = random.Random(5)
    us = [""] + ["".join(rnd.choice("ACGT") for _ in range(rnd.randint(9, 20))) for _ in range(9)]
    return us, B.Graph.build(5, *pack(us[1:]))


def test_write_triples_bytes(tmp_path):
    us, g = _hand()
    f = str(tmp_path / "t.tsv")
    counts = {(1, 2, 3): 2 ** 64 - 1, (-1, 2, 3): 1, (1, -2, 3): 2 ** 40 + 1, (1, 2, -3): 0, (9, 9, 9): 5, (4, -5, 4): 7, (2, 1, 9): 3}
    assert all(T.canonical(*t) == t for t in counts)
    arr = np.array([t + (0, n) for t, n in sorted(counts.items(), key=lambda kv: T.key(*kv[0]))], dtype=B.TRIPLE_DTYPE)
    B.write_triples(f, g, arr)
    got = open(f, "rb").read()
    assert got == T.triples_text(counts) and got.count(b"\n") == 7 and b"18446744073709551615" in got   # (the count of 0 is not written)
    assert T.parse_text(got) == {t: n for t, n in counts.items() if n}
    B.write_triples(f, g, arr[:0])
    assert open(f, "rb").read() == T.triples_text({}) == b"#from\tvia\tto\tcount\n"
    B.write_triples(f, g, arr)
    L = B.lib()
    assert L.bgr_write_triples(None, g.h, arr.ctypes.data, len(arr)) == -1 and L.bgr_write_triples(f.encode(), None, arr.ctypes.data, len(arr)) == -1
    assert L.bgr_write_triples(f.encode(), g.h, None, 1) == -1
    assert L.bgr_write_triples(str(tmp_path / "no" / "dir").encode(), g.h, arr.ctypes.data, len(arr)) == -3
    for field, v in (("from", 0), ("via", 10), ("to", -10), ("to", -2 ** 31)):
        bad = arr.copy()
        bad[2][field] = v
        assert L.bgr_write_triples(f.encode(), g.h, bad.ctypes.data, len(bad)) == -1 and b"record 2" in L.bgr_last_error(), (field, v)
    assert L.bgr_write_triples(f.encode(), g.h, arr[::-1].copy().ctypes.data, len(arr)) == -1 and b"sorted" in L.bgr_last_error()
    assert open(f, "rb").read() == got   # (a refused call leaves the file alone)


def test_bubbles_phase_and_its_writer_are_the_checkers(tmp_path):
    L = B.lib()
    n_recs = 0
    for seed in range(60):
        rnd = random.Random(1000 + seed)
        links, o = chain(rnd.randint(1, 6), rnd)
        links.update({l: v for l, v in planted(seed, n=len(o) + 40, n_bubbles=3, n_noise=4).items() if min(abs(x) for x in l) > len(o) or rnd.random() < 0.05})   # (bubbles and noise beside the chain, now and then into it)
        bubbles = BR.bubbles_of(links)
        triples = planted_triples(seed, bubbles)
        if seed % 7 == 0:
            triples = {}
        barr = np.array([(s, t, bc, cnt) for s, t, bc, cnt in bubbles], dtype=B.BUBBLE_DTYPE) if bubbles else np.zeros(0, dtype=B.BUBBLE_DTYPE)
        got = B.bubbles_phase(barr, T.sorted_triples(triples))
        want = P.phase_of(bubbles, triples)
        assert P.as_tuples(got) == want, seed
        assert all(int(r["reserved"]) == 0 for r in got)
        n_recs += len(want)
    assert n_recs >= 80, n_recs
    # the writer, with counts beyond 2^32 and sums beyond 2^64
    us, g = _hand()
    recs = [(4, 1, (2, 3), (5, 6), 7, (4, 1, 0, 5)), (5, -1, (2, -3), (-6, 8), -9, (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 2)), (6, 1, (2, 3), (5, 7), 8, (0, 0, 0, 0)),
            (7, 1, (2, 3), (5, 6), 8, (2 ** 40, 3, 3, 2 ** 40))]
    arr = np.array([(m, s, i, o_, t, 0, n) for m, s, i, o_, t, n in recs], dtype=B.PHASE_DTYPE)
    assert P.as_tuples(arr) == recs
    f = str(tmp_path / "p.tsv")
    B.write_phase(f, g, arr)
    got = open(f, "rb").read()
    assert got == P.phase_text(recs) and [ln.split("\t")[11] for ln in got.decode().split("\n")[1:-1]] == ["cis", "trans", ".", "cis"]
    B.write_phase(f, g, arr[:0])
    assert open(f, "rb").read() == P.phase_text([])
    B.write_phase(f, g, arr)
    assert L.bgr_write_phase(None, g.h, arr.ctypes.data, 4) == -1 and L.bgr_write_phase(f.encode(), None, arr.ctypes.data, 4) == -1 and L.bgr_write_phase(f.encode(), g.h, None, 1) == -1
    assert L.bgr_write_phase(str(tmp_path / "no" / "dir").encode(), g.h, arr.ctypes.data, 4) == -3
    for field, idx, v in (("via", None, 0), ("sink", None, 10), ("in", 1, -10), ("out", 0, -2 ** 31)):
        bad = arr.copy()
        if idx is None:
            bad[1][field] = v
        else:
            bad[1][field][idx] = v
        assert L.bgr_write_phase(f.encode(), g.h, bad.ctypes.data, len(bad)) == -1 and b"record 1" in L.bgr_last_error(), (field, v)
    assert open(f, "rb").read() == got


def test_bubbles_phase_refusals_and_the_cabi_surface(tmp_path):
    L = B.lib()
    for name in ("bgr_aligner_triples_enable", "bgr_aligner_triples", "bgr_aligner_reset_triples", "bgr_aligner_triples_info", "bgr_triple_canonical", "bgr_graph_triples_bound",
                 "bgr_graph_triples_enable", "bgr_graph_triples_enabled", "bgr_graph_triples", "bgr_write_triples", "bgr_bubbles_phase", "bgr_graph_phase_enable", "bgr_graph_phase",
                 "bgr_write_phase"):
        assert hasattr(L, name) and name in B.SYMBOLS
    assert C.sizeof(B.Triple) == 24 == B.TRIPLE_DTYPE.itemsize and B.Triple.count.offset == 16 == B.TRIPLE_DTYPE.fields["count"][1]
    assert C.sizeof(B.Phase) == 64 == B.PHASE_DTYPE.itemsize and B.Phase.count.offset == 32 == B.PHASE_DTYPE.fields["count"][1]
    bub = np.array([(1, 4, (2, 3), (1, 1, 1, 1)), (4, 7, (5, 6), (1, 1, 1, 1))], dtype=B.BUBBLE_DTYPE)
    tri = np.array([(2, 4, 5, 0, 3), (3, 4, 6, 0, 2)], dtype=B.TRIPLE_DTYPE)
    out = np.zeros(4, dtype=B.PHASE_DTYPE)
    n = C.c_uint64(9)
    call = lambda b, nb, t, nt, o=out, cap=4, pn=C.byref(n): L.bgr_bubbles_phase(None if b is None else b.ctypes.data, nb, None if t is None else t.ctypes.data, nt,
                                                                                 None if o is None else o.ctypes.data, cap, pn)
    assert call(bub, 2, tri, 2) == 0 and n.value == 1 and P.as_tuples(out[:1]) == [(4, 1, (2, 3), (5, 6), 7, (3, 0, 0, 2))]
    assert call(bub, 2, tri, 2, o=None, cap=0) == -4 and n.value == 1   # a cap that is too small: the number all the same
    assert call(bub, 2, tri, 2, pn=None) == -1
    for what, msg in ((lambda: call(None, 2, tri, 2), b"null"), (lambda: call(bub, 2, None, 2), b"null"), (lambda: call(bub, 2, tri, 2, o=None), b"null"),
                      (lambda: call(bub, 2, tri[::-1].copy(), 2), b"ascending"), (lambda: call(bub, 2, tri[[0, 0]].copy(), 2), b"ascending")):
        n.value = 9
        assert what() == -1 and msg in L.bgr_last_error() and n.value == 0, msg
    for t, msg in (((0, 4, 5), b"triple 0"), ((2, 4, -2 ** 31), b"triple 0"), ((2 ** 30, 4, 5), b"triple 0"), ((5, 4, 2), b"canonical"), ((-5, -4, -2), b"canonical")):
        bad = np.array([t + (0, 1)], dtype=B.TRIPLE_DTYPE)
        assert call(bub, 2, bad, 1) == -1 and msg in L.bgr_last_error(), t
    badb = bub.copy()
    badb[1]["branch"][0] = 0
    assert call(badb, 2, tri, 2) == -1 and b"bubble 1" in L.bgr_last_error()
    n.value = 9
    assert call(None, 0, None, 0, o=None, cap=0) == 0 and n.value == 0 and len(B.bubbles_phase(bub[:0], [])) == 0
    # the graph's switches: no totals before a run; min_link 0; non-ACGT unitigs; exhaustive mode refused before any device work
    g = B.Graph.from_fasta(os.path.join(GOLD, "toy_unitig.fa"), 4)
    for fn in (L.bgr_graph_triples, L.bgr_graph_phase):
        n.value = 9
        assert fn(g.h, None, 0, C.byref(n)) == -1 and b"bgr_align_all" in L.bgr_last_error() and n.value == 0
    assert not g.triples_enabled() and not g.phase_enabled()
    assert L.bgr_graph_phase_enable(g.h, 1, 0) == -1 and b"min_link" in L.bgr_last_error() and not g.phase_enabled()
    assert L.bgr_graph_phase_enable(None, 1, 1) == -1 and L.bgr_graph_triples_enable(None, 1) == -1
    ge = B.Graph.from_fasta(os.path.join(GOLD, EXC_GRAPHS[0]), 5)
    assert L.bgr_graph_phase_enable(ge.h, 1, 1) == -1 and b"ACGT" in L.bgr_last_error() and not ge.phase_enabled()
    ge.triples_enable()   # (triples need no characters)
    assert ge.triples_enabled()
    cnt = (C.c_uint64 * 5)()
    secs = C.c_double(0)
    o = B.RunOptions(C.sizeof(B.RunOptions), 1, 1)
    pb = B.Params(B.MODE_EXHAUSTIVE, 2, 2, 0)
    run = lambda: L.bgr_align_all(g.h, C.byref(pb), C.byref(o), b"x.fa", str(tmp_path / "p").encode(), str(tmp_path / "n").encode(), cnt, C.byref(secs))
    g.triples_enable()
    assert g.triples_enabled() and not g.links_enabled() and run() == -1 and b"-b" in L.bgr_last_error() and b"--triples" in L.bgr_last_error() and not os.path.exists(tmp_path / "p")
    g.triples_enable(False)
    g.phase_enable(min_link=2)
    assert g.phase_enabled() and not g.triples_enabled() and not g.bubbles_enabled() and run() == -1 and b"-b" in L.bgr_last_error() and b"--phase" in L.bgr_last_error()
    g.phase_enable(False)
    assert not g.phase_enabled() and run() != 0 and b"--phase" not in L.bgr_last_error() and b"--triples" not in L.bgr_last_error()
