"""The kernels that read a launch's result rows -- the path-stats / GAF walk (gaf_stat, walk_pass), the pileup kernel with its strands instance, the
abundance and links kernels in both forms, the CSR gather behind bgr_aligner_fetch -- on rows the mapper never writes: a unitig glued on in the
strand its sign does not name (the second try of the walk, at every lane and at lane 0 of a later pass), paths that spell no walk (found in the
first and in a later pass), ids that are 0, beyond the graph's or INT32_MIN, off == -1, off == plen, off == plen + 1, reads that overhang their
walk's end, on both strands, and rows placed in the arena in any order, shared by two reads, ending on the arena's last int, with empty rows between.

How: one bgr_align_device launch of the reads sizes the buffers; then the test writes its own (results, arena) through bgr_aligner_device_results
and calls bgr_aligner_path_stats with the option test.count_with_path_stats set, which queues every enabled counting kernel once over those rows.
Everything is compared exactly with the plain-Python definitions (gaf_ref, pileup_ref, strands_ref, abundance_ref, links_ref, variants_ref).

The graph: a random genome cut into some sixty unitigs of k .. k + 6 characters that overlap by k - 1 (test_gpu_variants.chain), written in shuffled
order with every third one as its reverse complement -- so the path along the genome has mixed signs -- plus one unitig that glues to nothing.

Known limits.  The pileup reads the characters as ASCII (the caller's reads buffer) through this seam; its plane and text sources, the text call's
record, GAF and correction kernels and their "bug compaction" exit see these rows in test_gpu_crafted_row_routes.py (option test.keep_rows).
Every crafted row here lies wholly inside the arena, below the 2 (total_bases + 8 n) ints every launch plan gives it.  A row that does not is an
empty row to the counting kernels, the path-stats kernel and the CSR gather (include/bgreat_gpu.h, bgr_aligner_device_results): that file tests
it, with rows at, across and behind the arena's logical end inside an allocation made large enough first.  Still not covered anywhere: offsets
that point outside the arena's allocation (a test must not read there), and the text-route kernels on rows outside the arena (they do not check)."""
import functools
import itertools
import random

import numpy as np
import pytest

import abundance_ref as A
import bgreat_amd as B
import gaf_ref as G
import links_ref as K
import pileup_ref as P
import strands_ref as S
import variants_ref as V
import wide_greedy_ref as W
from test_gpu_variants import chain, rc
from test_wide_k_host import pack

KS = [15, 33, 34, 64]   # 33: the last k whose (k-1)-mer fits one window of the walk; 34: the first WIDE one, its second window shifted by 62
N_CHAIN = 60
NUS = [1, 2, 15, 16, 17, 31, 32, 33, 48]   # unitigs per valid path: one, two and three passes of sixteen lanes, and both sides of each edge
FLIP_AT = [2, 16, 17, 32, 33]               # positions in the path (1-based) flipped in every row long enough: lane 1, lane 15, lane 0 of passes 2 and 3 ...
INT32_MIN = -(2 ** 31)
ALIGNED, RC = W.ST_ALIGNED, W.ST_ALIGNED | W.ST_RC


class Row:
    """one read with the row crafted for it: path = [off, ids ...] ([] = not mapped), base = the path before its signs were flipped"""

    def __init__(self, tag, status, path, read, base=None):
        self.tag, self.status, self.path, self.read, self.base = tag, status, list(path), read, list(path if base is None else base)
        self.share = None   # index of the row whose arena row this one uses too
        self.at_end = False   # the row ends on the arena's last int


@functools.lru_cache(maxsize=None)
def crafted(k):
    """-> dict(us, rows, results, arena, bound): the graph's unitigs (us[0] == ""), the reads with their rows, and the two device arrays"""
    rnd = random.Random(1000 + k)
    lens = [k + rnd.randrange(7) for _ in range(N_CHAIN)]
    cu, genome, starts = chain(k, lens, 31 * k)
    order = list(range(1, N_CHAIN + 1))
    rnd.shuffle(order)
    us, sid = [""], {}
    for f, c in enumerate(order, 1):   # unitig f of the file = unitig c of the chain, every third one reversed
        us.append(rc(cu[c]) if f % 3 == 0 else cu[c])
        sid[c] = -f if f % 3 == 0 else f
    us.append("".join(rnd.choice("ACGT") for _ in range(k + 3)))   # glues to nothing
    LONE, n_unitigs = N_CHAIN + 1, N_CHAIN + 1
    K1 = k - 1
    ends = {u[:K1] for u in us[1:LONE]} | {u[-K1:] for u in us[1:LONE]}
    ends |= {rc(e) for e in ends}
    assert not ({us[LONE][:K1], us[LONE][-K1:], rc(us[LONE][:K1]), rc(us[LONE][-K1:])} & ends)

    def stretch(a, nu, against):
        """the nu unitigs from a on, along the genome or against it -> (ids, walk)"""
        ids = [sid[c] for c in range(a, a + nu)]
        walk = genome[starts[a]:starts[a + nu - 1] + lens[a + nu - 2]]
        if against:
            ids, walk = [-x for x in reversed(ids)], rc(walk)
        assert G.walk_of(us, k, [0] + ids)[0] == walk
        return ids, walk

    def pick(nu):
        """a first unitig for a path of nu (a single unitig: one that a read of k + 1 fits)"""
        while True:
            a = rnd.randrange(1, N_CHAIN - nu + 2)
            if nu > 1 or lens[a - 1] >= k + 2:
                return a

    def read_of(walk, off, L, status, n_mut=0, with_n=False, at=()):
        """the read that lies on `walk` from off on (what hangs over its end is random), `at`: walk positions to substitute, n_mut more anywhere"""
        q = list(walk[off:off + L])
        q += [rnd.choice("ACGT") for _ in range(L - len(q))]
        for t in [p - off for p in at if off <= p < off + L] + [rnd.randrange(L) for _ in range(n_mut)]:
            q[t] = rnd.choice([c for c in "ACGT" if c != q[t]])
        if with_n:
            q[rnd.randrange(L)] = "N"
        q = "".join(q)
        return rc(q) if status & W.ST_RC else q

    def valid(nu, against, status, n_mut=1, with_n=False, tag="valid"):
        ids, walk = stretch(pick(nu), nu, against)
        plen = len(walk)
        off = rnd.randrange(0, min(plen - (k + 1), 40) + 1)
        L = rnd.randrange(k + 1, plen - off + 1)
        at = [len(us[abs(ids[0])]) - K1 + rnd.randrange(K1)] if nu > 1 else []   # on the k - 1 characters the first two unitigs share
        return Row(tag, status, [off] + ids, read_of(walk, off, L, status, n_mut, with_n, at))

    rows = []
    # valid paths, along the genome and against it, both statuses, 0-3 substitutions, an N in every third
    bases = []
    for i, (nu, against, status) in enumerate(itertools.product(NUS, (False, True), (ALIGNED, RC))):
        bases.append(valid(nu, against, status, n_mut=i % 4, with_n=i % 3 == 0))
    rows += bases
    # sign flips of unitigs other than the first: the walk is the same one (the second try glues the unitig on in the other strand)
    for i, b in enumerate(bases):
        nu = len(b.path) - 1
        every = i % 4 == (NUS.index(nu) % 4)   # one base row per length (the direction and the status change with the length): every unitig flipped alone
        for p in range(2, nu + 1):
            if every or p in FLIP_AT:
                f = list(b.path)
                f[p] = -f[p]
                rows.append(Row("flip", b.status, f, b.read, base=b.path))
        if nu > 1:
            rows.append(Row("flip-all", b.status, b.path[:2] + [-x for x in b.path[2:]], b.read, base=b.path))
    # no walk
    both = itertools.cycle((ALIGNED, RC))
    for nu in (2, 17, 40):   # the first unitig's sign flipped
        b = valid(nu, nu == 17, next(both))
        rows.append(Row("no-walk", b.status, [b.path[0], -b.path[1]] + b.path[2:], b.read))
    for p, nu in ((2, 3), (16, 17), (17, 20), (33, 40), (2, 40)):   # the unitig that glues to nothing
        for sign in (1, -1):
            b = valid(nu, sign < 0, next(both))
            b.path[p] = sign * LONE
            rows.append(Row("no-walk", b.status, b.path, b.read))
    for bad in (0, n_unitigs + 1, -(n_unitigs + 1), INT32_MIN):   # ids outside the graph, in the first and in the second pass
        for p, nu in ((1, 5), (3, 5), (16, 16), (3, 24), (17, 24), (20, 33), (33, 35)):
            b = valid(nu, bad < 0, next(both))
            b.path[p] = bad
            rows.append(Row("bad-id", b.status, b.path, b.read))
    for status in (ALIGNED, RC):
        b = valid(2, False, status)
        rows.append(Row("no-walk", status, b.path[:1], b.read))   # np == 1: an offset and no unitig
        for nu in (3, 20):
            b = valid(nu, status == RC, status)
            rows.append(Row("no-walk", status, [-1] + b.path[1:], b.read))
    # offsets at and behind the walk's end, reads that hang over it: both statuses, a path of one pass and a longer one
    for status, nu, against in itertools.product((ALIGNED, RC), (7, 16, 17, 37), (False, True)):
        ids, walk = stretch(pick(nu), nu, against)
        plen, L = len(walk), k + 1 + rnd.randrange(60)
        rows.append(Row("off-plen", status, [plen] + ids, read_of(walk, plen, L, status)))
        rows.append(Row("off-behind", status, [plen + 1] + ids, read_of(walk, plen, L, status)))
        L = max(min(L, plen), 19)   # (the read begins on the walk)
        for over in (1, 17, L - 1):
            rows.append(Row("overhang", status, [plen - (L - over)] + ids, read_of(walk, plen - (L - over), L, status, n_mut=2, with_n=over == 17)))
    # placement: two reads on one arena row (the same characters: their substitutions count twice; and other characters), empty rows, any order,
    # unused bits of the status byte
    n0 = len(rows)
    for i in range(0, n0, 9):
        if rows[i].tag in ("valid", "flip", "overhang"):
            r = Row(rows[i].tag, rows[i].status, rows[i].path, rows[i].read if i % 2 else read_of(rc(rows[i].read) if rows[i].status & W.ST_RC else rows[i].read, 0, len(rows[i].read), rows[i].status, n_mut=1), base=rows[i].base)
            r.share = i
            rows.append(r)
    for i in range(25):
        rows.append(Row("empty", (W.ST_NOANCHOR, W.ST_FAILED)[i % 2], [], "".join(rnd.choice("ACGT") for _ in range(k + 1 + rnd.randrange(40)))))
    perm = list(range(len(rows)))
    rnd.shuffle(perm)
    share = {id(rows[i]): rows[rows[i].share] for i in range(len(rows)) if rows[i].share is not None}
    rows = [rows[i] for i in perm]
    for i, r in enumerate(rows):
        r.share = next(j for j, x in enumerate(rows) if x is share[id(r)]) if id(r) in share else None
        if i % 5 == 0:
            r.status |= (0x08, 0x50, 0xF8)[i % 3]
    last = next(r for r in rows if r.tag == "valid" and len(r.path) > 33 and r.share is None and not any(x.share is not None and rows[x.share] is r for x in rows))
    last.at_end = True

    # the arena: rows in an order of their own, gaps between them, what no row owns filled with a pattern
    n, total = len(rows), sum(len(r.read) for r in rows)
    bound = 2 * (total + 8 * n)
    arena = np.full(bound, 0x5A5A5A5A, dtype=np.int32)
    results = np.zeros((n, 2), dtype=np.uint32)
    at, where = 0, {}
    for i in rnd.sample(range(n), n):
        r = rows[i]
        if r.share is not None or not r.path:
            continue
        x = bound - len(r.path) if r.at_end else at
        if not r.at_end:
            at += len(r.path) + rnd.randrange(3)
        arena[x:x + len(r.path)] = r.path
        where[i] = x
    assert at + 64 < bound
    for i, r in enumerate(rows):
        x = where[r.share] if r.share is not None else where.get(i, rnd.randrange(bound))   # (an empty row: its index is never followed)
        results[i] = (x, len(r.path) | (r.status << 24))
        assert x + len(r.path) <= bound and len(r.read) > k
    assert int(results[rows.index(last)][0]) + len(last.path) == bound
    return {"k": k, "us": us, "rows": rows, "results": results, "arena": arena, "bound": bound, "total": total}


def plan_of(c):
    """what bgr_plan_launch gives the launch of these reads (the graph's numbers that do not enter the arena's size: any)"""
    return B.plan_launch(k=c["k"], slot_fill_x100=150, table_bytes=4096, graph_bases=2 * sum(len(u) for u in c["us"]), n_unitigs=len(c["us"]) - 1, max_unitig_len=c["k"] + 6,
                         mode=B.MODE_GREEDY, max_mismatch=2, max_read_len=max(len(r.read) for r in c["rows"]), n_reads=len(c["rows"]), total_bases=c["total"], wide_keys=int(c["k"] > 32))


def pairs(rows, unflipped=False):
    return [(r.status, r.base if unflipped else r.path) for r in rows]


@pytest.mark.parametrize("k", KS)
def test_the_crafted_rows_cover_what_they_should(k):
    """from the definitions alone (no device): every class of rows the tests below are about is in the set, and the set fits the arena"""
    c = crafted(k)
    us, rows, K1 = c["us"], c["rows"], k - 1
    lens = A.unitig_lens(us)
    assert 200 <= len(rows) <= 900 and plan_of(c)["arena_ints"] >= c["bound"]
    n = dict.fromkeys(("flip_lane0", "late_no_walk", "first_no_walk", "rc_overhang", "fw_overhang", "off_plen", "off_behind", "long", "shared_mismatch", "bad_id", "shared", "n", "rc"), 0)
    for r in rows:
        if not r.path:
            continue
        w = G.walk_of(us, k, r.path)
        n["bad_id"] += any(not A.valid_id(lens, x) for x in r.path[1:])
        n["shared"] += r.share is not None
        if w is G.NO_WALK:
            ok16 = len(r.path) > 17 and G.walk_of(us, k, [0] + r.path[1:17]) is not G.NO_WALK
            n["late_no_walk"] += ok16 and r.path[0] >= 0 and G.walk_of(us, k, [0] + r.path[1:]) is G.NO_WALK
            n["first_no_walk"] += not ok16
            n["off_behind"] += r.path[0] >= 0 and G.walk_of(us, k, [0] + r.path[1:]) is not G.NO_WALK
            continue
        walk, orient = w
        off, L, plen = r.path[0], len(r.read), len(walk)
        n["flip_lane0"] += any(j and j % 16 == 0 and orient[j] != (x > 0) for j, x in enumerate(r.path[1:]))
        n["rc_overhang"] += off < plen < off + L and bool(r.status & W.ST_RC)
        n["fw_overhang"] += off < plen < off + L and not r.status & W.ST_RC
        n["off_plen"] += off == plen
        n["long"] += len(r.path) > 33
        n["n"] += "N" in r.read
        n["rc"] += bool(r.status & W.ST_RC)
        q = rc(r.read) if r.status & W.ST_RC else r.read
        ext = A.extents(lens, k, r.path)
        n["shared_mismatch"] += any(q[p - off] != walk[p] and any(ext[j + 1][0] <= p < ext[j][1] for j in range(len(ext) - 1)) for p in range(off, min(off + L, plen)))
        if r.base != r.path:   # a flip leaves the walk alone
            assert G.walk_of(us, k, r.base)[0] == walk and [abs(x) for x in r.base] == [abs(x) for x in r.path] and r.base[:2] == r.path[:2]
    assert all(v > 0 for v in n.values()) and n["flip_lane0"] >= 4 and n["late_no_walk"] >= 4 and n["rc_overhang"] >= 6 and n["off_plen"] >= 8 and n["shared_mismatch"] >= 20, n
    flipped = {p for r in rows if r.base != r.path for p in range(2, len(r.path)) if r.base[p] != r.path[p]}
    assert flipped == set(range(2, 49))
    p = P.pileup_of(us, k, [r.read for r in rows], pairs(rows))
    assert p.skipped >= 20 and len(V.sites_of(p, 2, 2, 200000)) > 0


def run(al, c, d_r, d_o, unflipped=False):
    """the tables zeroed, the rows written over the launch's, then path stats with the counting kernels behind -> the stats"""
    rows = c["rows"]
    al.reset_abundance()
    al.reset_links()
    al.reset_pileup()
    d_results, d_arena, _ = al.device_results()
    arena = c["arena"].copy()
    if unflipped:
        for i, r in enumerate(rows):
            if r.path and r.share is None:
                x = int(c["results"][i][0])
                arena[x:x + len(r.base)] = r.base
    B.device_upload(0, d_results, c["results"])
    B.device_upload(0, d_arena, arena)
    with B.options(**{"test.count_with_path_stats": 1}):
        stats = al.path_stats(d_r.data_ptr(), d_o.data_ptr(), len(rows))
    assert np.array_equal(B.device_download(0, d_arena, c["bound"], np.int32), arena)   # (nothing writes the rows)
    return stats


def flat_of(arr):
    """array of B.PILEUP_DTYPE -> (n, 6) int64, as Pileup.flat()"""
    return np.stack([arr[f] for f in B.PILEUP_DTYPE.names], axis=1).astype(np.int64)


def as_tuples(arr):
    return [tuple(int(x) for x in r) for r in arr]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2], ids=["formA", "formB"])
@pytest.mark.parametrize("k", KS)
def test_crafted_rows(k, form):
    """path stats, the fetched rows, pileup with its skipped count, forward pileup, abundance, links and the SNV sites: each what its definition says
    over the crafted rows; and pileup, forward pileup and abundance the same with the flipped signs put back (the walk does not change)"""
    c = crafted(k)
    us, rows = c["us"], c["rows"]
    n, reads = len(rows), [r.read for r in rows]
    lens = A.unitig_lens(us)
    g = B.Graph.build(k, *pack(us[1:]))
    with B.options(**{"test.links_capacity": 1 << 14}):   # (crafted pairs are no links of the graph: its bound does not hold for them)
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_ABUNDANCE_FORM, form)
        al.set_knob(B.KNOB_LINKS_FORM, form)
        al.abundance_enable()
        al.links_enable()
        al.pileup_strands_enable()
    assert al.abundance_plan(n, c["total"])["form"] == form and al.links_plan(n)["form"] == form
    rb, ro = pack(reads)
    d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
    assert plan_of(c)["arena_ints"] >= c["bound"] == 2 * (int(ro[-1]) + 8 * n)
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(ro[-1]), max(len(x) for x in reads), m=2, effort=2)
    al.sync()
    stats = run(al, c, d_r, d_o)
    # path stats: NO_WALK exactly where the definition says
    n_no_walk = 0
    for i, r in enumerate(rows):
        want = G.path_stat_row(us, k, r.read, r.status, r.path)
        assert tuple(int(x) for x in stats[i]) == want, (k, i, r.tag, r.status, r.path)
        n_no_walk += want[3] == B.PATH_STAT_NO_WALK
    # the rows and the status bytes come back verbatim
    got = W.rows_of(*al.fetch(n, sum(len(r.path) for r in rows)))
    assert got == [(r.status, r.path) for r in rows]
    # pileup, skipped, forward pileup
    p = P.pileup_of(us, k, reads, pairs(rows))
    f = S.forward_of(us, k, reads, pairs(rows))
    table, skipped = al.pileup()
    assert skipped == p.skipped == n_no_walk > 0
    assert np.array_equal(flat_of(table), p.flat())
    fwd = al.pileup_forward()
    assert np.array_equal(flat_of(fwd), f.flat()) and f.flat().any() and (f.flat() != p.flat()).any()
    # abundance, links
    ab = al.abundance()
    assert ab.tolist() == A.abundance_of(lens, k, [len(x) for x in reads], pairs(rows))[1:]
    info = al.links_info()
    assert info["overflow"] == 0 and info["capacity"] == 1 << 14, info
    links = al.links()
    out = [(int(x["from"]), int(x["to"]), int(x["count"])) for x in links]
    assert out == K.sorted_links(K.links_of(pairs(rows), len(us) - 1))
    # the SNV sites of that table
    for prm in ((1, 1, 0), (2, 2, 200000)):
        want = V.sites_of(p, *prm)
        assert as_tuples(al.pileup_sites(*prm)) == want and len(want) > 0, prm
    # the flipped signs put back: other links, the same everything else
    stats0 = run(al, c, d_r, d_o, unflipped=True)
    assert np.array_equal(stats0, stats)
    table0, skipped0 = al.pileup()
    assert skipped0 == skipped and np.array_equal(table0, table) and np.array_equal(al.pileup_forward(), fwd) and np.array_equal(al.abundance(), ab)
    out0 = [(int(x["from"]), int(x["to"]), int(x["count"])) for x in al.links()]
    assert out0 == K.sorted_links(K.links_of(pairs(rows, unflipped=True), len(us) - 1)) and out0 != out
    d_r.free()
    d_o.free()
