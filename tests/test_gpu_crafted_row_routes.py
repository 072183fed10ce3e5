"""The crafted rows of test_gpu_crafted_rows.py on the routes its seam (ASCII reads, bgr_aligner_path_stats) does not reach: the pileup kernel's
plane source (host-packed planes; planes made by the pre-pass, from reads end to end and from reads scattered in a text) and its text source,
the text call's record, GAF (plain, wide, tagged) and correction kernels with the "bug compaction" exit of the last two, and rows that do not lie
wholly inside the launch's arena.

How: option test.keep_rows.  A batch is mapped once by the route under test, which sizes every buffer; the test writes its own (results, arena)
through bgr_aligner_device_results; the same call is repeated with the option set: it does everything again but the mapping passes, so the
counting kernels read this launch's own read characters (planes, or the text) and the format launches read the text, all over the crafted rows.
Everything is compared exactly with the plain-Python definitions (gaf_ref, pileup_ref, strands_ref, abundance_ref, links_ref, triples_ref,
haplotag_ref; the corrected read: corrected_ref below, checked against wide_greedy_ref.recover_path).

The sets (rows_of_set): "all" = crafted(k) plus reads of the lengths around the 16- and 32-character steps of the plane source, an N at the
positions around them, under flipped unitigs, on both strands; "fasta" = those longer than k (what a FASTA parser accepts); "walks" = the rows
of "fasta" that spell a walk (GAF and correction end at the first row that does not); "exit ..." = "walks" and exactly one row that spells no walk.

Which source the pileup reads follows from the launch: ASCII or text characters where the sixteen-reads-per-wave greedy kernel packs the reads
itself (k <= 32 here, knob BGR_KNOB_GREEDY_PREPASS off), planes everywhere else -- so the text source runs at k = 15 only, as in production.

Rows outside the arena (test_rows_outside_the_arena): a row with results.x + ints > the arena ints of the launch is an empty row to every reader.
The test cannot fault even without a guard: a launch of three times the reads comes first, so the arena's allocation reaches far beyond the small
launch's logical size, and every int a guardless reader would follow holds a valid id or offset -- it would count them, and the comparison fail.
No text-route set holds such a row: the text kernels do not check that bound (only this seam can hand them foreign rows), and no crafted
offset points outside the allocation."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import abundance_ref as A
import bgreat_amd as B
import gaf_ref as G
import haplotag_ref as H
import links_ref as K
import pileup_ref as P
import strands_ref as S
import triples_ref as T
import wide_greedy_ref as W
from test_gpu_crafted_rows import ALIGNED, KS, RC, Row, crafted, flat_of, pairs
from test_gpu_haplotag import crafted_table
from test_gpu_variants import rc
from test_wide_k_host import pack

N_AT = (0, 15, 16, 31, 32)                       # read positions of an N (and the last one): both sides of the 16-character turns and of the plane's word
LENGTHS = (31, 32, 33, 47, 48, 49, 64, 65)       # and k itself; those >= k
KEEP = {"test.keep_rows": 1}
CAPS = {"test.links_capacity": 1 << 14, "test.triples_capacity": 1 << 15}   # (crafted pairs and triples are none of the graph: its bounds do not hold for them)
VARIANTS = [(1, 1), (0, 2), (1, 2), (0, 1)]      # (strands, form of the abundance and links kernels)
REGION = 128                                     # ints behind the arena's logical end that the rows outside it lie in


# ---- the sets -----------------------------------------------------------------------------------------------------------------------------------
def arrange(rows, order):
    """copies of rows[i] for i in order, .share following"""
    at = {i: j for j, i in enumerate(order)}
    out = []
    for i in order:
        r = rows[i]
        x = Row(r.tag, r.status, r.path, r.read, base=r.base)
        x.at_end = r.at_end
        x.share = at.get(r.share) if r.share is not None else None
        out.append(x)
    return out


def place(rows, seed, bound=None, room=0):
    """the two device arrays as crafted() lays them out: rows in an order of their own, gaps, what no row owns filled with a pattern"""
    rnd = random.Random(seed)
    n, total = len(rows), sum(len(r.read) for r in rows)
    bound = 2 * (total + 8 * n) if bound is None else bound
    arena = np.full(bound + room, 0x5A5A5A5A, dtype=np.int32)
    results = np.zeros((n, 2), dtype=np.uint32)
    at, where = 0, {}
    for i in rnd.sample(range(n), n):
        r = rows[i]
        if r.share is not None or not r.path or getattr(r, "x", None) is not None:
            continue
        x = bound - len(r.path) if r.at_end else at
        if not r.at_end:
            at += len(r.path) + rnd.randrange(3)
        arena[x:x + len(r.path)] = r.path
        where[i] = x
    assert at + 64 < bound
    for i, r in enumerate(rows):
        if getattr(r, "x", None) is not None:
            x = r.x   # (a row outside the arena: its ints are written by the caller)
        else:
            x = where[r.share] if r.share is not None else where.get(i, rnd.randrange(bound))
            assert x + len(r.path) <= bound
        results[i] = (x, len(r.path) | (r.status << 24))
    return {"rows": rows, "results": results, "arena": arena, "bound": bound, "total": total}


def chain_ids(k):
    """48 consecutive unitigs of the chain as one crafted row walks them"""
    return next(r for r in crafted(k)["rows"] if r.tag == "valid" and len(r.path) == 49).base[1:]


def extra_rows(k):
    """reads of every length of LENGTHS, forward and ST_RC, along the genome and against it: an N at every position of N_AT and at the last one,
    one substitution, every unitig behind the first glued on against its sign"""
    us, ids, rnd = crafted(k)["us"], chain_ids(k), random.Random(7000 + k)
    out = []
    for L in sorted({k, *LENGTHS}):
        if L < k:
            continue
        for status in (ALIGNED, RC):
            for against in (False, True):
                nu = 2
                while True:
                    a = rnd.randrange(0, len(ids) - nu + 1)
                    sub = [-x for x in reversed(ids[a:a + nu])] if against else ids[a:a + nu]
                    walk, off = G.walk_of(us, k, [0] + sub)[0], rnd.randrange(3)
                    if len(walk) >= off + L:
                        break
                    nu += 1
                q = list(walk[off:off + L])
                t = rnd.randrange(L)
                q[t] = rnd.choice([c for c in "ACGT" if c != q[t]])
                read = list(rc("".join(q)) if status & W.ST_RC else q)
                for p in (*N_AT, L - 1):
                    if p < L:
                        read[p] = "N"
                out.append(Row("n-flip", status, [off] + sub[:1] + [-x for x in sub[1:]], "".join(read), base=[off] + sub))
    return out


def walks(us, k, r):
    return not r.path or G.walk_of(us, k, r.path) is not G.NO_WALK


def breaks_late(us, k, r):
    """a row whose unitigs do not glue: False = the break is among the first sixteen, True = behind them; None for every other row"""
    if len(r.path) < 3 or r.path[0] < 0 or G.walk_of(us, k, [0] + r.path[1:]) is not G.NO_WALK:
        return None
    return G.walk_of(us, k, [0] + r.path[1:17]) is not G.NO_WALK


@functools.lru_cache(maxsize=None)
def rows_of_set(k, name):
    """-> dict(k, us, rows, results, arena, bound, total); name: "all", "fasta", "walks" or "exit <first|middle|last> <early|late>" """
    c = crafted(k)
    us = c["us"]
    if name == "all":
        rows = c["rows"] + extra_rows(k)
        order = list(range(len(rows)))
        random.Random(8000 + k).shuffle(order)
        rows = arrange(rows, order)
    elif name == "fasta":
        rows = rows_of_set(k, "all")["rows"]
        rows = arrange(rows, [i for i, r in enumerate(rows) if len(r.read) > k])
    elif name == "walks":
        rows = rows_of_set(k, "fasta")["rows"]
        rows = arrange(rows, [i for i, r in enumerate(rows) if walks(us, k, r)])
    else:
        _, where, when = name.split()
        rows = rows_of_set(k, "walks")["rows"]
        fasta = rows_of_set(k, "fasta")["rows"]
        bad = next(r for r in fasta if r.share is None and breaks_late(us, k, r) is (when == "late"))
        n = len(rows)
        at = {"first": 0, "middle": n // 2, "last": n}[where]
        both = rows + [bad]
        rows = arrange(both, list(range(at)) + [n] + list(range(at, n)))
    d = place(rows, 9000 + k)
    d.update(k=k, us=us)
    return d


@functools.lru_cache(maxsize=None)
def expected(k, name):
    """every table over the set, from the definitions"""
    c = rows_of_set(k, name) if name != "outside" else outside_rows(k)
    return tables_of(c["us"], k, c["rows"], c.get("seen"))


def tables_of(us, k, rows, seen=None):
    reads, prs = [r.read for r in rows], seen if seen is not None else pairs(rows)
    return {"pileup": P.pileup_of(us, k, reads, prs), "forward": S.forward_of(us, k, reads, prs),
            "abundance": A.abundance_of(A.unitig_lens(us), k, [len(x) for x in reads], prs)[1:],
            "links": K.sorted_links(K.links_of(prs, len(us) - 1)), "triples": T.sorted_triples(T.triples_of(prs, len(us) - 1))}


def corrected_ref(us, k, r):
    """what -c writes for a mapped read: the walk from the row's offset on, as long as the read or to the walk's end, reverse complemented for ST_RC"""
    walk = G.walk_of(us, k, r.path)[0]
    c = walk[r.path[0]:r.path[0] + len(r.read)]
    return rc(c) if r.status & W.ST_RC else c


def header_of(i, fastq=False):
    """headers of different lengths; some with text behind the name, a tab, or no name at all"""
    name = "" if i % 29 == 7 else "r%d" % i
    rest = ("", " " + "x" * (i % 37), "\tt%d" % i)[i % 3]
    return ("@" if fastq else ">") + name + (rest if name or rest else " -")


def text_of(rows, fastq=False):
    heads = [header_of(i, fastq) for i in range(len(rows))]
    recs = [h + "\n" + r.read + "\n" + ("+\n" + "I" * len(r.read) + "\n" if fastq else "") for h, r in zip(heads, rows)]
    return heads, "".join(recs).encode("latin-1")


def records_ref(heads, rows):
    """want_output 1: header, then the row's ints each with a '.' behind it; an empty row: header and read into the other stream"""
    p = "".join(h + "\n" + "".join("%d." % v for v in r.path) + "\n" for h, r in zip(heads, rows) if r.path)
    return p.encode("latin-1"), unmapped_ref(heads, rows)


def unmapped_ref(heads, rows):
    return "".join(h + "\n" + r.read + "\n" for h, r in zip(heads, rows) if not r.path).encode("latin-1")


def gaf_lines_ref(us, k, heads, rows, table=None):
    out = []
    for h, r in zip(heads, rows):
        if r.path:
            line = G.line_of(h, r.read, G.stats(us, k, r.read, r.status, r.path))
            out.append(H.tagged_line(line, H.tag_of(table, r.path)) if table else line)
    return "".join(out).encode("latin-1")


def corrected_lines_ref(us, k, heads, rows):
    return "".join(h + "\n" + corrected_ref(us, k, r) + "\n" for h, r in zip(heads, rows) if r.path).encode("latin-1")


# ---- rows outside the arena ---------------------------------------------------------------------------------------------------------------------
def plan_of_reads(c, reads):
    return B.plan_launch(k=c["k"], slot_fill_x100=150, table_bytes=4096, graph_bases=2 * sum(len(u) for u in c["us"]), n_unitigs=len(c["us"]) - 1, max_unitig_len=c["k"] + 6,
                         mode=B.MODE_GREEDY, max_mismatch=2, max_read_len=max(len(x) for x in reads), n_reads=len(reads), total_bases=sum(len(x) for x in reads),
                         wide_keys=int(c["k"] > 32))


@functools.lru_cache(maxsize=None)
def outside_rows(k):
    """the "all" set with five rows more, to lie at the arena's logical end `cap`: one ending exactly at cap (counted), the same row one int
    longer, two ints from cap - 1, a row from cap on and one from cap + 100 on -> dict(rows, special, seen: the rows as every reader must take them)"""
    c = rows_of_set(k, "all")
    us, ids, rnd = c["us"], chain_ids(k), random.Random(9500 + k)
    # two consecutive unitigs of the chain with positive signs, the first at most k: arena[cap - 1] and arena[cap] are ids of two rows and offsets of two others
    m, run = None, None
    for cand in (ids, [-x for x in reversed(ids)]):
        for j in range(4, len(cand)):
            if 0 < cand[j - 1] <= k and cand[j] > 0 and m is None:
                m, run = j, cand
    assert m is not None
    w = run[m - 4:m + 1]                                   # five unitigs, w[-2] and w[-1] as above
    behind = ids[:47]                                      # the unitigs behind arena[cap]: a walk of at least k + 46 >= 61 >= any id
    walk_of = lambda x: G.walk_of(us, k, [0] + x)[0]
    assert w[-1] <= len(walk_of(behind))

    def read_on(walk, off, status):
        q = (walk[off:] + "".join(rnd.choice("ACGT") for _ in range(k + 2)))[:k + 2 + rnd.randrange(20)]
        return rc(q) if status & W.ST_RC else q

    special = [Row("control", ALIGNED, [1] + w[:-1], read_on(walk_of(w[:-1]), 1, ALIGNED)),
               Row("outside", RC, [1] + w, read_on(walk_of(w), 1, RC)),
               Row("outside", ALIGNED, [w[-2], w[-1]], read_on(us[w[-1]], w[-2], ALIGNED)),
               Row("outside", RC, [w[-1]] + behind, read_on(walk_of(behind), w[-1], RC)),
               Row("outside", ALIGNED, [3] + ids[10:19], read_on(walk_of(ids[10:19]), 3, ALIGNED))]
    assert all(G.walk_of(us, k, r.path) is not G.NO_WALK for r in special)   # (what a guardless reader would count)
    n = len(c["rows"])
    order = list(range(n))
    for j, at in enumerate((12, 200, 201, 350, 500)):
        order.insert(at, n + j)
    rows = arrange(c["rows"] + special, order)
    for r in rows:
        r.at_end = False
    special = [rows[order.index(n + j)] for j in range(5)]
    return {"k": k, "us": us, "rows": rows, "special": special, "ids": ids, "seen": [(r.status, [] if r.tag == "outside" else r.path) for r in rows]}


@functools.lru_cache(maxsize=None)
def outside(k, cap):
    """the device arrays of outside_rows(k) for an arena of `cap` ints (bgr_aligner_arena_ints), REGION ints longer: every int of
    [cap - 8, cap + REGION) is a valid id, and a plausible offset where a guardless reader would take it for one"""
    c = outside_rows(k)
    rows, special, ids = c["rows"], c["special"], c["ids"]
    for r, x in zip(special, (cap - 5, cap - 5, cap - 1, cap, cap + 100)):
        r.x = x
    d = place(rows, 9600 + k, bound=cap, room=REGION)
    d["arena"][cap - 8:] = [ids[i % len(ids)] for i in range(REGION + 8)]
    for r in special:
        d["arena"][r.x:r.x + len(r.path)] = r.path
    assert list(d["arena"][cap - 5:cap + 1]) == special[1].path and d["arena"][cap + 100] == 3
    assert all(r.x + len(r.path) <= cap + REGION for r in special)
    d.update(c)
    d["cap"] = cap
    return d


# ---- without a device ---------------------------------------------------------------------------------------------------------------------------
def classes_of(us, k, rows):
    n = dict.fromkeys(("flip_lane1", "flip_lane15", "flip_lane0_pass2", "flip_lane0_pass3", "rc_overhang", "fw_overhang", "n_under_flip", "shared", "at_end", "empty"), 0)
    for r in rows:
        n["shared"] += r.share is not None
        n["at_end"] += r.at_end
        n["empty"] += not r.path
        if not r.path or G.walk_of(us, k, r.path) is G.NO_WALK:
            continue
        walk, orient = G.walk_of(us, k, r.path)
        flipped = [j for j, x in enumerate(r.path[1:]) if orient[j] != (x > 0)]
        for key, j in (("flip_lane1", 1), ("flip_lane15", 15), ("flip_lane0_pass2", 16), ("flip_lane0_pass3", 32)):
            n[key] += j in flipped
        off, L = r.path[0], len(r.read)
        n["rc_overhang"] += off < len(walk) < off + L and bool(r.status & W.ST_RC)
        n["fw_overhang"] += off < len(walk) < off + L and not r.status & W.ST_RC
        if "N" in r.read and flipped:
            p = P.pileup_of(us, k, [r.read], [(r.status, r.path)])
            n["n_under_flip"] += any(p.alt[abs(r.path[1 + j])][:, 4].sum() > 0 for j in flipped)
    return n


@pytest.mark.parametrize("k", KS)
def test_every_class_of_rows_is_in_every_routes_set(k):
    """from the definitions alone: flips at lane 1, lane 15 and lane 0 of passes 2 and 3, overhangs on both strands, an N under a flipped unitig
    (pileup_ref's N column is not zero there), shared rows and the row at the arena's end are in every set; the extra reads hold their Ns and
    lengths on both strands; the exit sets hold exactly one row that spells no walk, where and of the kind their names say"""
    us = crafted(k)["us"]
    for name in ("all", "fasta", "walks"):
        c = rows_of_set(k, name)
        n = classes_of(us, k, c["rows"])
        assert all(v > 0 for v in n.values()) and n["at_end"] == 1 and n["n_under_flip"] >= 8, (name, n)
        assert c["bound"] == 2 * (c["total"] + 8 * len(c["rows"])) <= plan_of_reads(c, [r.read for r in c["rows"]])["arena_ints"]
        last = next(i for i, r in enumerate(c["rows"]) if r.at_end)
        assert int(c["results"][last][0]) + len(c["rows"][last].path) == c["bound"]
        assert all(len(r.read) > k for r in c["rows"]) == (name != "all") and 200 <= len(c["rows"]) <= 1100
        assert all(walks(us, k, r) for r in c["rows"]) == (name == "walks")
    extra = [r for r in rows_of_set(k, "all")["rows"] if r.tag == "n-flip"]
    assert {len(r.read) for r in extra} == {L for L in (k, *LENGTHS) if L >= k}
    for L in {len(r.read) for r in extra}:
        for status in (ALIGNED, RC):
            some = [r for r in extra if len(r.read) == L and r.status & 7 == status]
            assert some and all({p for p in (*N_AT, L - 1) if p < L} == {i for i, ch in enumerate(r.read) if ch == "N"} for r in some)
            assert all(r.path[2:] == [-x for x in r.base[2:]] and len(r.path) >= 3 and G.walk_of(us, k, r.path)[0] == G.walk_of(us, k, r.base)[0] for r in some)
    n_walks = len(rows_of_set(k, "walks")["rows"])
    for where, at in (("first", 0), ("middle", n_walks // 2), ("last", n_walks)):
        for when in ("early", "late"):
            rows = rows_of_set(k, "exit %s %s" % (where, when))["rows"]
            bad = [i for i, r in enumerate(rows) if not walks(us, k, r)]
            assert bad == [at] and len(rows) == n_walks + 1 and breaks_late(us, k, rows[at]) is (when == "late")
            assert when == "early" or len(rows[at].path) > 17


@pytest.mark.parametrize("k", KS)
def test_the_corrected_read_of_the_test_is_the_references(k):
    """corrected_ref (the walk of gaf_ref, cut) == recover_path + the reverse complement of alignerGreedy.cpp:394-400, on every mapped row of "walks" """
    c = rows_of_set(k, "walks")
    ref = W.GreedyRef(k, c["us"][1:])
    n = 0
    for r in c["rows"]:
        if r.path:
            assert corrected_ref(c["us"], k, r) == ref.corrected(r.read, r.status, r.path), (r.tag, r.path)
            n += len(corrected_ref(c["us"], k, r)) < len(r.read)
    assert n >= 6   # (reads that overhang the walk: the corrected read is shorter)


@pytest.mark.parametrize("k", KS)
def test_the_rows_outside_the_arena_are_what_the_test_says(k):
    reads = [r.read for r in outside_rows(k)["rows"]]
    cap, big = plan_of_reads(outside_rows(k), reads)["arena_ints"], plan_of_reads(outside_rows(k), reads * 3)["arena_ints"]
    c = outside(k, cap)
    rows = c["rows"]
    assert big >= cap + 4 * sum(len(x) for x in reads) > cap + REGION + 64 and len(c["arena"]) == cap + REGION
    ends = [int(c["results"][rows.index(r)][0]) + len(r.path) - cap for r in c["special"]]
    assert ends == [0, 1, 1, 48, 110] and [r.x - cap for r in c["special"]] == [-5, -5, -1, 0, 100]
    assert sum(1 for _, p in c["seen"] if not p) == sum(1 for r in rows if not r.path) + 4
    e, full = expected(k, "outside"), tables_of(c["us"], k, rows)
    assert e["abundance"] != full["abundance"] and e["links"] != full["links"] and e["triples"] != full["triples"]   # (a guardless reader shows)
    assert (e["pileup"].flat() != full["pileup"].flat()).any() and e["pileup"].skipped == full["pileup"].skipped


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------
def aligner_of(g, strands, form, tag_table=None):
    with B.options(**CAPS):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_ABUNDANCE_FORM, form)
        al.set_knob(B.KNOB_LINKS_FORM, form)
        al.abundance_enable()
        al.links_enable()
        al.triples_enable()
        if strands:
            al.pileup_strands_enable()
        else:
            al.pileup_enable()
    if tag_table is not None:
        al.haplotag_enable(tag_table)
    return al


def write_rows(al, c):
    """the tables zeroed, the crafted rows over the launch's"""
    al.sync()
    al.reset_abundance()
    al.reset_links()
    al.reset_triples()
    al.reset_pileup()
    d_results, d_arena, _ = al.device_results()
    B.device_upload(0, d_results, c["results"])
    B.device_upload(0, d_arena, c["arena"])


def check_tables(al, c, e, strands, what):
    table, skipped = al.pileup()
    assert skipped == e["pileup"].skipped, what
    assert np.array_equal(flat_of(table), e["pileup"].flat()), what
    if strands:
        assert np.array_equal(flat_of(al.pileup_forward()), e["forward"].flat()), what
    assert al.abundance().tolist() == e["abundance"], what
    assert al.links_info()["overflow"] == 0 and al.triples_info()["overflow"] == 0
    assert [(int(x["from"]), int(x["to"]), int(x["count"])) for x in al.links()] == e["links"], what
    assert T.as_tuples(al.triples()) == e["triples"], what
    d_arena = al.device_results()[1]
    assert np.array_equal(B.device_download(0, d_arena, len(c["arena"]), np.int32), c["arena"]), what   # (nothing writes the rows)


def packed_call(al, pk, cap):
    """bgr_align_batch_packed with room for `cap` path ints (crafted rows are longer than the mapper's bound) -> rows"""
    n = pk["n"]
    paths, poffs, status = np.empty(cap, dtype=np.int32), np.empty(n + 1, dtype=np.uint64), np.empty(n, dtype=np.uint8)
    s = B.PackedReads(pk["read_offsets"].ctypes.data, pk["fw3"].ctypes.data, pk["hasn"].ctypes.data, pk["nm_index"].ctypes.data if len(pk["nm_index"]) else None,
                      pk["nm_value"].ctypes.data if len(pk["nm_value"]) else None, len(pk["nm_index"]), pk["max_read_len"])
    p = B.Params(B.MODE_GREEDY, 2, 2, 0)
    B._check(B.lib().bgr_align_batch_packed(al.h, C.byref(p), C.byref(s), n, paths.ctypes.data, cap, poffs.ctypes.data, status.ctypes.data))
    return W.rows_of(paths, poffs, status)


def graph_of(c):
    return B.Graph.build(c["k"], *pack(c["us"][1:]))


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_host_packed_planes(k):
    """pack_reads + bgr_align_batch_packed: every table what its definition says over the crafted rows, the rows back verbatim"""
    c, e = rows_of_set(k, "all"), expected(k, "all")
    g, rows = graph_of(c), c["rows"]
    pk = B.pack_reads(*pack([r.read for r in rows]))
    ints = sum(len(r.path) for r in rows)
    for strands, form in VARIANTS:
        al = aligner_of(g, strands, form)
        al.align_packed(pk)
        assert al.arena_ints() >= c["bound"]
        write_rows(al, c)
        with B.options(**KEEP):
            got = packed_call(al, pk, ints + 8)
        assert got == [(r.status, r.path) for r in rows]
        check_tables(al, c, e, strands, (k, strands, form))
        # the seam refuses a launch the buffers were not sized for, and without the option the same call maps
        with B.options(**KEEP):
            with pytest.raises(B.BgrError, match="error -1.*test.keep_rows"):
                al.align_packed(B.pack_reads(*pack([r.read for r in rows[:-1]])))
        mapped = al.align_packed(pk)
        assert W.rows_of(*mapped) == W.rows_of(*B.Aligner(g, 0).align_packed(pk)) != got
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_planes_of_the_pre_pass(k):
    """ASCII reads on the device with BGR_KNOB_GREEDY_PREPASS 1: bgr_pack_reads_kernel's planes feed the pileup"""
    c, e = rows_of_set(k, "all"), expected(k, "all")
    g, rows = graph_of(c), c["rows"]
    rb, ro = pack([r.read for r in rows])
    d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
    n, args = len(rows), (len(rows), int(ro[-1]), max(len(r.read) for r in rows))
    for strands, form in VARIANTS:
        al = aligner_of(g, strands, form)
        al.set_knob(B.KNOB_GREEDY_PREPASS, 1)
        al.align_device(d_r.data_ptr(), d_o.data_ptr(), *args, m=2, effort=2)
        write_rows(al, c)
        with B.options(**KEEP):
            al.align_device(d_r.data_ptr(), d_o.data_ptr(), *args, m=2, effort=2)
        al.sync()
        assert W.rows_of(*al.fetch(n, sum(len(r.path) for r in rows))) == [(r.status, r.path) for r in rows]
        check_tables(al, c, e, strands, (k, strands, form))
        al.close()
    d_r.free()
    d_o.free()


def text_call(al, text, want, fastq, keep, **kw):
    with B.options(**(KEEP if keep else {})):
        p, n, info = al.align_fasta_text(text, m=2, effort=2, want_output=want, staged=True, fastq=fastq, **kw)
    return p, n, info


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,prepass", [("fasta", 0), ("fasta", 1), ("fastq", 0)])
@pytest.mark.parametrize("k", KS)
def test_text_piece_records_and_tables(k, fmt, prepass):
    """bgr_align_fasta_text with a stage, want_output 1: the tables over the crafted rows -- the pileup from the text where the mapping kernels pack
    the reads themselves, else from planes made out of the text --, the record bytes the definition writes (by the one-launch format kernel, and
    by the write kernel behind too small a buffer)"""
    name, fastq = ("fasta", False) if fmt == "fasta" else ("all", True)
    c, e = rows_of_set(k, name), expected(k, name)
    g, rows = graph_of(c), c["rows"]
    heads, text = text_of(rows, fastq)
    want_p, want_n = records_ref(heads, rows)
    assert len(want_p) > 1000 and want_n
    for strands, form in VARIANTS:
        al = aligner_of(g, strands, form)
        al.set_knob(B.KNOB_GREEDY_PREPASS, prepass)
        _, _, info = text_call(al, text, 1, fastq, False)
        assert not info["irregular"] and info["n_accepted"] == info["n_records"] == len(rows)
        if k <= 32:
            assert al.launch_info()["four_reads_per_wave"]   # (the kernel that packs the reads itself unless the knob says pre-pass)
        write_rows(al, c)
        got_p, got_n, info = text_call(al, text, 1, fastq, True, paths_cap=2 * len(want_p) + 64)
        assert not info["irregular"] and info["n_accepted"] == len(rows)
        assert got_p == want_p and got_n == want_n
        check_tables(al, c, e, strands, (k, fmt, prepass, strands, form))
        write_rows(al, c)
        got_p, got_n, info = text_call(al, text, 1, fastq, True, paths_cap=1000)   # BGR_E_CAPACITY, then bgr_aligner_fetch_text
        assert got_p == want_p and got_n == want_n
        check_tables(al, c, e, strands, (k, fmt, prepass, strands, form, "small buffer"))
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_text_piece_gaf_and_correction(k):
    """want_output 3 (plain and tagged) and 2 over the rows that spell a walk: the lines of gaf_ref (+ haplotag_ref), the corrected reads, byte for
    byte; the other stream = the records of the empty rows; and the tables as ever"""
    c, e = rows_of_set(k, "walks"), expected(k, "walks")
    g, rows, us = graph_of(c), c["rows"], c["us"]
    table = crafted_table()
    assert len(table) == len(us) and sum(1 for r in rows if r.path and H.tag_of(table, r.path)[0]) > 100
    for fastq in (False, True):
        heads, text = text_of(rows, fastq)
        want_n = unmapped_ref(heads, rows)
        wants = {(3, False): gaf_lines_ref(us, k, heads, rows), (3, True): gaf_lines_ref(us, k, heads, rows, table), (2, False): corrected_lines_ref(us, k, heads, rows)}
        assert b"<" in wants[3, False] and b">" in wants[3, False] and b"\n*\t" in wants[3, False] and b"PS:i:" in wants[3, True]
        for (want, tagged), want_p in wants.items():
            strands, form = VARIANTS[(want + tagged + fastq) % 4]
            al = aligner_of(g, strands, form, table if tagged else None)
            _, _, info = text_call(al, text, want, fastq, False)
            assert not info["irregular"] and info["n_accepted"] == len(rows)
            write_rows(al, c)
            got_p, got_n, info = text_call(al, text, want, fastq, True)
            assert not info["irregular"], (k, want, tagged)
            assert got_p == want_p, (k, want, tagged, fastq)
            assert got_n == want_n
            check_tables(al, c, e, strands, (k, want, tagged, fastq))
            al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("when", ["early", "late"])
@pytest.mark.parametrize("k", KS)
def test_text_piece_exit_on_a_row_that_spells_no_walk(k, when):
    """"walks" plus one row that spells no walk -- its break in the first pass of sixteen unitigs, or in a later one -- at the first, a middle and
    the last accepted read, under want_output 3 and 2: irregular == 2, no stream bytes, the tables what the definitions say; and the next
    ordinary call on that aligner returns what a fresh aligner returns"""
    g = graph_of(rows_of_set(k, "walks"))
    for i, where in enumerate(("first", "middle", "last")):
        name = "exit %s %s" % (where, when)
        c, e = rows_of_set(k, name), expected(k, name)
        heads, text = text_of(c["rows"])
        for want in (3, 2):
            strands, form = VARIANTS[(i + want) % 4]
            al = aligner_of(g, strands, form)
            _, _, info = text_call(al, text, want, False, False)
            assert not info["irregular"] and info["n_accepted"] == len(c["rows"])
            write_rows(al, c)
            got_p, got_n, info = text_call(al, text, want, False, True)
            assert info["irregular"] and info.get("no_walk") and got_p == b"" and got_n == b"", (k, name, want)
            check_tables(al, c, e, strands, (k, name, want))
            if where == "middle":
                fresh = B.Aligner(g, 0)
                for w in (want, 1):
                    assert text_call(al, text, w, False, False) == text_call(fresh, text, w, False, False)
                fresh.close()
            al.close()


def arrays_behind(al, k, big):
    """the arrays for the arena of the launch just made; `big`: the arena ints of the launch before it, which the allocation still holds (bgr_plan_launch's
    numbers, through bgr_aligner_arena_ints): every int the rows name lies inside it"""
    cap = al.arena_ints()
    assert big >= cap + REGION + 64
    return outside(k, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["ascii", "packed"])
@pytest.mark.parametrize("k", KS)
def test_rows_outside_the_arena(k, route):
    """a row that does not lie wholly inside the launch's arena ints is an empty row: to the counting kernels (and not "skipped" to the pileup), to
    bgr_aligner_path_stats (zeros) and to bgr_aligner_fetch (an empty path, the status byte as stored)"""
    r0, e = outside_rows(k), expected(k, "outside")
    g, rows, us = graph_of(r0), r0["rows"], r0["us"]
    reads = [r.read for r in rows]
    n, ints = len(rows), sum(len(p) for _, p in r0["seen"])
    rb, ro = pack(reads)
    rb3, ro3 = pack(reads * 3)
    for strands, form in VARIANTS[:2]:
        al = aligner_of(g, strands, form)
        if route == "ascii":
            d_r, d_o, d_r3, d_o3 = (B.DeviceBuffer(0, x) for x in (rb, ro, rb3, ro3))
            al.align_device(d_r3.data_ptr(), d_o3.data_ptr(), 3 * n, int(ro3[-1]), max(len(x) for x in reads), m=2, effort=2)
            al.sync()
            big = al.arena_ints()
            al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(ro[-1]), max(len(x) for x in reads), m=2, effort=2)
            al.sync()
            c = arrays_behind(al, k, big)
            write_rows(al, c)
            with B.options(**{"test.count_with_path_stats": 1}):
                stats = al.path_stats(d_r.data_ptr(), d_o.data_ptr(), n)
            for i, (r, (st, path)) in enumerate(zip(rows, r0["seen"])):
                assert tuple(int(x) for x in stats[i]) == G.path_stat_row(us, k, r.read, st, path), (k, i, r.tag)
            got = W.rows_of(*al.fetch(n, ints))
            for x in (d_r, d_o, d_r3, d_o3):
                x.free()
        else:
            pk, pk3 = B.pack_reads(rb, ro), B.pack_reads(rb3, ro3)
            al.align_packed(pk3)
            big = al.arena_ints()
            al.align_packed(pk)
            c = arrays_behind(al, k, big)
            write_rows(al, c)
            with B.options(**KEEP):
                got = packed_call(al, pk, ints)
        assert got == r0["seen"]
        assert [p for (_, p), r in zip(got, rows) if r.tag == "control"] == [r0["special"][0].path]
        check_tables(al, c, e, strands, (k, route, strands, form))
        al.close()
