"""The cs:Z: field of GAF lines on the GPU (--gaf --cs, bgr_aligner_gaf_cs_enable, bgr_graph_gaf_cs_enable) and bgr_aligner_path_diffs, byte for
byte / entry for entry against gaf_ref.py + gaf_cs_ref.py (the definition in plain Python, checked without the product by test_gaf_cs_host.py).

Crafted rows (the seam of test_gpu_crafted_row_routes.py: option test.keep_rows for the text call, bgr_aligner_device_results for the device call):
a chain graph of 140 short unitigs per k, so that a read of 257 characters crosses four passes of sixteen unitigs; reads of every length around
the 16-character lane step and the 256-character turn; differences at position 0, at the last position, on both sides of the steps, adjacent, none,
at every character, an N, inside the k - 1 characters two unitigs share and on the first new base of the unitigs around the pass borders; both
strands, along the genome and against it, off > 0, overhangs, no aligned character at all; 1 .. 65 reads per launch; rows that spell no walk; rows
at, across and behind the arena's end.  Mapper rows: a seeded Synth graph with mutated reads through the CLI on every route, -q, -G, with and
without a haplotag table, and a round trip that rebuilds every mapped read from the --gfa and --gaf --cs files of one run."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import bgreat_amd as B
import gaf_cs_ref as CS
import gaf_ref as G
import haplotag_ref as H
import wide_greedy_ref as W
from test_gpu_crafted_row_routes import KEEP, arrays_behind, outside_rows, text_of, unmapped_ref
from test_gpu_crafted_rows import ALIGNED, KS, RC, Row, crafted
from test_gpu_triples import ROUTE_IDS, ROUTES, run
from test_gpu_variants import chain, rc
from test_wide_k_host import pack, strings
from tools.synth import Synth

pytestmark = pytest.mark.gpu

N_CHAIN = 140
LENGTHS = (15, 16, 17, 31, 32, 33, 255, 256, 257)   # and k + 1; those above k
LAUNCHES = (1, 3, 4, 5, 63, 64, 65)
PATHS = (1, 2, 16, 17, 33)


# ---- the crafted set ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(k):
    """-> dict(k, us, rows): the chain graph (unitigs in shuffled order, every third one reversed, one that glues to nothing) and the rows"""
    rnd = random.Random(4000 + k)
    lens = [k + rnd.randrange(1, 6) for _ in range(N_CHAIN)]
    cu, genome, starts = chain(k, lens, 53 * k)
    order = list(range(1, N_CHAIN + 1))
    rnd.shuffle(order)
    us, sid = [""], {}
    for f, c in enumerate(order, 1):
        us.append(rc(cu[c]) if f % 3 == 0 else cu[c])
        sid[c] = -f if f % 3 == 0 else f
    us.append("".join(rnd.choice("ACGT") for _ in range(k + 3)))
    LONE, K1 = N_CHAIN + 1, k - 1

    def stretch(a, nu, against):
        """the nu unitigs from a on -> (ids, walk, walk positions of every unitig's first new base)"""
        ids = [sid[c] for c in range(a, a + nu)]
        walk = genome[starts[a]:starts[a + nu - 1] + lens[a + nu - 2]]
        if against:
            ids, walk = [-x for x in reversed(ids)], rc(walk)
        w = G.walk_of(us, k, [0] + ids)
        assert w is not G.NO_WALK and w[0] == walk
        new, at = [], 0
        for j, x in enumerate(ids):
            new.append(at)
            at += len(us[abs(x)]) - (K1 if j else 0)
        assert at == len(walk)
        return ids, walk, new

    def covering(need, against):
        """the fewest unitigs from a random start whose walk has `need` characters"""
        while True:
            a = rnd.randrange(1, N_CHAIN // 4)
            for nu in range(1, N_CHAIN - a + 2):
                ids, walk, new = stretch(a, nu, against)
                if len(walk) >= need:
                    return ids, walk, new

    def row(tag, ids, walk, off, L, status, at=(), every=False, n_at=None):
        """the read on walk[off ...] of L characters (what hangs over the walk's end is random), substitutions at the READ positions `at` that lie in
        its aligned part, at every character, an N at read position n_at; the read as it stands in the input (ST_RC: the reverse complement)"""
        q = list(walk[off:off + L])
        cl = len(q)
        q += [rnd.choice("ACGT") for _ in range(L - cl)]
        on_rc = bool(status & W.ST_RC)
        to_q = lambda p: L - 1 - p if on_rc else p   # read position -> position on the walk's strand
        other = lambda c: rnd.choice([x for x in "ACGT" if x != c])
        for j in (range(cl) if every else sorted({to_q(p) for p in at})):
            if 0 <= j < cl:
                q[j] = other(q[j])
        if n_at is not None and 0 <= to_q(n_at) < L:
            q[to_q(n_at)] = "N"
        q = "".join(q)
        return Row(tag, status, [off] + ids, rc(q) if on_rc else q)

    rows = []
    both = [(s, a) for s in (ALIGNED, RC) for a in (False, True)]
    # every length: none, first, last, around the lane step and the turn, two neighbours, every character, an N
    for L in sorted({k + 1, *LENGTHS}):
        if L <= k:
            continue
        for status, against in both:
            off = rnd.randrange(1, 6)
            ids, walk, _ = covering(off + L, against)
            mid = rnd.randrange(1, L - 2)
            pats = [("none", ()), ("first", (0,)), ("last", (L - 1,)), ("adjacent", (mid, mid + 1)), ("ends", (0, L - 1))]
            if L > 16:
                pats += [("step16", (15, 16)), ("step16a", (15,)), ("step16b", (16,))]
            if L > 256:
                pats += [("turn256", (255, 256)), ("turn256a", (255,)), ("turn256b", (256,)), ("many", tuple(range(3, L, 13)))]
            for tag, at in pats:
                rows.append(row(tag, ids, walk, off, L, status, at))
            rows.append(row("every", ids, walk, off, L, status, every=True))
            rows.append(row("n", ids, walk, off, L, status, at=(mid,), n_at=rnd.choice((0, L - 1, 15, 16, mid + 1)) % L))
    # paths of 1, 2, 16, 17 and 33 unitigs, the read over the whole walk: a difference inside the characters two unitigs share, on the first new base of
    # the unitigs at the pass borders, and runs that cross them
    for nu in PATHS:
        for status, against in both:
            while True:
                a = rnd.randrange(1, N_CHAIN - nu + 1)
                ids, walk, new = stretch(a, nu, against)
                if len(walk) >= k + 2:
                    break
            plen = len(walk)
            off = rnd.randrange(0, min(3, plen - (k + 1)) + 1)
            L = plen - off
            to_read = lambda w: L - 1 - (w - off) if status & W.ST_RC else w - off   # walk position -> read position
            marks = [new[j] for j in (1, 15, 16, 17, 32) if j < nu]                   # first new bases: unitigs 2, 16, 17, 18, 33
            shared = [new[j] - 1 - rnd.randrange(k - 1) for j in (1, 16, 32) if j < nu]
            for tag, ws in (("new-base", marks), ("shared", shared), ("both", marks + shared), ("none", [])):
                rows.append(row("path%d-%s" % (nu, tag), ids, walk, off, L, status, at=[to_read(w) for w in ws if w >= off]))
            rows.append(row("path%d-every" % nu, ids, walk, off, L, status, every=True))
    # reads that hang over the walk's end, and reads with no aligned character
    for status, against in both:
        for nu in (1, 7, 17, 35):
            ids, walk, _ = stretch(rnd.randrange(1, N_CHAIN - nu + 1), nu, against)
            plen, L = len(walk), k + 1 + rnd.randrange(40)
            for over in sorted({1, min(17, L - 2), L - 1}):
                off = max(0, plen - (L - over))
                cl = min(L, plen - off)
                lo = L - cl if status & W.ST_RC else 0
                rows.append(row("overhang", ids, walk, off, L, status, at=(lo, lo + cl - 1)))
            rows.append(row("cl0", ids, walk, plen, L, status))
    for i in range(12):
        rows.append(Row("empty", (W.ST_NOANCHOR, W.ST_FAILED)[i % 2], [], "".join(rnd.choice("ACGT") for _ in range(k + 1 + rnd.randrange(40)))))
    rnd.shuffle(rows)
    next(r for r in rows if r.tag.startswith("path33")).at_end = True   # a row that ends on the arena's last int
    bad = []
    for nu, p in ((3, 2), (20, 17)):   # rows that spell no walk: the break in the first pass, and in the second
        ids, walk, _ = stretch(5, nu, False)
        ids[p - 1] = LONE
        bad.append(Row("no-walk", ALIGNED if nu == 3 else RC, [1] + ids, walk[1:k + 9]))
    return {"k": k, "us": us, "rows": rows, "bad": bad}


def lines_ref(us, k, heads, rows, table=None):
    tag = (lambda line, path: H.tagged_line(line, H.tag_of(table, path))) if table else None
    text, bug = CS.gaf_cs_of(us, k, heads, [r.read for r in rows], [(r.status, r.path) for r in rows], tag)
    assert bug is None
    return text.encode("latin-1")


def table_of(us, k):
    rng = random.Random(17 * k)
    return [0] + [(rng.randrange(1, 7) << 1 | rng.randrange(2)) if rng.random() < 0.5 else 0 for _ in range(len(us) - 1)]


@pytest.mark.parametrize("k", KS)
def test_the_crafted_set_covers_what_it_should(k):
    """from the definitions alone: every class of the module's head is in the set"""
    w = world(k)
    us, rows = w["us"], w["rows"]
    n = dict.fromkeys(("nm0", "nm1", "nm2", "all", "n", "rc", "fw", "first", "last", "step16", "turn256", "adjacent", "cl0", "overhang", "shared", "new17", "pass2", "pass3",
                       "pass4", "one", "long_run"), 0)
    for r in rows:
        if not r.path:
            continue
        s = G.stats(us, k, r.read, r.status, r.path)
        assert s is not G.NO_WALK
        d = [j for j, _, _ in CS.diffs_of(s["Q"], r.read[s["qstart"]:s["qend"]])]
        L, cl, nu = len(r.read), s["cl"], len(r.path) - 1
        n["nm0"] += not d and cl > 0
        n["nm1"] += len(d) == 1
        n["nm2"] += len(d) >= 2
        n["all"] += cl > 0 and len(d) == cl
        n["n"] += "n" in CS.cs_of(r.read, s)
        n["rc" if r.status & W.ST_RC else "fw"] += 1
        n["first"] += bool(d) and d[0] == 0
        n["last"] += bool(d) and d[-1] == cl - 1
        n["step16"] += 15 in d and 16 in d
        n["turn256"] += 255 in d and 256 in d
        n["adjacent"] += any(b == a + 1 for a, b in zip(d, d[1:]))
        n["cl0"] += cl == 0
        n["overhang"] += 0 < cl < L
        n["shared"] += r.tag.endswith("shared") and len(d) >= 1
        n["new17"] += r.tag.endswith("new-base") and nu >= 17
        n["pass2"] += 16 < nu <= 32
        n["pass3"] += 32 < nu <= 48
        n["pass4"] += nu > 48
        n["one"] += nu == 1
        n["long_run"] += any(op[0] == "=" and op[1] >= 100 for op in CS.parse_ops(CS.cs_of(r.read, s)))
    assert all(v > 0 for v in n.values()) and n["rc"] > 100 and n["fw"] > 100 and n["pass4"] >= 8 and n["cl0"] >= 8, n
    assert {len(r.read) for r in rows} >= {x for x in (k + 1, *LENGTHS) if x > k}
    assert {len(r.path) - 1 for r in rows if r.path} >= set(PATHS)
    assert all(G.walk_of(us, k, r.path) is G.NO_WALK for r in w["bad"])


def place(rows, seed):
    """the two device arrays, as test_gpu_crafted_row_routes.place lays them out but for launches of any size: rows in an order of their own inside
    the 2 (bases + 8 reads) ints every launch plan gives its arena, small gaps, a pattern where no row lies"""
    rnd = random.Random(seed)
    n, total = len(rows), sum(len(r.read) for r in rows)
    bound = 2 * (total + 8 * n)
    arena = np.full(bound, 0x5A5A5A5A, dtype=np.int32)
    results = np.zeros((n, 2), dtype=np.uint32)
    at = 0
    for i in rnd.sample(range(n), n):
        r = rows[i]
        x = rnd.randrange(bound)   # (an empty row: its index is never followed)
        if r.path:
            x = bound - len(r.path) if r.at_end else at
            if not r.at_end:
                at += len(r.path) + rnd.randrange(3)
            arena[x:x + len(r.path)] = r.path
        results[i] = (x, len(r.path) | (r.status << 24))
    assert at <= bound - max([len(r.path) for r in rows if r.at_end] + [0])
    return {"results": results, "arena": arena, "bound": bound}


def upload_rows(al, c):
    al.sync()
    d_results, d_arena, _ = al.device_results()
    assert al.arena_ints() >= c["bound"]
    B.device_upload(0, d_results, c["results"])
    B.device_upload(0, d_arena, c["arena"])


def text_call(al, text, keep, **kw):
    with B.options(**(KEEP if keep else {})):
        return al.align_fasta_text(text, m=2, effort=2, want_output=3, staged=True, **kw)


def crafted_lines(al, rows, seed, **kw):
    """the text call over `rows` written into the result buffers -> (paths bytes, notAligned bytes, info, headers)"""
    heads, text = text_of(rows)
    _, _, info = text_call(al, text, False)   # (sizes every buffer)
    assert not info["irregular"] and info["n_accepted"] == len(rows)
    upload_rows(al, place(rows, seed))
    return text_call(al, text, True, **kw) + (heads,)


@pytest.mark.parametrize("k", KS)
def test_crafted_rows_text_call(k):
    """want_output 3 with the switch on, plain and tagged: gaf_ref + gaf_cs_ref, byte for byte, over the whole set and at 1 .. 65 reads per launch;
    with the switch off again, the bytes of an aligner that never had it"""
    w = world(k)
    us, rows = w["us"], w["rows"]
    g = B.Graph.build(k, *pack(us[1:]))
    table = table_of(us, k)
    al, off = B.Aligner(g, 0), B.Aligner(g, 0)
    al.gaf_cs_enable()
    for n in LAUNCHES + (len(rows),):
        part = [Row(r.tag, r.status, r.path, r.read) for r in rows[:n]]
        if n == len(rows):
            for x, r in zip(part, rows):
                x.at_end = r.at_end
        got_p, got_n, info, heads = crafted_lines(al, part, 100 * k + n)
        assert not info["irregular"], (k, n)
        assert got_p == lines_ref(us, k, heads, part), (k, n)
        assert got_n == unmapped_ref(heads, part)
    assert got_p.count(b"\tcs:Z:\n") >= 8 and got_p.count(b"*") > 1000
    # the switch off: today's bytes
    plain, _, _, heads = crafted_lines(off, part, 100 * k + len(rows))
    want_plain = G.gaf_of(us, k, heads, [r.read for r in part], [(r.status, r.path) for r in part])[0].encode("latin-1")
    assert plain == want_plain and b"cs:Z:" not in plain
    al.gaf_cs_enable(False)
    assert crafted_lines(al, part, 100 * k + len(rows))[0] == plain
    # tagged, and through the write launch of a second fetch
    al.gaf_cs_enable()
    al.haplotag_enable(table)
    got_p, _, _, heads = crafted_lines(al, part, 100 * k + len(rows))
    want = lines_ref(us, k, heads, part, table)
    assert got_p == want and want.count(b"\tPS:i:") > 100
    assert crafted_lines(al, part, 100 * k + len(rows), paths_cap=1000)[0] == want   # BGR_E_CAPACITY, then bgr_aligner_fetch_text
    al.close()
    off.close()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("k", KS)
def test_crafted_rows_that_spell_no_walk_end_the_stream(k, where):
    """as without the field: irregular == 2 and no stream bytes, the break in the first pass of sixteen unitigs and in a later one"""
    w = world(k)
    g = B.Graph.build(k, *pack(w["us"][1:]))
    al = B.Aligner(g, 0)
    al.gaf_cs_enable()
    for bad in w["bad"]:
        rows = [Row(r.tag, r.status, r.path, r.read) for r in w["rows"][:40]]
        rows.insert({"first": 0, "middle": 20, "last": 40}[where], Row(bad.tag, bad.status, bad.path, bad.read))
        got_p, got_n, info, _ = crafted_lines(al, rows, 7 * k)
        assert info["irregular"] and info.get("no_walk") and got_p == b"" and got_n == b"", (k, where)
    good = [Row(r.tag, r.status, r.path, r.read) for r in w["rows"][:40]]   # the next call on that aligner is an ordinary one
    got_p, _, info, heads = crafted_lines(al, good, 7 * k)
    assert not info["irregular"] and got_p == lines_ref(w["us"], k, heads, good)
    al.close()


def diffs_ref(us, k, rows, seen=None):
    """-> (offsets, entries) of bgr_aligner_path_diffs over the rows (seen: the (status, path) every reader must take them for)"""
    offs, out = [0], []
    for i, r in enumerate(rows):
        st, path = seen[i] if seen is not None else (r.status, r.path)
        out += CS.path_diff_rows(us, k, r.read, st, path)
        offs.append(len(out))
    return offs, out


def check_diffs(al, us, k, rows, d_r, d_o, seen=None):
    n = len(rows)
    stats = al.path_stats(d_r.data_ptr(), d_o.data_ptr(), n)
    offs, out = al.path_diffs(d_r.data_ptr(), d_o.data_ptr(), n)
    want_offs, want = diffs_ref(us, k, rows, seen)
    assert offs.tolist() == want_offs, k
    assert [(int(x["read_pos"]), int(x["path_base"]), int(x["read_base"])) for x in out] == want and not out["reserved"].any()
    counts = np.diff(offs.astype(np.int64))
    nm = stats["mismatches"].astype(np.int64)
    assert np.array_equal(counts, np.where(nm == B.PATH_STAT_NO_WALK, 0, nm))   # as many entries as path stats counts mismatches
    return len(want)


@pytest.mark.parametrize("k", KS)
def test_path_diffs_over_crafted_rows(k):
    """the rows of the text test and those of test_gpu_crafted_rows.py (flipped signs, ids outside the graph, paths that spell no walk, two reads on
    one row) through bgr_align_device + bgr_aligner_device_results: offsets and entries what gaf_cs_ref says, the counts bgr_aligner_path_stats's"""
    w, c0 = world(k), crafted(k)
    us = w["us"]
    g = B.Graph.build(k, *pack(us[1:]))
    al = B.Aligner(g, 0)
    rows = w["rows"] + w["bad"]
    for n in LAUNCHES + (len(rows),):
        part = [Row(r.tag, r.status, r.path, r.read) for r in rows[len(rows) - n:]]
        rb, ro = pack([r.read for r in part])
        d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
        al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(ro[-1]), max(len(r.read) for r in part), m=2, effort=2)
        upload_rows(al, place(part, 31 * k + n))
        total = check_diffs(al, us, k, part, d_r, d_o)
        d_r.free()
        d_o.free()
    assert total > 1000
    # the capacity protocol
    rb, ro = pack([r.read for r in rows])
    d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), len(rows), int(ro[-1]), max(len(r.read) for r in rows), m=2, effort=2)
    upload_rows(al, place([Row(r.tag, r.status, r.path, r.read) for r in rows], 5))
    offs, nn = np.zeros(len(rows) + 1, dtype=np.uint64), B.C.c_uint64(0)
    small = np.zeros(total - 1, dtype=B.PATH_DIFF_DTYPE)
    small.view(np.uint8)[:] = 0xAB
    rc_ = B.lib().bgr_aligner_path_diffs(al.h, d_r.data_ptr(), d_o.data_ptr(), len(rows), offs.ctypes.data, small.ctypes.data, total - 1, B.C.byref(nn))
    assert rc_ == -4 and nn.value == total and int(offs[-1]) == total and (small["read_pos"] == 0xABABABAB).all()
    with pytest.raises(B.BgrError, match="error -1.*n_reads"):
        al.path_diffs(d_r.data_ptr(), d_o.data_ptr(), len(rows) - 1)
    d_r.free()
    d_o.free()
    # the other crafted set: its own graph
    g2 = B.Graph.build(k, *pack(c0["us"][1:]))
    al2 = B.Aligner(g2, 0)
    rb, ro = pack([r.read for r in c0["rows"]])
    d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
    al2.align_device(d_r.data_ptr(), d_o.data_ptr(), len(c0["rows"]), int(ro[-1]), max(len(r.read) for r in c0["rows"]), m=2, effort=2)
    upload_rows(al2, c0)
    assert check_diffs(al2, c0["us"], k, c0["rows"], d_r, d_o) > 300
    d_r.free()
    d_o.free()
    al.close()
    al2.close()


@pytest.mark.parametrize("k", KS)
def test_path_diffs_rows_at_across_and_behind_the_arenas_end(k):
    """test_gpu_crafted_row_routes.outside_rows: a row that ends on the arena's last int has its differences, one that does not lie wholly inside
    the arena has none (the allocation reaches beyond: a launch of three times the reads comes first)"""
    r0 = outside_rows(k)
    rows, us = r0["rows"], r0["us"]
    reads = [r.read for r in rows]
    g = B.Graph.build(k, *pack(us[1:]))
    al = B.Aligner(g, 0)
    rb, ro = pack(reads)
    rb3, ro3 = pack(reads * 3)
    d_r, d_o, d_r3, d_o3 = (B.DeviceBuffer(0, x) for x in (rb, ro, rb3, ro3))
    al.align_device(d_r3.data_ptr(), d_o3.data_ptr(), 3 * len(rows), int(ro3[-1]), max(len(x) for x in reads), m=2, effort=2)
    al.sync()
    big = al.arena_ints()
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), len(rows), int(ro[-1]), max(len(x) for x in reads), m=2, effort=2)
    al.sync()
    c = arrays_behind(al, k, big)
    d_results, d_arena, _ = al.device_results()
    B.device_upload(0, d_results, c["results"])
    B.device_upload(0, d_arena, c["arena"])
    check_diffs(al, us, k, rows, d_r, d_o, seen=r0["seen"])
    for x in (d_r, d_o, d_r3, d_o3):
        x.free()
    al.close()


# ---- mapper rows --------------------------------------------------------------------------------------------------------------------------------
def run_inputs(k, tmp):
    """a seeded Synth graph, a few thousand reads with up to three substitutions, every second one on its reverse complement, some with an N; as FASTA
    and FASTQ files, with a blocks file -> dict"""
    s = Synth(60000, max(40, 2 * k), 2, k, 700 + k)
    seqs, offs = s.unitigs()
    us = [""] + strings(seqs, offs)
    reads = []
    for L, n in ((k + 1, 30), (150, 2500), (251, 300), (1000, 40), (5000, 4)):
        rb, ro = s.reads(0, n, L, 3, 13 * k + L)
        reads += strings(rb, ro)
    rnd = random.Random(k)
    reads = [W.reverse_complements(r) if i % 2 else r for i, r in enumerate(reads)]
    for i in range(0, len(reads), 9):
        r = list(reads[i])
        r[rnd.randrange(len(r))] = "N"
        reads[i] = "".join(r)
    rnd.shuffle(reads)
    heads = ["r%d" % i + (" pair/1" if i % 3 == 0 else "\tx" if i % 5 == 0 else "") for i in range(len(reads))]
    uf, rf, qf, bf = (os.path.join(tmp, x) for x in ("u.fa", "r.fa", "r.fq", "blocks.tsv"))
    with open(uf, "w") as f:
        f.write("".join(">%d\n%s\n" % (i, u) for i, u in enumerate(us[1:])))
    with open(rf, "w") as f:
        f.write("".join(">%s\n%s\n" % (h, r) for h, r in zip(heads, reads)))
    with open(qf, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (h, r, "I" * len(r)) for h, r in zip(heads, reads)))
    n_unitigs = len(us) - 1
    ids = list(range(1, n_unitigs + 1))
    rnd.shuffle(ids)
    ids = ids[:2 * (n_unitigs // 3)]
    import blocks_ref as BR
    data = (BR.HEADER + "".join("%d\t0\t1\t1\t1\t2\t%d\t%d\t+\t.\n" % (1 + i % 12, ids[2 * i] * rnd.choice((1, -1)), ids[2 * i + 1] * rnd.choice((1, -1))) for i in range(len(ids) // 2))).encode()
    open(bf, "wb").write(data)
    table = H.table_of_file(data, n_unitigs)
    g = B.Graph.build(k, seqs, offs)
    ga = B.Graph.build(k, seqs, offs, anchors=True) if k <= 32 else None
    al = B.Aligner(g, 0)
    rows = W.rows_of(*al.align(*pack(reads), m=2, effort=2))
    al.close()
    return dict(k=k, g=g, ga=ga, us=us, heads=heads, reads=reads, rows=rows, table=table, uf=uf, rf=rf, qf=qf, bf=bf, args=["-k", str(k), "-g", uf, "-m", "2", "-e", "2", "--gaf"])


@pytest.fixture(scope="module", params=[31, 48], ids=["k31", "k48"])
def inputs(request, tmp_path_factory):
    return run_inputs(request.param, str(tmp_path_factory.mktemp("gaf_cs")))


def want_of(c, rows, fastq=False, tagged=False):
    heads = [("@" if fastq else ">") + h for h in c["heads"]]
    tag = (lambda line, path: H.tagged_line(line, H.tag_of(c["table"], path))) if tagged else None
    text, bug = CS.gaf_cs_of(c["us"], c["k"], heads, c["reads"], rows, tag)
    assert bug is None
    return text.encode("latin-1")


def test_the_mapper_rows_have_lines_of_every_kind(inputs):
    c = inputs
    by_nm = {0: 0, 1: 0, 2: 0}
    for i, (st, path) in enumerate(c["rows"]):
        if path:
            s = G.stats(c["us"], c["k"], c["reads"][i], st, path)
            CS.check_invariants(c["us"], c["k"], c["reads"][i], s, CS.cs_of(c["reads"][i], s))
            by_nm[min(2, s["nm"])] += 1
    # (reads with 0 .. 3 substitutions at -m 2: those with three cannot map, the others do where their anchors allow -- more than half of all; the
    # kinds of lines: what the issue asks for, at least one of each)
    assert sum(by_nm.values()) > len(c["reads"]) // 2 and min(by_nm.values()) > 0 and any(st & W.ST_RC for st, p in c["rows"] if p), by_nm
    assert b"*an" in want_of(c, c["rows"]) or b"*cn" in want_of(c, c["rows"])


@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "tagged"])
@pytest.mark.parametrize("extra", ROUTES, ids=ROUTE_IDS)
def test_cli_run_bytes(inputs, extra, tagged):
    """--gaf --cs on every route, with and without --haplotag: the definition's bytes; the device route and --host-route agree through it"""
    c = inputs
    more = ["--cs"] + (["--haplotag", c["bf"]] if tagged else [])
    on = run(["-r", c["rf"]] + c["args"] + extra, flags=(), more=more)
    assert on["paths"] == want_of(c, c["rows"], tagged=tagged), (c["k"], extra)
    if not extra and not tagged:   # notAligned.fa, the counters and stdout are those of the run without the flag, which writes today's bytes
        off = run(["-r", c["rf"]] + c["args"], flags=())
        assert off["paths"] == G.gaf_of(c["us"], c["k"], [">" + h for h in c["heads"]], c["reads"], c["rows"])[0].encode("latin-1")
        assert on["na"] == off["na"]
        strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
        assert strip(on["out"]) == strip(off["out"])


@pytest.mark.parametrize("extra", [[], ["--host-route"]], ids=["device", "host"])
def test_cli_fastq_and_anchors(inputs, extra):
    c = inputs
    # -q: which records a FASTQ file has is the parser's business (it keeps the reference's quirks), so the lines are checked one by one: without
    # their last field they are the bytes of the run without --cs, and the field is the definition's for the line's read and intervals
    off = run(["-r", c["qf"], "-q"] + c["args"] + extra, flags=(), more=["--haplotag", c["bf"]])
    on = run(["-r", c["qf"], "-q"] + c["args"] + extra, flags=(), more=["--cs", "--haplotag", c["bf"]])
    reads = dict(zip((h.split(" ")[0].split("\t")[0] for h in c["heads"]), c["reads"]))
    lines = [ln.rpartition("\tcs:Z:") for ln in on["paths"].decode().split("\n")[:-1]]
    assert "".join(base + "\n" for base, _, _ in lines).encode() == off["paths"] and b"\tPS:i:" in off["paths"] and on["na"] == off["na"]
    phantom = 0
    for base, _, ops in lines:
        f = G.parse_line("\t".join(base.split("\t")[:13]) + "\n")
        if f["name"] == "*":   # (the reference's phantom record behind a FASTQ file's last one: no header to find its read by)
            phantom += 1
            continue
        walk, read = G.spell(c["us"], c["k"], f["segments"]), reads[f["name"]]
        assert ops == CS.ops_of(walk[f["pstart"]:f["pend"]], read[f["qstart"]:f["qend"]]), base
    assert len(lines) > len(c["reads"]) // 2 and any("*" in o for _, _, o in lines) and phantom <= 1
    if c["ga"] is not None:   # -G: other rows (the anchors mode's), the same definition
        al = B.Aligner(c["ga"], 0)
        rows = W.rows_of(*al.align(*pack(c["reads"]), m=2, effort=2, mode=B.MODE_ANCHORS))
        al.close()
        on = run(["-r", c["rf"], "-G"] + c["args"] + extra, flags=(), more=["--cs"])
        assert on["paths"] == want_of(c, rows) and on["paths"].count(b"\n") > len(c["reads"]) // 2


@pytest.mark.parametrize("route", [0, 1], ids=["text", "host"])
def test_align_all_with_the_graphs_switch(inputs, route, tmp_path):
    c = inputs
    g = c["g"]
    PF, NF = str(tmp_path / "p"), str(tmp_path / "n")
    B.align_all(g, c["rf"], PF, NF, m=2, effort=2, route=route, gaf=True)
    before = open(PF, "rb").read()
    g.gaf_cs_enable()
    try:
        with pytest.raises(B.BgrError, match="error -1.*gaf"):
            B.align_all(g, c["rf"], PF, NF, m=2, effort=2, route=route)
        B.align_all(g, c["rf"], PF, NF, m=2, effort=2, route=route, gaf=True, threads=3)
        assert open(PF, "rb").read() == want_of(c, c["rows"])
    finally:
        g.gaf_cs_enable(False)
    B.align_all(g, c["rf"], PF, NF, m=2, effort=2, route=route, gaf=True)
    assert open(PF, "rb").read() == before and b"cs:Z:" not in before   # the flag off: the bytes of the same run without it


def test_cli_refusals(inputs, tmp_path):
    c = inputs
    base = [B.CLI_PATH, "-r", c["rf"], "-k", str(c["k"]), "-g", c["uf"]]
    for extra, msg in ((["--cs"], "--gaf"), (["--cs", "--gaf", "-b"], "-b"), (["--cs", "--gaf", "-c"], "-c")):
        pr = subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert pr.returncode == 2 and msg in pr.stderr, (extra, pr.returncode, pr.stderr[-500:])
    assert not os.path.exists(tmp_path / "paths")


def test_cli_round_trip_from_gfa_and_gaf(inputs):
    """one run writes --gfa and --gaf --cs: the unitigs of the GFA file, glued along every line's segments, cut to its path interval and changed by
    its ops, give back the aligned part of every mapped read"""
    c = inputs
    r = run(["-r", c["rf"]] + c["args"], flags=("gfa",), more=["--cs"])
    segs = {}
    for ln in r["gfa"].decode().split("\n"):
        f = ln.split("\t")
        if f[0] == "S":
            segs[int(f[1])] = f[2]
    us = [""] + [segs[i] for i in range(1, len(segs) + 1)]
    reads = dict(zip((h.split(" ")[0].split("\t")[0] for h in c["heads"]), c["reads"]))
    n = 0
    for ln in r["paths"].decode().split("\n")[:-1]:
        line, _, ops = ln.rpartition("\tcs:Z:")
        f = G.parse_line(line + "\n")
        walk = G.spell(us, c["k"], f["segments"])
        read = reads[f["name"]]
        assert len(walk) == f["plen"]
        assert CS.apply_ops(ops, walk[f["pstart"]:f["pend"]]) == "".join(x if x in "ACGT" else "n" for x in read[f["qstart"]:f["qend"]]), ln
        assert ops.count("*") == f["nm"]
        n += 1
    assert n == sum(1 for _, p in c["rows"] if p) > len(c["reads"]) // 2
