"""The paths of exhaustive launches as output (--exhaustive-paths, bgr_aligner_exhaustive_paths_enable, bgr_graph_exhaustive_paths_enable) on the GPU:
what is counted and formatted behind an exhaustive launch equals the plain-Python definitions of the greedy modes (abundance_ref, links_ref,
triples_ref, pileup_ref, strands_ref, gaf_ref, gaf_cs_ref, haplotag_ref) fed with the oracle's exhaustive rows (Oracle.align(mode=1)) minus their last
int (exhaustive_rows_ref).  Batch API with two launches and both LDS forms, a launch that has to be settled, the readers of the last launch's rows,
the view rule on rows the mapper never writes, the text route, and the command line end to end with every new refusal."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import abundance_ref as A
import bgreat_amd as B
import bubbles_ref as BR
import exhaustive_rows_ref as X
import gaf_cs_ref as CS
import gaf_ref as G
import haplotag_ref as H
import links_ref as K
import oracle_py
import pileup_ref as P
import strands_ref as S
import triples_ref as T
import wide_greedy_ref as W
from tools.synth import Synth
from util import GOLD

pytestmark = pytest.mark.gpu

EXH = B.MODE_EXHAUSTIVE


def strings(buf, offs):
    return [bytes(buf[int(offs[i]):int(offs[i + 1])]).decode("latin-1") for i in range(len(offs) - 1)]


def pack(strs):
    offs = np.zeros(len(strs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in strs])
    return np.frombuffer("".join(strs).encode("latin-1"), dtype=np.uint8).copy(), offs


@functools.lru_cache(maxsize=None)
def workload(name):
    """-> dict(k, m, us ("" at 0), seqs, offs, reads (str), rb, ro, rows (the oracle's exhaustive rows), view (without their last int)), computed once"""
    if name == "deg":   # the k = 5 degenerate golden: the first 400 reads, m = 5
        k, m = 5, 5
        us = G.load_unitigs(os.path.join(GOLD, "deg_unitig.fa"), k)
        reads, roffs, _, _ = oracle_py.parse_file(os.path.join(GOLD, "deg_reads.fa"), k)
        reads = strings(reads, roffs)[:400]
    else:
        k = 31
        if name == "default":   # the default graph's shape, small: 150 bp reads, m = 2
            s, m = Synth(20000, 75, 2, 31, 11), 2
            reads = strings(*s.reads(0, 300, 150, 2, 12))
        else:                   # the branchy workload, small: 250 bp reads and -- for paths of more than sixteen unitigs -- 400 bp reads, m = 5
            s, m = Synth(20000, 36, 4, 31, 12), 5
            reads = strings(*s.reads(0, 150, 250, 5, 13)) + strings(*s.reads(150, 100, 400, 5, 14))
        us = [""] + strings(*s.unitigs())
    seqs, offs = pack(us[1:])
    rb, ro = pack(reads)
    rows = W.rows_of(*oracle_py.Oracle(k, seqs, offs).align(rb, ro, m=m, mode=1))
    return dict(k=k, m=m, us=us, seqs=seqs, offs=offs, reads=reads, rb=rb, ro=ro, rows=rows, view=X.view_rows(rows))


def counting_aligner(g, form=0, strands=True):
    al = B.Aligner(g, 0)
    al.exhaustive_paths_enable()
    al.set_knob(B.KNOB_ABUNDANCE_FORM, form)
    al.set_knob(B.KNOB_LINKS_FORM, form)
    al.abundance_enable()
    al.links_enable()
    al.triples_enable()
    if strands:
        al.pileup_strands_enable()
    else:
        al.pileup_enable()
    return al


def flat_of(arr):
    return np.stack([arr[f] for f in B.PILEUP_DTYPE.names], axis=1).astype(np.int64)


def check_tables(al, w, view, times=1, strands=True):
    """the aligner's four tables = the definitions over the view rows, each read counted `times` times"""
    us, k, reads = w["us"], w["k"], w["reads"][:len(view)]
    lens = A.unitig_lens(us)
    want = np.array(A.abundance_of(lens, k, [len(r) for r in reads], view)[1:], dtype=np.uint64)
    assert np.array_equal(al.abundance(), times * want)
    links = [(int(x["from"]), int(x["to"]), int(x["count"])) for x in al.links()]
    assert links == [(a, b, times * c) for a, b, c in K.sorted_links(K.links_of(view, len(us) - 1))] and al.links_info()["overflow"] == 0
    trip = T.as_tuples(al.triples())
    assert trip == [t[:3] + (times * t[3],) for t in T.sorted_triples(T.triples_of(view, len(us) - 1))]
    p = P.pileup_of(us, k, reads, view)
    table, skipped = al.pileup()
    assert skipped == times * p.skipped == 0 and np.array_equal(flat_of(table), times * p.flat()) and p.flat().any()
    if strands:
        f = S.forward_of(us, k, reads, view)
        assert np.array_equal(flat_of(al.pileup_forward()), times * f.flat())


def test_the_workloads_hold_every_kind_of_row():
    """from the oracle alone: rows that begin [0, ..], rows that end in 0, paths of more than sixteen unitigs (the walk's later passes) -- and links, triples"""
    n = dict(begin0=0, end0=0, long=0, mapped=0, unmapped=0)
    for name in ("default", "branchy", "deg"):
        w = workload(name)
        assert 50 <= len(w["reads"]) <= 400 and len(w["us"]) < 5000
        for (st, p), (vst, v) in zip(w["rows"], w["view"]):
            n["unmapped"] += not p
            if p:
                assert st == vst == W.ST_ALIGNED and len(p) >= 3 and v == p[:-1]
                n["mapped"] += 1
                n["begin0"] += p[0] == 0
                n["end0"] += p[-1] == 0
                n["long"] += len(v) - 1 > 16
    assert n["begin0"] >= 5 and n["end0"] >= 2 and n["long"] >= 20 and n["mapped"] >= 500 and n["unmapped"] >= 1, n
    assert max(len(v) - 1 for _, v in workload("branchy")["view"]) > 16 and any(p and p[-1] == 0 for _, p in workload("deg")["rows"])


@pytest.mark.parametrize("form", [1, 2], ids=["formA", "formB"])
@pytest.mark.parametrize("name", ["default", "branchy", "deg"])
def test_counting_behind_exhaustive_launches(name, form):
    """abundance, links, triples and the pileup with strands, summed over two launches of the batch API, in both LDS forms; what the launches return stays
    the reference's rows with the end offset"""
    w = workload(name)
    g = B.Graph.build(w["k"], w["seqs"], w["offs"])
    al = counting_aligner(g, form)
    n = len(w["reads"])
    assert al.abundance_plan(n // 2, int(w["ro"][n // 2]))["form"] == form and al.links_plan(n // 2)["form"] == form
    got = []
    for lo, hi in ((0, n // 2), (n // 2, n)):
        rb, ro = pack(w["reads"][lo:hi])
        got += W.rows_of(*al.align(rb, ro, m=w["m"], mode=EXH))
    assert got == w["rows"]
    check_tables(al, w, w["view"])
    al.close()


def test_with_the_switch_off_nothing_changes():
    """the refusals keep their words, and an aligner that has the switch taken away again refuses as before"""
    w = workload("default")
    g = B.Graph.build(w["k"], w["seqs"], w["offs"])
    al = B.Aligner(g, 0)
    al.abundance_enable()
    with pytest.raises(B.BgrError, match="error -1.*counts unitig abundance.*exhaustive mode \\(-b\\) is refused"):
        al.align(w["rb"], w["ro"], m=2, mode=EXH)
    al.exhaustive_paths_enable()
    assert W.rows_of(*al.align(w["rb"], w["ro"], m=2, mode=EXH)) == w["rows"]
    assert np.array_equal(al.abundance(), np.array(A.abundance_of(A.unitig_lens(w["us"]), 31, [len(r) for r in w["reads"]], w["view"])[1:], dtype=np.uint64))
    al.exhaustive_paths_enable(False)
    with pytest.raises(B.BgrError, match="error -1.*exhaustive mode \\(-b\\) is refused"):
        al.align(w["rb"], w["ro"], m=2, mode=EXH)
    al.abundance_enable(False)
    d_r, d_o = B.DeviceBuffer(0, w["rb"]), B.DeviceBuffer(0, w["ro"])
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), len(w["reads"]), int(w["ro"][-1]), 150, m=2, mode=EXH)
    with pytest.raises(B.BgrError, match="error -1.*the last launch was exhaustive; paths of the greedy modes only"):
        al.path_stats(d_r.data_ptr(), d_o.data_ptr(), len(w["reads"]))
    with pytest.raises(B.BgrError, match="error -1.*bgr_aligner_device_rows_view"):
        al.device_rows_view()
    al.exhaustive_paths_enable()
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), len(w["reads"]), int(w["ro"][-1]), 150, m=2)   # a greedy launch has no view
    with pytest.raises(B.BgrError, match="error -1.*bgr_aligner_device_rows_view"):
        al.device_rows_view()
    g.inside_build()
    al.inside_enable()
    with pytest.raises(B.BgrError, match="error -1.*inside pass.*exhaustive mode \\(-b\\) is refused"):   # the inside pass writes greedy rows
        al.align(w["rb"], w["ro"], m=2, mode=EXH)
    al.sync()
    d_r.free()
    d_o.free()
    al.close()


def settling(al):
    """the knobs under which the last pass of a launch on the branchy graph hands most of its reads back (test_gpu_parity: a table of 8 entries)"""
    al.set_knob(B.KNOB_EXH_FAST, 1)
    al.set_knob(B.KNOB_EXH_FRAME_CAP, 3)
    al.set_knob(B.KNOB_EXH_MEMO_CAP, 8)


def test_a_launch_that_has_to_be_settled_is_counted_once():
    """the last pass hands reads back: the tables equal the definition, every read counted once; and a second launch with no wait in between -- the first
    one is settled and counted by it -- loses nothing"""
    w = workload("branchy")
    g = B.Graph.build(w["k"], w["seqs"], w["offs"])
    al = counting_aligner(g)
    settling(al)
    n, total, longest = len(w["reads"]), int(w["ro"][-1]), max(len(r) for r in w["reads"])
    d_r, d_o = B.DeviceBuffer(0, w["rb"]), B.DeviceBuffer(0, w["ro"])
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, total, longest, m=w["m"], mode=EXH)
    check_tables(al, w, w["view"])   # (reading a table settles and counts the launch)
    assert al.last_pass_runs()[0] >= 2   # reads were handed back
    assert W.rows_of(*al.fetch(n, total + 8 * n)) == w["rows"]
    check_tables(al, w, w["view"])   # (a fetch behind it counts nothing again)
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, total, longest, m=w["m"], mode=EXH)
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, total, longest, m=w["m"], mode=EXH)
    assert al.counters()["reads"] == 3 * n
    check_tables(al, w, w["view"], times=3)
    d_r.free()
    d_o.free()
    al.close()


def test_the_view_kernel_has_a_slot_of_its_own_in_the_kernel_times():
    """the kernels behind the settling are timed as kernels of their launch: the host's wait, the view kernel, the counting kernels -- asking for the
    times settles and counts a launch in flight; with the switch off the slots are those of the passes alone"""
    w = workload("default")
    g = B.Graph.build(w["k"], w["seqs"], w["offs"])
    n = len(w["reads"])
    d_r, d_o = B.DeviceBuffer(0, w["rb"]), B.DeviceBuffer(0, w["ro"])
    al = B.Aligner(g, 0)
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(w["ro"][-1]), 150, m=w["m"], mode=EXH)
    launches, passes = al.kernel_times()
    assert launches == 1 and all(name.startswith("bgr_align_exhaustive") for name, _ in passes) and len(passes) >= 2
    al.close()
    al = B.Aligner(g, 0)
    al.exhaustive_paths_enable()
    al.abundance_enable()
    al.triples_enable()
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(w["ro"][-1]), 150, m=w["m"], mode=EXH)
    launches, slots = al.kernel_times()
    names = [name for name, _ in slots]
    assert launches == 1 and names[:len(passes)] == [name for name, _ in passes]
    assert names[len(passes):] == ["settle_launch (host)", "bgr_exhaustive_rows_kernel", "bgr_abundance_kernel", "bgr_triples_kernel"], names
    assert all(ms > 0 for _, ms in slots)
    check = np.array(A.abundance_of(A.unitig_lens(w["us"]), w["k"], [len(r) for r in w["reads"]], w["view"])[1:], dtype=np.uint64)
    assert np.array_equal(al.abundance(), check)
    d_r.free()
    d_o.free()
    al.close()


def test_readers_of_the_last_launch_take_the_view():
    """path_stats, path_diffs and haplotags behind an exhaustive launch = the definitions over the view; the whole read is aligned; the stored end offset
    (bgr_aligner_fetch) follows from the stats; bgr_aligner_device_rows_view is the rule over the device's result words"""
    for name in ("default", "branchy"):
        w = workload(name)
        us, k, reads, n = w["us"], w["k"], w["reads"], len(w["reads"])
        g = B.Graph.build(k, w["seqs"], w["offs"])
        al = B.Aligner(g, 0)
        al.exhaustive_paths_enable()
        rng = np.random.default_rng(5)
        table = np.zeros(len(us), dtype=np.uint32)
        tagged = rng.choice(np.arange(1, len(us)), size=len(us) // 3, replace=False)
        table[tagged] = rng.integers(2, 40, size=len(tagged))
        al.haplotag_enable(table)
        d_r, d_o = B.DeviceBuffer(0, w["rb"]), B.DeviceBuffer(0, w["ro"])
        al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(w["ro"][-1]), max(len(r) for r in reads), m=w["m"], mode=EXH)
        stats = al.path_stats(d_r.data_ptr(), d_o.data_ptr(), n)
        offs, diffs = al.path_diffs(d_r.data_ptr(), d_o.data_ptr(), n)
        tags = al.haplotags(n)
        fetched = W.rows_of(*al.fetch(n, int(w["ro"][-1]) + 8 * n))
        assert fetched == w["rows"]
        want_diffs, want_offs = [], [0]
        for i, ((st, v), (_, full)) in enumerate(zip(w["view"], fetched)):
            want = G.path_stat_row(us, k, reads[i], st, v)
            assert tuple(int(x) for x in stats[i]) == want, (name, i)
            assert tuple(int(x) for x in tags[i]) == H.tag_of(table.tolist(), v), (name, i)
            want_diffs += CS.path_diff_rows(us, k, reads[i], st, v)
            want_offs.append(len(want_diffs))
            if v:
                assert want[2] == len(reads[i])   # aligned = the read's length
                if "N" not in reads[i]:
                    assert want[3] <= w["m"]
                # the end offset the fetch delivers, from the stats: begin + L - (walk - last unitig), or 0 where that is the last unitig's length
                last = len(us[abs(v[-1])])
                e = int(stats[i]["path_start"]) + int(stats[i]["aligned"]) - (int(stats[i]["path_len"]) - last)
                assert full[-1] == e or (full[-1] == 0 and e == last), (name, i)
                assert full[-1] in X.end_offsets(us, k, len(reads[i]), v)
        assert offs.tolist() == want_offs and [(int(x["read_pos"]), int(x["path_base"]), int(x["read_base"])) for x in diffs] == want_diffs and len(want_diffs) > 0
        assert tags["block"].any()
        d_results, _, _ = al.device_results()
        res = B.device_download(0, d_results, 2 * n, np.uint32).reshape(n, 2)
        view = B.device_download(0, al.device_rows_view(), 2 * n, np.uint32).reshape(n, 2)
        ints = al.arena_ints()
        assert [tuple(int(x) for x in r) for r in view] == [X.view_word(int(o), int(x), ints) for o, x in res]
        assert [int(x) & 0xFFFFFF for x in view[:, 1]] == [len(v) for _, v in w["view"]]
        d_r.free()
        d_o.free()
        al.close()


def test_the_view_rule_on_rows_the_mapper_never_writes():
    """rows of 0, 1, 2 and 3 ints, rows with a status other than aligned and n > 0, spare bits in the status byte, rows at, across and behind the arena's end:
    written over a launch's results (option test.keep_rows, as tests/test_gpu_crafted_row_routes.py), the view and the counted tables follow
    exhaustive_rows_ref"""
    w = workload("default")
    us, k, reads, n = w["us"], w["k"], w["reads"], len(w["reads"])
    g = B.Graph.build(k, w["seqs"], w["offs"])
    al = counting_aligner(g)
    d_r, d_o = B.DeviceBuffer(0, w["rb"]), B.DeviceBuffer(0, w["ro"])
    launch = lambda: al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(w["ro"][-1]), 150, m=w["m"], mode=EXH)
    launch()
    al.sync()
    for reset in (al.reset_abundance, al.reset_links, al.reset_triples, al.reset_pileup):
        reset()
    bound = al.arena_ints()
    assert bound >= 2 * (int(w["ro"][-1]) + 8 * n)
    mapped = [i for i, (_, p) in enumerate(w["rows"]) if len(p) >= 4]
    assert len(mapped) >= 200
    results = np.zeros((n, 2), dtype=np.uint32)
    arena = np.full(4096 + sum(len(p) for _, p in w["rows"]), 0x5A5A5A5A, dtype=np.int32)
    crafted, at = {}, 0
    for j, i in enumerate(mapped):
        st, p = w["rows"][i]
        kind = j % 12 if j % 12 != 7 or j == 7 else 11     # (one row ends on the arena's last int)
        if kind < 4:
            p = p[:kind]                                   # 0, 1, 2 and 3 ints, the status aligned
        elif kind == 4:
            st = W.ST_FAILED                               # not aligned, n > 0
        elif kind == 5:
            st = W.ST_NOANCHOR
        elif kind == 6:
            st = W.ST_ALIGNED | 0x50                       # spare bits of the status byte travel with the row
        crafted[i] = (st, p, kind)
    for i in range(n):
        if i not in crafted:
            results[i] = (0x7FFFFFF0, W.ST_NOANCHOR << 24 if not w["rows"][i][1] else W.ST_FAILED << 24)   # empty rows: the offset is never followed
            continue
        st, p, kind = crafted[i]
        if kind == 7:
            off = bound - len(p)            # ends on the arena's last int
        elif kind == 8:
            off = bound - len(p) + 1        # one int across the end
        elif kind == 9:
            off = bound + 5                 # behind the end
        elif kind == 10:
            off = 0xFFFFFFF0                # the 32-bit sum wraps: it is taken in 64 bits
        else:
            off = at
            arena[at:at + len(p)] = p
            at += len(p) + 1
        results[i] = (off, len(p) | (st << 24))
    ends = [i for i in crafted if crafted[i][2] == 7]
    assert len(ends) == 1 and at < len(arena)
    tail = crafted[ends[0]][1]
    d_results, d_arena, _ = al.device_results()
    B.device_upload(0, d_results, results)
    B.device_upload(0, d_arena, arena[:at])
    B.device_upload(0, d_arena + 4 * (bound - len(tail)), np.array(tail, dtype=np.int32))
    with B.options(**{"test.keep_rows": 1}):
        launch()   # everything of the launch but its mapping passes: the counting kernels behind it, over the view of these rows
        view = B.device_download(0, al.device_rows_view(), 2 * n, np.uint32).reshape(n, 2)
    assert [tuple(int(x) for x in r) for r in view] == [X.view_word(int(o), int(x), bound) for o, x in results]
    seen, kinds = [], {}
    for i in range(n):
        off, x = int(view[i][0]), int(view[i][1])
        np_ = x & 0xFFFFFF
        if np_ == 0:
            seen.append((x >> 24, []))
            continue
        assert i in crafted
        kind = crafted[i][2]
        kinds[kind] = kinds.get(kind, 0) + 1
        if kind == 7:
            assert off + np_ + 1 == bound
        seen.append((x >> 24, crafted[i][1][:np_]))
    assert set(kinds) == {3, 6, 7, 11} and kinds[7] == 1 and all(kinds[x] >= 10 for x in (3, 6, 11)), kinds   # rows of three ints and whole rows inside the arena: nothing else is read
    assert all(st == (W.ST_ALIGNED | 0x50) for i, (st, v) in enumerate(seen) if i in crafted and crafted[i][2] == 6 and v)
    us_reads = reads
    lens = A.unitig_lens(us)
    assert np.array_equal(al.abundance(), np.array(A.abundance_of(lens, k, [len(r) for r in us_reads], seen)[1:], dtype=np.uint64))
    assert [(int(x["from"]), int(x["to"]), int(x["count"])) for x in al.links()] == K.sorted_links(K.links_of(seen, len(us) - 1))
    assert T.as_tuples(al.triples()) == T.sorted_triples(T.triples_of(seen, len(us) - 1))
    p = P.pileup_of(us, k, us_reads, seen)
    table, skipped = al.pileup()
    assert skipped == p.skipped and np.array_equal(flat_of(table), p.flat())
    assert np.array_equal(flat_of(al.pileup_forward()), S.forward_of(us, k, us_reads, seen).flat())
    d_r.free()
    d_o.free()
    al.close()


def fasta_of(reads):
    heads = [">q%d some words" % i for i in range(len(reads))]
    return heads, "".join("%s\n%s\n" % (h, r) for h, r in zip(heads, reads)).encode("latin-1")


@pytest.mark.parametrize("cs", [False, True], ids=["plain", "cs"])
@pytest.mark.parametrize("tagged", [False, True], ids=["untagged", "tagged"])
def test_text_route_writes_gaf_lines_in_exhaustive_mode(cs, tagged):
    """align_fasta_text(mode=EXHAUSTIVE, want_output=3) = gaf_ref over the view rows, with cs:Z: and haplotags on and off; once with a staged piece and
    once behind a launch that had to be settled; the record info comes with it, and a counting aligner counts the piece once"""
    w = workload("branchy")
    us, k, reads = w["us"], w["k"], w["reads"]
    heads, text = fasta_of(reads)
    g = B.Graph.build(k, w["seqs"], w["offs"])
    table = np.zeros(len(us), dtype=np.uint32)
    table[1::3] = 2 + (np.arange(len(table[1::3])) % 7)
    tag = (lambda line, path: H.tagged_line(line, H.tag_of(table.tolist(), path))) if tagged else None
    if cs:
        want, bad = CS.gaf_cs_of(us, k, heads, reads, w["view"], tag)
    else:
        want, bad = G.gaf_of(us, k, heads, reads, w["view"])
        if tagged:
            lines = iter(want.splitlines(keepends=True))
            want = "".join(tag(next(lines), v) for _, v in w["view"] if v)
    assert bad is None and want.count("\n") == sum(1 for _, v in w["view"] if v)
    want_n = "".join("%s\n%s\n" % (h, r) for h, r, (_, v) in zip(heads, reads, w["view"]) if not v)
    want_info = np.array([0x80000000 | (0x40000000 if v else 0) | len(r) for r, (_, v) in zip(reads, w["view"])], dtype=np.uint32)
    for how in ("plain", "staged", "settled"):
        al = counting_aligner(g, strands=False) if how != "staged" else B.Aligner(g, 0)
        al.exhaustive_paths_enable()
        if tagged:
            al.haplotag_enable(table)
        al.gaf_cs_enable(cs)
        if how == "settled":
            settling(al)
        with B.options(poison_device_buffers=1):
            p, nn, info = al.align_fasta_text(text, m=w["m"], mode=EXH, want_output=3, staged=how == "staged", record_info=True)
        assert not info["irregular"] and info["n_accepted"] == len(reads), how
        assert p.decode("latin-1") == want and nn.decode("latin-1") == want_n, how
        assert np.array_equal(info["records"], want_info), how
        if how == "settled":
            assert al.last_pass_runs()[0] >= 2
        if how != "staged":
            check_tables(al, w, w["view"], strands=False)
        al.close()
    al = B.Aligner(g, 0)   # without the switch: refused as ever
    with pytest.raises(B.BgrError, match="error -1.*GAF output needs.*a greedy mode"):
        al.align_fasta_text(text, m=w["m"], mode=EXH, want_output=3)
    al.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
FLAGS = ("abundance", "gfa", "pileup", "triples", "bubbles")


def cli(args, flags=FLAGS, check=True):
    """-> (status, stdout, stderr, paths, notAligned.fa, {flag: file bytes or None})"""
    d = tempfile.mkdtemp()
    try:
        files = [x for f in flags for x in ("--" + f, os.path.join(d, "out." + f))]
        pr = subprocess.run([B.CLI_PATH] + list(args) + files, cwd=d, capture_output=True, text=True, timeout=300)
        if check and pr.returncode != 0:
            raise RuntimeError("%s failed (%d): %s" % (args, pr.returncode, pr.stderr[-2000:]))
        cat = lambda name: open(os.path.join(d, name), "rb").read() if os.path.exists(os.path.join(d, name)) else None
        return pr.returncode, pr.stdout, pr.stderr, cat("paths") or b"", cat("notAligned.fa") or b"", {f: cat("out." + f) for f in flags}
    finally:
        shutil.rmtree(d)


def stable(stdout):
    return [ln for ln in stdout.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]


@pytest.fixture(scope="module")
def cli_cases():
    """(args, k, m, unitigs, headers, reads, view rows) of two goldens and one synthetic pair"""
    d = tempfile.mkdtemp()
    out = []
    for rfile, ufile, k, m in (("deg_reads.fa", "deg_unitig.fa", 5, 5), ("syn_r250.fa", "syn_unitig.fa", 31, 5)):
        out.append((os.path.join(GOLD, rfile), os.path.join(GOLD, ufile), k, m))
    s = Synth(20000, 36, 4, 31, 12)
    s.write_unitigs(os.path.join(d, "u.fa"))
    s.write_reads(os.path.join(d, "r.fa"), 0, 300, 250, 5, 13)
    out.append((os.path.join(d, "r.fa"), os.path.join(d, "u.fa"), 31, 5))
    cases = []
    for rf, uf, k, m in out:
        us = G.load_unitigs(uf, k)
        rb, ro, hb, ho = oracle_py.parse_file(rf, k)
        rows = W.rows_of(*oracle_py.Oracle(k, fasta=uf).align(rb, ro, m=m, mode=1))
        cases.append((["-r", rf, "-k", str(k), "-g", uf, "-m", str(m), "-b"], k, m, us, strings(hb, ho), strings(rb, ro), X.view_rows(rows)))
    yield cases
    shutil.rmtree(d)


@pytest.mark.parametrize("extra", [[], ["--host-route"]], ids=["text", "host"])
def test_cli_end_to_end(cli_cases, extra):
    """-b --exhaustive-paths --gaf --cs with the counting files: every file = its definition over the view rows; notAligned.fa and stdout are those of
    -b --write-exhaustive; both routes write the same bytes"""
    for args, k, m, us, heads, reads, view in cli_cases:
        _, out0, _, _, na0, _ = cli(args + ["--write-exhaustive"] + extra, flags=())
        _, out, _, paths, na, f = cli(args + ["--exhaustive-paths", "--gaf", "--cs"] + extra)
        want, bad = CS.gaf_cs_of(us, k, heads, reads, view)
        assert bad is None and paths.decode("latin-1") == want and len(want) > 0, args
        assert na == na0 and stable(out) == stable(out0), args
        lens = A.unitig_lens(us)
        table = A.abundance_of(lens, k, [len(r) for r in reads], view)
        links = K.links_of(view, len(us) - 1)
        assert f["abundance"] == A.text_of(lens, table), args
        assert f["gfa"] == K.gfa_text(us, k, table, links), args
        assert f["pileup"] == P.sites_text_of(us, P.pileup_of(us, k, reads, view)), args
        assert f["triples"] == T.triples_text(T.triples_of(view, len(us) - 1)), args
        assert f["bubbles"] == BR.bubbles_text(us, BR.bubbles_of(links)), args
        # without --gaf the two files are what -b gives today: nothing, unless --write-exhaustive asks for the reference's records
        _, out1, _, paths1, na1, f1 = cli(args + ["--exhaustive-paths"] + extra, flags=("abundance",))
        assert paths1 == b"" and na1 == b"" and stable(out1) == stable(out0) and f1["abundance"] == f["abundance"], args
        _, _, _, paths2, na2, f2 = cli(args + ["--exhaustive-paths", "--write-exhaustive"] + extra, flags=("triples",))
        _, _, _, paths3, _, _ = cli(args + ["--write-exhaustive"] + extra, flags=())
        assert paths2 == paths3 and len(paths2) > 0 and na2 == na0 and f2["triples"] == f["triples"], args


def test_cli_refusals(cli_cases, tmp_path):
    args = cli_cases[0][0]
    greedy = [a for a in args if a != "-b"]
    for bad, word in ((greedy + ["--exhaustive-paths"], "-b"), (args + ["--exhaustive-paths", "-i"], "-i"), (args + ["--exhaustive-paths", "--inside"], "--inside"),
                      (args + ["--exhaustive-paths", "--gaf", "--write-exhaustive"], "--write-exhaustive")):
        rc, _, err, paths, na, f = cli(bad, flags=("abundance",), check=False)
        assert rc == 2 and "--exhaustive-paths" in err or "--gaf" in err, (bad, err[-300:])
        assert rc == 2 and word in err and f["abundance"] is None, (bad, err[-300:])
    # the same command lines without the flag end as they always did
    for more, words in ((["--gaf"], ("--gaf", "greedy modes", "exhaustive mode (-b) writes no paths")),
                        (["--gaf", "--cs"], ("--gaf", "exhaustive mode (-b) writes no paths")),
                        (["--abundance", str(tmp_path / "a")], ("--abundance", "the rows of exhaustive mode (-b) have another layout")),
                        (["--gfa", str(tmp_path / "g")], ("--gfa", "the rows of exhaustive mode (-b) have another layout")),
                        (["--pileup", str(tmp_path / "p")], ("--pileup", "the rows of exhaustive mode (-b) have another layout")),
                        (["--triples", str(tmp_path / "t")], ("--triples", "the rows of exhaustive mode (-b) have another layout")),
                        (["--bubbles", str(tmp_path / "b")], ("--bubbles", "the rows of exhaustive mode (-b) have another layout")),
                        (["--inside"], ("--inside", "exhaustive mode (-b) is refused"))):
        pr = subprocess.run([B.CLI_PATH] + args + more, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert pr.returncode == 2 and all(x in pr.stderr for x in words), (more, pr.stderr[-300:])
    assert not any(os.path.exists(tmp_path / x) for x in "agptb")


def test_align_all_with_the_graphs_switch(cli_cases, tmp_path):
    args, k, m, us, heads, reads, view = cli_cases[1]
    g = B.Graph.from_fasta(args[5], k)
    pf, nf = str(tmp_path / "p"), str(tmp_path / "n")
    with pytest.raises(B.BgrError, match="error -1.*--gaf.*greedy modes"):
        B.align_all(g, args[1], pf, nf, m=m, mode=EXH, gaf=True)
    assert not g.exhaustive_paths_enabled()
    B.align_all(g, args[1], pf, nf, m=m, mode=EXH, gaf=True, abundance=True, links=True, exhaustive_paths=True)
    assert not g.exhaustive_paths_enabled()
    assert open(pf).read() == G.gaf_of(us, k, heads, reads, view)[0]
    lens = A.unitig_lens(us)
    assert [tuple(int(x) for x in r) for r in g.abundance()] == [tuple(r) for r in A.abundance_of(lens, k, [len(r) for r in reads], view)[1:]]
    with pytest.raises(B.BgrError, match="error -1.*need exhaustive mode"):
        B.align_all(g, args[1], pf, nf, m=m, exhaustive_paths=True)
    with pytest.raises(B.BgrError, match="error -1.*partial paths"):
        B.align_all(g, args[1], pf, nf, m=m, mode=EXH, partial=True, exhaustive_paths=True)
    with pytest.raises(B.BgrError, match="error -1.*--write-exhaustive"):
        B.align_all(g, args[1], pf, nf, m=m, mode=EXH, gaf=True, write_exhaustive=True, exhaustive_paths=True)
