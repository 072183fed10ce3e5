"""Links on the GPU: `--gfa` through the CLI on every route, bgr_aligner_links behind the batch, text and device-resident calls, both forms
of the kernel -- against links_ref.py (the definitions in plain Python, pinned by test_links_host.py) over rows of the oracle (goldens) or of
the batch API itself (pinned to the oracle and to wide_greedy_ref elsewhere)."""
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import abundance_ref as A
import bgreat_amd as B
import gaf_ref as G
import links_ref as K
import wide_greedy_ref as W
from test_abundance_host import abundance_cases
from test_gaf_host import EXC_GRAPHS, golden_rows
from test_gpu_abundance import _mixed_reads
from test_wide_k_host import pack, strings
from tools.synth import Synth
from util import GOLD, parse_counters, resolve_args, sha

pytestmark = pytest.mark.gpu

CASES = abundance_cases()


def run(args, gfa=True, timeout=600):
    """the CLI (with --gfa) in a scratch directory -> (stdout, paths bytes -- the pairs of a split run concatenated --, notAligned bytes,
    GFA bytes or None, abundance bytes or None, the names in the directory)"""
    d = tempfile.mkdtemp()
    try:
        p = subprocess.run([B.CLI_PATH] + list(args) + (["--gfa", os.path.join(d, "g.gfa")] if gfa else []), cwd=d, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:
            raise RuntimeError("%s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
        def cat(name):
            if os.path.exists(os.path.join(d, name + ".0")):
                return b"".join(open(os.path.join(d, "%s.%d" % (name, i)), "rb").read() for i in range(8) if os.path.exists(os.path.join(d, "%s.%d" % (name, i))))
            return open(os.path.join(d, name), "rb").read() if os.path.exists(os.path.join(d, name)) else None
        return p.stdout, cat("paths") or b"", cat("notAligned.fa") or b"", cat("g.gfa"), cat("ab.tsv"), sorted(os.listdir(d))
    finally:
        shutil.rmtree(d)


def links_dict(arr):
    """array of B.LINK_DTYPE -> links_ref's counts; the order the library delivered them in is checked on the way"""
    out = [(int(r["from"]), int(r["to"]), int(r["count"])) for r in arr]
    assert out == K.sorted_links({(a, b): c for a, b, c in out}) and len({(a, b) for a, b, _ in out}) == len(out)
    assert all(K.canonical(a, b) == (a, b) for a, b, _ in out)
    return {(a, b): c for a, b, c in out}


def want_gfa(a, us, R, rows):
    lens = A.unitig_lens(us)
    return K.gfa_text(us, a["k"], A.abundance_of(lens, a["k"], [len(r) for r in R], rows), K.links_of(rows, len(us) - 1))


@pytest.mark.parametrize("case", CASES, ids=["%02d-%s" % (c["id"], c["group"]) for c in CASES])
def test_cli_gfa_on_the_goldens(case):
    """the file = links_ref over the oracle's rows, whatever the route, the batching, the key layout and the number of lanes; paths, notAligned.fa
    and the counters stay the golden's"""
    a, us, H, R, rows = golden_rows(case)
    want = want_gfa(a, us, R, rows)
    lanes = ["--gpus", "2", "--set", "test.lanes_on_one_device=1"]
    variants = [[], ["--host-route"], ["-t", "5", "--batch", "37", "--chunk-bytes", "600"], lanes, lanes + ["--split-output"]]
    if not a["anchors"]:
        variants.append(["--set", "test.wide_keys=1"])
    stopped = not case["counters"]   # the reference's run ended with "bug compaction" (-c on a graph with exception planes): no totals, no file
    lens = A.unitig_lens(us)
    for extra in variants:
        with_ab = extra[:1] == ["-t"]   # one of the variants asks for --abundance as well
        out, paths, na, gfa, ab, _ = run(resolve_args(case["args"]) + extra + (["--abundance", "ab.tsv"] if with_ab else []))
        if stopped:
            assert gfa is None and ab is None and "bug compaction" in out and parse_counters(out) == {}, (case["args"], extra)
            continue
        assert gfa == want, (case["args"], extra)
        assert parse_counters(out) == case["counters"], (case["args"], extra)
        assert len(paths) == case["paths_len"] and sha(paths) == case["paths_sha256"], (case["args"], extra)
        assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"], (case["args"], extra)
        if with_ab:   # the S lines' RC and KC are that file's columns
            flens, table = A.parse_text(ab)
            k1, segs, links = K.parse_gfa(gfa)
            assert flens == lens and [(s[2], s[3], s[4]) for s in segs] == [(lens[i], table[i][0], table[i][2]) for i in range(1, len(lens))], case["args"]
            assert k1 == (a["k"] - 1 if links else None)
    if stopped or a["correct"] or a["graph"] in EXC_GRAPHS:
        return
    # with --gaf: every consecutive pair of segments of every GAF line is an L line of the same run's GFA after canonicalisation -- the lines of reads
    # mapped on their reverse complement hold their paths reversed and flipped -- and the L counts sum to the segments less one over the lines
    gaf, bug = G.gaf_of(us, a["k"], H, R, rows)
    assert bug is None
    out, paths, na, gfa, _, _ = run(resolve_args(case["args"]) + ["--gaf"])
    assert gfa == want and paths == gaf.encode("latin-1") and parse_counters(out) == case["counters"], case["args"]
    k1, segs, links = K.parse_gfa(gfa)
    seen, n_pairs = {}, 0
    for ln in paths.decode("latin-1").split("\n")[:-1]:
        segments = G.parse_line(ln + "\n")["segments"]
        n_pairs += len(segments) - 1
        for x, y in K.gaf_pairs(segments):
            c = K.canonical(x, y)
            assert c in links, (case["args"], ln)
            seen[c] = seen.get(c, 0) + 1
    assert seen == links and sum(links.values()) == n_pairs, case["args"]


def test_the_goldens_cover_what_they_should():
    assert len(CASES) >= 70 and any(c for c in CASES if "-G" in c["args"]) and any(c for c in CASES if "-q" in c["args"]) and any(c for c in CASES if "-c" in c["args"])
    assert any(c for c in CASES if any(x in EXC_GRAPHS for x in c["args"]))
    # reads mapped on their reverse complement with paths of several unitigs: the strand rule has something to pin
    case = next(c for c in CASES if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    _, _, _, _, rows = golden_rows(case)
    assert sum(1 for st, p in rows if st & W.ST_RC and len(p) > 2) > 20


def test_cli_output_without_the_flag_is_unchanged():
    """stdout too: the flag adds a file and nothing else"""
    case = next(c for c in CASES if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    out, paths, na, gfa, _, names = run(resolve_args(case["args"]))
    out0, paths0, na0, gfa0, _, names0 = run(resolve_args(case["args"]), gfa=False)
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
    assert strip(out0) == strip(out) and paths0 == paths and na0 == na
    assert names0 == ["notAligned.fa", "paths"] and names == ["g.gfa", "notAligned.fa", "paths"] and gfa0 is None
    k1, segs, links = K.parse_gfa(gfa)
    assert k1 == 30 and links[(363, 364)] >= 1 and links[(364, -366)] >= 1 and links[(-366, 367)] >= 1   # (r0 of the file: 363 364 -366 367)


@pytest.mark.parametrize("k", [8, 31, 33, 64])
def test_batch_api_deltas(k):
    """after every launch the table has grown by links_ref over the rows that launch returned; all three knob values, side by side"""
    rnd = random.Random(k)
    s = Synth(60000, max(40, 2 * k), 2, k, 900 + k)
    seqs, offs = s.unitigs()
    n_unitigs = len(offs) - 1
    g = B.Graph.build(k, seqs, offs)
    als = []
    for form in (B.LINKS_GLOBAL, B.LINKS_LDS, B.LINKS_AUTO):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_LINKS_FORM, form)
        al.links_enable()
        assert len(al.links()) == 0
        info = al.links_info()
        assert info["bound"] == g.links_bound() and info["capacity"] >= 2 * info["bound"] and info["capacity"] & (info["capacity"] - 1) == 0 and info["overflow"] == 0
        als.append(al)
    assert [al.links_plan(1000)["form"] for al in als] == [1, 2, 1 if g.links_bound() > 1024 else 2]
    reads = _mixed_reads(s, k, rnd)
    total = {}
    n_mapped = n_multi = 0
    for lo, hi in ((0, 1), (1, 18), (18, 277), (277, len(reads))):   # ragged batches
        batch = reads[lo:hi]
        rb, ro = pack(batch)
        for m, e in ((0, 0), (2, 2), (5, 5)):
            rows = None
            for al in als:
                got = W.rows_of(*al.align(rb, ro, m=m, effort=e))
                assert rows is None or got == rows
                rows = got
            total = K.add_counts(total, K.links_of(rows, n_unitigs))
            for al in als:
                assert links_dict(al.links()) == total, (k, lo, m, e)
            n_mapped += sum(1 for _, p in rows if p)
            n_multi += sum(1 for _, p in rows if len(p) > 18)   # (more than 17 unitigs: a pair straddles two passes of the kernel's sixteen lanes)
    print("k", k, "mapped", n_mapped, "paths of more than 17 unitigs", n_multi, "links", len(total), "bound", g.links_bound())
    assert n_mapped > 500 and n_multi > 0 and len(total) > 100 and len(total) <= g.links_bound()
    assert all(al.links_info()["overflow"] == 0 for al in als)
    al = als[0]
    assert "bgr_links_kernel" in [n for n, _ in al.kernel_times()[1]]
    # the other entry points: packed planes, begin / wait, the device-resident call with a fetch into a buffer that is too small first
    # (the text call: test_text_form_counts_once)
    sub = reads[18:277]
    rb, ro = pack(sub)
    rows = W.rows_of(*al.align_packed(B.pack_reads(rb, ro), m=2, effort=2))
    assert rows == W.rows_of(*al.align_wait(al.align_begin(rb, ro, m=2, effort=2)))
    d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), len(ro) - 1, int(ro[-1]), max(len(x) for x in sub), m=2, effort=2)
    with pytest.raises(B.BgrError, match="error -4"):
        al.fetch(len(ro) - 1, 4)
    assert W.rows_of(*al.fetch(len(ro) - 1, int(ro[-1]) + 8 * len(ro))) == rows
    one = K.links_of(rows, n_unitigs)
    total = K.add_counts(total, K.add_counts(one, K.add_counts(one, one)))
    assert links_dict(al.links()) == total
    # a small cap: BGR_E_CAPACITY and the right n
    n = B.C.c_uint64(0)
    buf = np.zeros(3, dtype=B.LINK_DTYPE)
    assert B.lib().bgr_aligner_links(al.h, buf.ctypes.data, 3, B.C.byref(n)) == -4 and n.value == len(total) and not buf["count"].any()
    # disabled launches add nothing; the table stays; reset zeroes
    al.links_enable(False)
    al.align(rb, ro, m=2, effort=2)
    assert links_dict(al.links()) == total
    al.links_enable(True)
    al.reset_links()
    assert len(al.links()) == 0
    al.align(rb, ro, m=2, effort=2)
    assert links_dict(al.links()) == one
    d_r.free()
    d_o.free()


def test_text_form_counts_once():
    """a paths buffer that is too small: BGR_E_CAPACITY, then the same device results through bgr_aligner_fetch_text -- one launch, counted once"""
    k, n = 31, 6000
    s = Synth(150000, 90, 2, k, 21)
    seqs, offs = s.unitigs()
    g = B.Graph.build(k, seqs, offs)
    rb, ro = s.reads(0, n, 150, 2, 22)
    text = "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(strings(rb, ro))).encode()
    rows = W.rows_of(*B.Aligner(g, 0).align(rb, ro, m=2, effort=2))
    want = K.links_of(rows, len(offs) - 1)
    al = B.Aligner(g, 0)
    al.links_enable()
    p, na, info = al.align_fasta_text(text, m=2, effort=2, paths_cap=1000)
    assert not info["irregular"] and len(p) > 1000 and len(want) > 1000
    assert links_dict(al.links()) == want
    for want_output in (2, 3):   # -c and GAF through the text call
        al.align_fasta_text(text, m=2, effort=2, want_output=want_output, paths_cap=1000)
    assert links_dict(al.links()) == {l: 3 * c for l, c in want.items()}


def _tandem():
    """three unitigs by hand, k = 9: the middle one begins and ends with the same 8-mer, so a walk crosses it any number of times in a row"""
    rnd = random.Random(5)
    w, sp = "AACCGGTA", "CTCAG"
    fa, fb = ("".join(rnd.choice("ACGT") for _ in range(40)) for _ in range(2))
    unitigs = [fa + w, w + sp + w, w + fb]
    reads = []
    for r in (1, 2, 3, 5, 8, 20, 33):
        s = fa + w + (sp + w) * r + fb
        reads += [s[lo:len(s) - hi] for lo, hi in ((0, 0), (10, 5), (30, 30))]
    reads += [W.reverse_complements(x) for x in reads]
    reads.append((sp + w) * 4)
    return unitigs, reads


def test_tandem_repeat_graph():
    """a read's path holds (a, a), and the same link several times; with 33 copies the repeat spans three passes of the kernel.  The table of links is
    shrunk to 64 slots through the test hook -- links_ref says the graph's three links fit -- and the overflow word behind it stays 0."""
    unitigs, reads = _tandem()
    g = B.Graph.build(9, *pack(unitigs))
    assert g.links_bound() >= 3
    rb, ro = pack(reads)
    want = None
    for form in (B.LINKS_GLOBAL, B.LINKS_LDS, B.LINKS_AUTO):
        with B.options(**{"test.links_capacity": 64}):
            al = B.Aligner(g, 0)
            al.set_knob(B.KNOB_LINKS_FORM, form)
            al.links_enable()
        assert al.links_info()["capacity"] == 64
        rows = W.rows_of(*al.align(rb, ro, m=0, effort=2))
        if want is None:
            want = K.links_of(rows, 3)
            assert rows[0][1] == [0, 1, 2, 3] and any(p[1:] == [1] + [2] * 33 + [3] for _, p in rows) and any(p[1:] == [-3] + [-2] * 20 + [-1] for _, p in rows)
            assert set(want) == {(1, 2), (2, 2), (2, 3)} and want[(2, 2)] > 4 * want[(1, 2)] and want[(1, 2)] == want[(2, 3)] == 42
        assert links_dict(al.links()) == want, form
        al.align(rb, ro, m=0, effort=2)
        assert links_dict(al.links()) == {l: 2 * c for l, c in want.items()}, form
        info = al.links_info()
        assert info["overflow"] == 0 and info["lds_fell_through"] == 0, (form, info)


def _skewed(n, L):
    k, K1 = 31, 30
    rng = np.random.default_rng(3)
    genome = "".join("ACGT"[i] for i in rng.integers(0, 4, size=390))
    cuts = [0, 65, 130, 195, 260, 325, 390]   # (a cut every 65 bases: each window of 100 holds the k-1 bases in front of one, the overlap a read needs to map at all)
    unitigs = [genome[max(0, cuts[i] - K1): cuts[i + 1]] for i in range(len(cuts) - 1)]
    starts = rng.integers(0, len(genome) - L, size=n)
    reads = [genome[int(x): int(x) + L] for x in starts]
    return unitigs, [W.reverse_complements(r) if i % 3 == 0 else r for i, r in enumerate(reads)]


def test_skewed_input_is_exact():
    """every read of 210 000 lands on a graph of six unitigs: all traversals of the launch meet in five links"""
    n, L = 210000, 100
    unitigs, reads = _skewed(n, L)
    g = B.Graph.build(31, *pack(unitigs))
    assert g.info()["n_unitigs"] == 6 and 5 <= g.links_bound() <= 1024
    rb, ro = pack(reads)
    want = None
    for form in (B.LINKS_GLOBAL, B.LINKS_LDS, B.LINKS_AUTO):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_LINKS_FORM, form)
        al.set_knob(B.KNOB_BATCH_OVERLAP, 1)   # one launch
        al.links_enable()
        assert al.links_plan(n)["form"] == (1 if form == B.LINKS_GLOBAL else 2)   # (the automatic choice here is form B)
        rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
        if want is None:
            want = K.links_of(rows, 6)
            assert sum(1 for _, p in rows if p) >= 200000 and sum(want.values()) > 100000 and len(want) == 5
        for rep in range(1, 4):
            assert links_dict(al.links()) == {l: c * rep for l, c in want.items()}, (form, rep)
            al.align(rb, ro, m=2, effort=2)
        assert al.links_info()["lds_fell_through"] == 0


def test_lds_form_falls_through_on_a_graph_with_more_links_than_it_holds():
    """form B forced on a graph with several times the links its LDS table holds, in one launch large enough that a workgroup (one of 512, more than
    a thousand reads each) meets more distinct links than the 2 048 slots: the traversals that find no place go straight to the table in HBM"""
    k, n = 31, 600000
    s = Synth(200000, 75, 2, k, 77)
    seqs, offs = s.unitigs()
    n_unitigs = len(offs) - 1
    g = B.Graph.build(k, seqs, offs)
    rb, ro = s.reads(0, n, 150, 2, 78, threads=8)
    assert B.plan_links(g.links_bound(), n)["form"] == 1   # (the automatic choice here is form A)
    want = None
    for form in (B.LINKS_LDS, B.LINKS_GLOBAL):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_LINKS_FORM, form)
        al.set_knob(B.KNOB_BATCH_OVERLAP, 1)   # one launch
        al.links_enable()
        plan = al.links_plan(n)
        assert plan["form"] == (2 if form == B.LINKS_LDS else 1) and plan == B.plan_links(g.links_bound(), n, form=form), plan
        res = al.align(rb, ro, m=2, effort=2)
        if want is None:
            want = K.links_of(W.rows_of(*res), n_unitigs)
            assert len(want) > 2 * 2048 and len(want) <= g.links_bound()
        assert links_dict(al.links()) == want, form
        al.align(rb, ro, m=2, effort=2)
        assert links_dict(al.links()) == {l: 2 * c for l, c in want.items()}, form
        info = al.links_info()
        assert info["overflow"] == 0 and (info["lds_fell_through"] > 0) == (form == B.LINKS_LDS), (form, info)


def test_overlapped_batches_share_the_table():
    """one bgr_align_batch of >= 512 k reads runs in pieces on four streams (the aligner and its twins), which add to one table"""
    k = 31
    s = Synth(150000, 90, 2, k, 5)
    seqs, offs = s.unitigs()
    g = B.Graph.build(k, seqs, offs)
    n = 540000
    rb, ro = s.reads(0, n, 100, 2, 6, threads=8)
    al = B.Aligner(g, 0)
    al.set_knob(B.KNOB_LINKS_FORM, B.LINKS_LDS)   # (set before the twins exist: it must reach them)
    al.links_enable()
    rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
    want = K.links_of(rows, len(offs) - 1)
    assert links_dict(al.links()) == want and sum(want.values()) > n // 4
    al.set_knob(B.KNOB_LINKS_FORM, B.LINKS_GLOBAL)   # (the twins exist: it must reach them too)
    al.align(rb, ro, m=2, effort=2)
    assert links_dict(al.links()) == {l: 2 * c for l, c in want.items()}
    al.reset_links()
    assert len(al.links()) == 0
    al.links_enable(False)
    al.align(rb, ro, m=2, effort=2)
    assert len(al.links()) == 0


def test_refusals(tmp_path):
    s = Synth(20000, 75, 2, 31, 5)
    g = B.Graph.build(31, *s.unitigs())
    al = B.Aligner(g, 0)
    rb, ro = s.reads(0, 50, 150, 2, 6)
    with pytest.raises(B.BgrError, match="error -1.*never enabled"):
        al.links()
    al.links_enable()
    with pytest.raises(B.BgrError, match="error -1.*exhaustive"):
        al.align(rb, ro, mode=B.MODE_EXHAUSTIVE)
    assert len(al.links()) == 0
    al.links_enable(False)
    al.align(rb, ro, mode=B.MODE_EXHAUSTIVE)   # (not counting: exhaustive launches are welcome again)
    assert len(al.links()) == 0
    with pytest.raises(B.BgrError, match="error -1"):
        al.set_knob(B.KNOB_LINKS_FORM, 3)
    pr = subprocess.run([B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5", "-g", os.path.join(GOLD, "deg_unitig.fa"), "-b", "--gfa", str(tmp_path / "g.gfa")],
                        cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 2 and "--gfa" in pr.stderr and "-b" in pr.stderr and not os.path.exists(tmp_path / "g.gfa"), (pr.returncode, pr.stderr[-500:])


def test_align_all_keeps_the_totals_in_the_graph(tmp_path):
    case = next(c for c in CASES if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    a, us, H, R, rows = golden_rows(case)
    lens = A.unitig_lens(us)
    table = A.abundance_of(lens, 31, [len(r) for r in R], rows)
    want = K.links_of(rows, len(us) - 1)
    g = B.Graph.from_fasta(os.path.join(GOLD, "syn_unitig.fa"), 31)
    f = os.path.join(GOLD, "syn_r150.fa")
    P, N = str(tmp_path / "p"), str(tmp_path / "n")
    with pytest.raises(B.BgrError):
        g.links()
    B.align_all(g, f, P, N, m=2, effort=2, threads=2, links=True)
    assert links_dict(g.links()) == want and [[int(x) for x in r] for r in g.abundance()] == table[1:]
    B.align_all(g, f, P, N, m=2, effort=2)   # the keyword put the switch back: a run with it off leaves the totals alone
    assert links_dict(g.links()) == want
    g.links_enable()   # sticky: every later run counts, and the next such run replaces the totals
    B.align_all(g, f + "," + f, P, N, m=2, effort=2, threads=2, route=1)
    assert links_dict(g.links()) == {l: 2 * c for l, c in want.items()}
    B.write_gfa(str(tmp_path / "g.gfa"), g, g.abundance(), g.links())
    assert open(tmp_path / "g.gfa", "rb").read() == K.gfa_text(us, 31, [[2 * x for x in t] for t in table], {l: 2 * c for l, c in want.items()})
    with pytest.raises(B.BgrError):   # a run that fails leaves none
        B.align_all(g, str(tmp_path / "missing.fa"), P, N)
    with pytest.raises(B.BgrError):
        g.links()
    with pytest.raises(B.BgrError, match="-b.*--gfa|--gfa.*-b"):
        B.align_all(g, f, P, N, mode=B.MODE_EXHAUSTIVE)
