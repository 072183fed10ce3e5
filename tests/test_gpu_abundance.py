"""Per-unitig abundance on the GPU: `--abundance` through the CLI on every route, bgr_aligner_abundance behind the batch, text and
device-resident calls, both forms of the kernel -- against abundance_ref.py (the definition in plain Python, pinned by test_abundance_host.py)
over rows of the oracle (goldens), of wide_greedy_ref (k > 32) or of the batch API itself (pinned to both elsewhere)."""
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
import wide_greedy_ref as W
from test_abundance_host import abundance_cases, paths_bytes
from test_gaf_host import EXC_GRAPHS, golden_rows
from test_gpu_wide_k import graph_and_reads
from test_wide_k_host import pack, strings
from tools.synth import Synth
from util import GOLD, parse_counters, resolve_args, sha

pytestmark = pytest.mark.gpu

CASES = abundance_cases()


def run(args, timeout=600):
    """the CLI with --abundance in a scratch directory -> (stdout, paths bytes -- the pairs of a split run concatenated --, notAligned bytes, abundance bytes)"""
    d = tempfile.mkdtemp()
    try:
        p = subprocess.run([B.CLI_PATH] + list(args) + ["--abundance", os.path.join(d, "ab.tsv")], cwd=d, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:
            raise RuntimeError("%s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
        def cat(name):
            if os.path.exists(os.path.join(d, name + ".0")):
                return b"".join(open(os.path.join(d, "%s.%d" % (name, i)), "rb").read() for i in range(8) if os.path.exists(os.path.join(d, "%s.%d" % (name, i))))
            return open(os.path.join(d, name), "rb").read() if os.path.exists(os.path.join(d, name)) else b""
        ab = os.path.join(d, "ab.tsv")   # (None: the run wrote no abundance file)
        return p.stdout, cat("paths"), cat("notAligned.fa"), open(ab, "rb").read() if os.path.exists(ab) else None
    finally:
        shutil.rmtree(d)


def table_of(arr):
    """(n, 3) array of the API -> abundance_ref's table (entry 0 unused)"""
    return [[0, 0, 0]] + [[int(x) for x in r] for r in arr]


def add_tables(a, b):
    return [[x + y for x, y in zip(r, s)] for r, s in zip(a, b)]


@pytest.mark.parametrize("case", CASES, ids=["%02d-%s" % (c["id"], c["group"]) for c in CASES])
def test_cli_abundance_on_the_goldens(case):
    """the file = abundance_ref over the oracle's rows, whatever the route, the batching, the key layout, the number of lanes and the other
    outputs asked for; paths, notAligned.fa and the counters stay the golden's"""
    a, us, H, R, rows = golden_rows(case)
    lens = A.unitig_lens(us)
    want = A.text_of(lens, A.abundance_of(lens, a["k"], [len(r) for r in R], rows))
    plain = not a["correct"]
    acgt = a["graph"] not in EXC_GRAPHS
    lanes = ["--gpus", "2", "--set", "test.lanes_on_one_device=1"]
    variants = [[], ["--host-route"], ["-t", "5", "--batch", "37", "--chunk-bytes", "600"], lanes, lanes + ["--split-output"]]
    if not a["anchors"]:
        variants.append(["--set", "test.wide_keys=1"])
    stopped = not case["counters"]   # the reference's run ended with "bug compaction" (-c on a graph with exception planes): no totals, no file
    for extra in variants:
        out, paths, na, ab = run(resolve_args(case["args"]) + extra)
        if stopped:
            assert ab is None and "bug compaction" in out and parse_counters(out) == {}, (case["args"], extra)
            if extra[:1] != ["--gpus"]:   # (one lane: the files end where the reference's do)
                assert len(paths) == case["paths_len"] and sha(paths) == case["paths_sha256"], (case["args"], extra)
                assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"], (case["args"], extra)
            continue
        assert ab == want, (case["args"], extra)
        assert parse_counters(out) == case["counters"], (case["args"], extra)
        assert len(paths) == case["paths_len"] and sha(paths) == case["paths_sha256"], (case["args"], extra)
        assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"], (case["args"], extra)
        if plain:   # the reads column by another road: the ids of the paths file this run wrote
            assert [t[0] for t in A.parse_text(ab)[1]] == A.ids_in_paths(paths, len(lens) - 1), (case["args"], extra)
    if plain and acgt:   # together with the outputs that replace the path records
        gaf, bug = G.gaf_of(us, a["k"], H, R, rows)
        assert bug is None
        for extra in ([], ["--host-route"]):
            out, paths, na, ab = run(resolve_args(case["args"]) + ["--gaf"] + extra)
            assert ab == want and paths == gaf.encode("latin-1") and parse_counters(out) == case["counters"], (case["args"], extra)
            out, paths, na, ab = run(resolve_args(case["args"]) + ["-c"] + extra)
            assert ab == want and parse_counters(out) == case["counters"], (case["args"], extra)
            assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"], (case["args"], extra)


def test_cli_output_without_the_flag_is_unchanged():
    """stdout too: the flag adds a file and nothing else"""
    case = next(c for c in CASES if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    out, paths, na, ab = run(resolve_args(case["args"]))
    d = tempfile.mkdtemp()
    try:
        p = subprocess.run([B.CLI_PATH] + resolve_args(case["args"]), cwd=d, capture_output=True, text=True, timeout=600)
        strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
        assert p.returncode == 0 and strip(p.stdout) == strip(out)
        assert open(os.path.join(d, "paths"), "rb").read() == paths and open(os.path.join(d, "notAligned.fa"), "rb").read() == na
        assert sorted(os.listdir(d)) == ["notAligned.fa", "paths"]
    finally:
        shutil.rmtree(d)
    t = A.parse_text(ab)[1]
    assert t[363][0] >= 1 and t[364][1] >= 87   # (r0 of the file lies on 363 364 366 367: test_abundance_host.test_hand_checked_rows)


def test_the_goldens_cover_what_they_should():
    assert len(CASES) >= 70 and any(c for c in CASES if "-G" in c["args"]) and any(c for c in CASES if "-q" in c["args"])
    assert any(c for c in CASES if any(x in EXC_GRAPHS for x in c["args"]))


@pytest.mark.parametrize("fastq", [False, True])
@pytest.mark.parametrize("k", [33, 47, 63, 64])
def test_cli_abundance_wide_k(k, fastq, tmp_path):
    unitigs, reads = graph_and_reads(k, 100 * k)
    reads = [r for r in reads if len(r) > k]   # (as test_gpu_wide_k.test_cli_k63: a FASTA reader drops the others)
    with open(tmp_path / "u.fa", "w") as f:
        for i, u in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, u))
    rf = tmp_path / ("r.fq" if fastq else "r.fa")
    heads = [("@r%d" if fastq else ">r%d") % i for i in range(len(reads))]
    with open(rf, "w") as f:
        for h, r in zip(heads, reads):
            f.write(("%s\n%s\n+\n%s\n" % (h, r, "I" * len(r))) if fastq else ("%s\n%s\n" % (h, r)))
    args = ["-r", str(rf), "-k", str(k), "-g", str(tmp_path / "u.fa"), "-m", "2", "-e", "2", "-t", "4"] + (["-q"] if fastq else [])
    ref = W.GreedyRef(k, unitigs)
    rows, cnt = ref.align(reads, 2, 2)
    lens = A.unitig_lens([""] + unitigs)
    table = A.abundance_of(lens, k, [len(r) for r in reads], rows)
    want = A.text_of(lens, table)
    assert cnt["aligned"] > 50 and sum(t[2] for t in table) > 0
    _, pa, na, ab = run(args)
    _, pb, nb, ab2 = run(args + ["--host-route"])
    assert ab == want and ab2 == want and pa == pb == paths_bytes(heads, rows) and na == nb
    # the GAF lines of the same input: every k-mer of a covered stretch lies in exactly one unitig
    _, pg, _, ab3 = run(args + ["--gaf"])
    assert ab3 == want
    blocks = [G.parse_line(ln + "\n")["block"] for ln in pg.decode().split("\n")[:-1]]
    assert len(blocks) == cnt["aligned"] and sum(max(0, b - (k - 1)) for b in blocks) == sum(t[2] for t in table)


def _mixed_reads(s, k, rnd):
    reads = []
    for L, n in ((k + 1, 40), (2 * k + 3, 100), (150, 300), (251, 100), (1000, 20), (20000, 4)):
        rb, ro = s.reads(0, n, L, 3, 31 * k + L)
        reads += strings(rb, ro)
    reads = [W.reverse_complements(r) if i % 2 else r for i, r in enumerate(reads)]
    for i in range(0, len(reads), 6):   # N reads
        r = list(reads[i])
        r[rnd.randrange(len(r))] = "N"
        reads[i] = "".join(r)
    rnd.shuffle(reads)
    return reads


@pytest.mark.parametrize("k", [8, 15, 31, 32, 33, 48, 64])
def test_batch_api_deltas(k):
    """after every launch the table has grown by abundance_ref over the rows that launch returned; both forms of the kernel, side by side"""
    rnd = random.Random(k)
    s = Synth(60000, max(40, 2 * k), 2, k, 900 + k)
    seqs, offs = s.unitigs()
    lens = A.unitig_lens([""] + strings(seqs, offs))
    g = B.Graph.build(k, seqs, offs)
    als = []
    for form in (B.ABUNDANCE_GLOBAL, B.ABUNDANCE_LDS, B.ABUNDANCE_AUTO):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_ABUNDANCE_FORM, form)
        al.abundance_enable()
        assert not al.abundance().any()
        als.append(al)
    reads = _mixed_reads(s, k, rnd)
    total = [[0, 0, 0] for _ in lens]
    n_mapped = n_multi = n_long = 0
    for lo, hi in ((0, 1), (1, 18), (18, 277), (277, len(reads))):   # ragged batches
        batch = reads[lo:hi]
        rb, ro = pack(batch)
        for m, e in ((0, 0), (2, 2), (5, 5), (2, 1)):
            rows = None
            for al in als:
                got = W.rows_of(*al.align(rb, ro, m=m, effort=e))
                assert rows is None or got == rows
                rows = got
            total = add_tables(total, A.abundance_of(lens, k, [len(r) for r in batch], rows))
            for al in als:
                assert table_of(al.abundance()) == total, (k, lo, m, e)
            n_mapped += sum(1 for _, p in rows if p)
            n_multi += sum(1 for _, p in rows if len(p) > 17)   # (more unitigs than one pass of the kernel's sixteen lanes takes)
            n_long += sum(1 for i, (_, p) in enumerate(rows) if len(p) > 40 and len(batch[i]) == 20000)
    print("k", k, "mapped", n_mapped, "multi-pass paths", n_multi, "20 kb reads with long paths", n_long)
    # (at k = 8 the 60 kb genome holds most 8-mers more than once: its unitigs are a few bases long and no 20 kb read maps, as in test_gpu_gaf.test_path_stats_rows)
    assert n_mapped > 500 and n_multi > 0 and (n_long > 0 or k == 8) and sum(t[2] for t in total) > 0
    al = als[0]
    assert "bgr_abundance_kernel" in [n for n, _ in al.kernel_times()[1]]
    # the other entry points: packed planes, begin / wait, the device-resident call with a fetch into a buffer that is too small first
    rb, ro = pack(reads[18:277])
    rows = W.rows_of(*al.align_packed(B.pack_reads(rb, ro), m=2, effort=2))
    assert rows == W.rows_of(*al.align_wait(al.align_begin(rb, ro, m=2, effort=2)))
    d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
    al.align_device(d_r.data_ptr(), d_o.data_ptr(), len(ro) - 1, int(ro[-1]), max(len(x) for x in reads[18:277]), m=2, effort=2)
    with pytest.raises(B.BgrError, match="error -4"):
        al.fetch(len(ro) - 1, 4)
    assert W.rows_of(*al.fetch(len(ro) - 1, int(ro[-1]) + 8 * len(ro))) == rows
    one = A.abundance_of(lens, k, [len(r) for r in reads[18:277]], rows)
    total = add_tables(total, add_tables(one, add_tables(one, one)))
    assert table_of(al.abundance()) == total
    # disabled launches add nothing; the table stays; reset zeroes
    al.abundance_enable(False)
    al.align(rb, ro, m=2, effort=2)
    assert table_of(al.abundance()) == total
    al.abundance_enable(True)
    al.reset_abundance()
    assert not al.abundance().any()
    al.align(rb, ro, m=2, effort=2)
    assert table_of(al.abundance()) == one
    d_r.free()
    d_o.free()


@pytest.mark.parametrize("genome,fits", [(200000, True), (600000, False)])
def test_forms_on_larger_tables(genome, fits):
    """form B with a table beyond 48 KB of LDS, and a graph whose table no workgroup can hold (knob 2 then runs form A)"""
    k = 31
    s = Synth(genome, 75, 2, k, 77)
    seqs, offs = s.unitigs()
    lens = A.unitig_lens([""] + strings(seqs, offs))
    assert (48 * 1024 < 12 * len(lens) <= 160 * 1024) == fits and (fits or 12 * len(lens) > 160 * 1024)
    g = B.Graph.build(k, seqs, offs)
    rb, ro = s.reads(0, 60000, 150, 2, 78)
    want = None
    for form in (B.ABUNDANCE_GLOBAL, B.ABUNDANCE_LDS, B.ABUNDANCE_AUTO):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_ABUNDANCE_FORM, form)
        al.abundance_enable()
        # which kernel runs (the tables cannot tell): knob 2 is form B with the whole table in a workgroup's LDS where it fits, form A where not
        plan = al.abundance_plan(60000, 60000 * 150)
        if form == B.ABUNDANCE_AUTO:   # (60 000 reads on thousands of counters per workgroup: below the automatic choice's threshold, pinned in test_abundance_host)
            assert plan == B.plan_abundance(len(lens) - 1, k, 60000, 60000 * 150) and plan["form"] == 1, plan
        else:
            assert plan["form"] == (2 if fits and form == B.ABUNDANCE_LDS else 1), (form, plan)
        assert plan["lds_bytes"] == (12 * len(lens) if plan["form"] == 2 else 0) and plan["blocks"] > 0
        rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
        if want is None:
            want = A.abundance_of(lens, k, [150] * 60000, rows)
        assert table_of(al.abundance()) == want, form
        al.align(rb, ro, m=2, effort=2)
        assert table_of(al.abundance()) == add_tables(want, want), form
    assert sum(t[0] for t in want) > 100000


def test_overlapped_and_split_batches():
    """one bgr_align_batch of >= 512 k reads runs in pieces on four streams (the aligner and its twins): the table is the sum over its rows;
    a small split limit maps a batch in many launches: the same table"""
    k = 31
    s = Synth(150000, 90, 2, k, 5)
    seqs, offs = s.unitigs()
    lens = A.unitig_lens([""] + strings(seqs, offs))
    g = B.Graph.build(k, seqs, offs)
    n = 540000
    rb, ro = s.reads(0, n, 100, 2, 6, threads=8)
    al = B.Aligner(g, 0)
    al.set_knob(B.KNOB_ABUNDANCE_FORM, B.ABUNDANCE_LDS)   # (set before the twins exist: it must reach them)
    al.abundance_enable()
    rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
    want = A.abundance_of(lens, k, [100] * n, rows)
    assert table_of(al.abundance()) == want and sum(t[0] for t in want) > n
    assert al.counters()["reads"] == n
    al.set_knob(B.KNOB_ABUNDANCE_FORM, B.ABUNDANCE_GLOBAL)   # (the twins exist: it must reach them too)
    al.align(rb, ro, m=2, effort=2)
    assert table_of(al.abundance()) == add_tables(want, want)
    al.reset_abundance()   # (the twins' tables too)
    assert not al.abundance().any()
    al.abundance_enable(False)
    al.align(rb, ro, m=2, effort=2)
    assert not al.abundance().any()
    # many launches of one call
    m = 30000
    al2 = B.Aligner(g, 0)
    al2.abundance_enable()
    al2.set_knob(B.KNOB_BATCH_SPLIT_LIMIT, 200000)
    assert W.rows_of(*al2.align(rb[: int(ro[m])], ro[: m + 1], m=2, effort=2)) == rows[:m]
    assert table_of(al2.abundance()) == A.abundance_of(lens, k, [100] * m, rows[:m])


def test_text_form_counts_once():
    """a paths buffer that is too small: BGR_E_CAPACITY, then the same device results through bgr_aligner_fetch_text -- one launch, counted once"""
    k, n = 31, 20000
    s = Synth(150000, 90, 2, k, 21)
    seqs, offs = s.unitigs()
    lens = A.unitig_lens([""] + strings(seqs, offs))
    g = B.Graph.build(k, seqs, offs)
    rb, ro = s.reads(0, n, 150, 2, 22)
    reads = strings(rb, ro)
    text = "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)).encode()
    rows = W.rows_of(*B.Aligner(g, 0).align(rb, ro, m=2, effort=2))
    want = A.abundance_of(lens, k, [150] * n, rows)
    al = B.Aligner(g, 0)
    al.abundance_enable()
    p, na, info = al.align_fasta_text(text, m=2, effort=2, paths_cap=1000)
    assert not info["irregular"] and p == paths_bytes([">r%d" % i for i in range(n)], rows) and len(p) > 1000
    assert table_of(al.abundance()) == want
    for want_output in (2, 3):   # -c and GAF through the text call
        al.align_fasta_text(text, m=2, effort=2, want_output=want_output, paths_cap=1000)
    assert table_of(al.abundance()) == add_tables(want, add_tables(want, want))


def test_skewed_input_is_exact():
    """every read of >= 200 k lands on a graph of a handful of unitigs: all adds of the launch meet in a few counters"""
    k, K1 = 31, 30
    rng = np.random.default_rng(3)
    genome = "".join("ACGT"[i] for i in rng.integers(0, 4, size=390))
    cuts = [0, 65, 130, 195, 260, 325, 390]   # (a cut every 65 bases: each window of 100 holds the k-1 bases in front of one, the overlap a read needs to map at all)
    unitigs = [genome[max(0, cuts[i] - K1): cuts[i + 1]] for i in range(len(cuts) - 1)]
    lens = A.unitig_lens([""] + unitigs)
    g = B.Graph.build(k, *pack(unitigs))
    assert g.info()["n_unitigs"] == 6
    n, L = 210000, 100
    starts = rng.integers(0, len(genome) - L, size=n)
    reads = [genome[int(x): int(x) + L] for x in starts]
    reads = [W.reverse_complements(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    rb, ro = pack(reads)
    want = None
    for form in (B.ABUNDANCE_GLOBAL, B.ABUNDANCE_LDS, B.ABUNDANCE_AUTO):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_ABUNDANCE_FORM, form)
        al.set_knob(B.KNOB_BATCH_OVERLAP, 1)   # one launch
        al.abundance_enable()
        assert al.abundance_plan(n, n * L)["form"] == (1 if form == B.ABUNDANCE_GLOBAL else 2)   # (the automatic choice here is form B)
        rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
        if want is None:
            want = A.abundance_of(lens, k, [L] * n, rows)
            mapped = sum(1 for _, p in rows if p)
            assert mapped >= 200000, mapped
            assert sum(t[2] for t in want) == mapped * (L - K1)   # (every mapped read is covered in full: each of its k-mers lies in one unitig)
        for rep in range(1, 4):
            assert table_of(al.abundance()) == [[x * rep for x in t] for t in want], (form, rep)
            al.align(rb, ro, m=2, effort=2)


def test_refusals(tmp_path):
    s = Synth(20000, 75, 2, 31, 5)
    g = B.Graph.build(31, *s.unitigs())
    al = B.Aligner(g, 0)
    rb, ro = s.reads(0, 50, 150, 2, 6)
    with pytest.raises(B.BgrError, match="error -1.*never enabled"):
        al.abundance()
    al.abundance_enable()
    with pytest.raises(B.BgrError, match="error -1.*exhaustive"):
        al.align(rb, ro, mode=B.MODE_EXHAUSTIVE)
    assert not al.abundance().any()
    al.abundance_enable(False)
    al.align(rb, ro, mode=B.MODE_EXHAUSTIVE)   # (not counting: exhaustive launches are welcome again)
    assert not al.abundance().any()
    with pytest.raises(B.BgrError, match="error -1"):
        al.set_knob(B.KNOB_ABUNDANCE_FORM, 3)
    out = np.zeros((3, 3), dtype=np.uint64)
    assert B.lib().bgr_aligner_abundance(al.h, out.ctypes.data, 3) == -1 and b"n_rows" in B.lib().bgr_last_error()
    pr = subprocess.run([B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5", "-g", os.path.join(GOLD, "deg_unitig.fa"), "-b", "--abundance", str(tmp_path / "ab")],
                        cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 2 and "--abundance" in pr.stderr and "-b" in pr.stderr and not os.path.exists(tmp_path / "ab"), (pr.returncode, pr.stderr[-500:])


def test_align_all_keeps_the_totals_in_the_graph(tmp_path):
    case = next(c for c in CASES if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    a, us, H, R, rows = golden_rows(case)
    lens = A.unitig_lens(us)
    want = A.abundance_of(lens, 31, [len(r) for r in R], rows)
    g = B.Graph.from_fasta(os.path.join(GOLD, "syn_unitig.fa"), 31)
    f = os.path.join(GOLD, "syn_r150.fa")
    with pytest.raises(B.BgrError):
        g.abundance()
    B.align_all(g, f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2, threads=2, abundance=True)
    assert table_of(g.abundance()) == want
    B.align_all(g, f + "," + f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2, threads=2, route=1, abundance=True)   # the next such run replaces them
    assert table_of(g.abundance()) == add_tables(want, want)
    B.align_all(g, f, str(tmp_path / "p"), str(tmp_path / "n"), m=2, effort=2)   # a run without the flag leaves them
    assert table_of(g.abundance()) == add_tables(want, want)
    with pytest.raises(B.BgrError):   # a run that fails leaves none
        B.align_all(g, str(tmp_path / "missing.fa"), str(tmp_path / "p"), str(tmp_path / "n"), abundance=True)
    with pytest.raises(B.BgrError):
        g.abundance()
    B.write_abundance(str(tmp_path / "ab"), g, np.array(want[1:], dtype=np.uint64))
    assert open(tmp_path / "ab", "rb").read() == A.text_of(lens, want)
