"""Bubbles on the GPU: bgr_links_bubbles on crafted lists and across the tile seams of the compaction, bgr_aligner_bubbles on an aligner's live
table, `--bubbles` through the CLI on every route -- against bubbles_ref.py (the definition in plain Python, which test_bubbles_host.py makes
check itself) over links_ref of the rows of the batch API (pinned to the oracle and to wide_greedy_ref here), of the oracle (goldens) or of
the same run's GFA."""
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bgreat_amd as B
import bubbles_ref as BR
import gaf_ref as G
import links_ref as K
import oracle_py
import wide_greedy_ref as W
from test_abundance_host import abundance_cases
from test_gaf_host import EXC_GRAPHS, golden_rows
from test_wide_k_host import strings
from tools.synth import Synth
from util import GOLD, parse_counters, resolve_args, sha

pytestmark = pytest.mark.gpu

CASES = abundance_cases()
TILE = B.BUBBLES_TILE
BIG = 2 ** 32


def call(counts, n_unitigs, min_link=1):
    """bgr_links_bubbles on links_ref counts -> the records; they are the reference's"""
    with B.options(poison_device_buffers=1):   # (a slot that pass 1 never wrote must not be read: it holds a pattern, not zeroes)
        got = BR.as_tuples(B.links_bubbles(K.sorted_links(counts), n_unitigs, min_link))
    assert got == BR.bubbles_of(counts, min_link), (counts, min_link)
    return got


def canon(links):
    return {K.canonical(a, b): c for (a, b), c in links.items()}


ONE = {(1, 2): 7, (1, 3): 2, (2, 4): 6, (3, 4): 1}


def test_one_bubble_and_its_strand_mate():
    assert call(ONE, 4) == [(1, 4, (2, 3), (7, 6, 2, 1))]
    assert call(ONE, 9) == [(1, 4, (2, 3), (7, 6, 2, 1))]
    # every id negated and reversed: the same links after canonicalisation -- and spelled from the other side with other unitigs, the same single record
    assert canon({(-b, -a): c for (a, b), c in ONE.items()}) == ONE
    assert call(canon({(-4, -2): 6, (-4, -3): 1, (-2, -1): 7, (-3, -1): 2}), 4) == [(1, 4, (2, 3), (7, 6, 2, 1))]
    # walked against its unitigs: the source is the oriented id with the smaller unitig, the branches in (|id|, id < 0) order
    assert call(canon({(-3, -2): 2, (-3, 1): 3, (-2, 4): 4, (1, 4): 5}), 4) == [(-3, 4, (1, -2), (3, 5, 2, 4))]
    assert call(canon({(7, -5): 2, (7, 5000): 3, (-5, -6): 4, (5000, -6): 5}), 5000) == [(6, -7, (5, -5000), (4, 2, 5, 3))]


def test_three_ways_out_store_no_third_successor():
    """1 has three successors; the slots behind its two belong to -1, which opens a bubble of its own: a third successor stored anywhere would spoil it"""
    links = canon({(1, 2): 1, (1, 3): 1, (1, 4): 1, (2, 5): 1, (3, 5): 1, (4, 5): 1, (-1, 6): 3, (-1, 7): 4, (6, 8): 5, (7, 8): 6})
    assert call(links, 8) == [(-1, 8, (6, 7), (3, 5, 4, 6))]
    assert call(canon({(1, 2): 1, (1, 3): 1, (1, 4): 1, (2, 5): 1, (3, 5): 1, (4, 5): 1}), 5) == []
    many = canon({(9, x): x for x in range(1, 9)})   # eight ways out of the last unitig: seven of them only count
    assert call(many, 9) == []


def test_what_is_no_bubble():
    assert call({**ONE, **canon({(5, 2): 1})}, 5) == []        # an extra way into a branch
    assert call({**ONE, **canon({(5, 4): 1})}, 5) == []        # ... into the sink
    assert call({**ONE, **canon({(2, 5): 1})}, 5) == []        # a second way out of a branch
    assert call({(1, 2): 1, (1, 3): 1, (2, 4): 1, (3, 5): 1}, 5) == []            # branches that lead to different sinks
    assert call(canon({(1, 2): 1, (1, 3): 1, (2, 4): 1, (3, -4): 1}), 4) == []   # ... to the sink in its two orientations
    assert call(canon({(1, -1): 1, (1, 2): 1, (2, 4): 1, (-1, 4): 1}), 4) == []  # a link that is its own strand mate at the source
    assert call(canon({(1, 1): 1, (1, 2): 1, (1, 3): 1, (2, 4): 1, (3, 4): 1}), 4) == [] and call(canon({(1, 1): 1, (1, 2): 1, (2, 4): 1}), 4) == []   # a link (a, a)
    assert call(canon({(1, 2): 1, (1, 3): 1, (2, 1): 1, (3, 1): 1}), 3) == []    # the sink is the source
    assert call(canon({(1, 2): 1, (1, -2): 1, (2, 3): 1, (-2, 3): 1}), 3) == []  # the branches are one unitig on its two strands
    assert call(canon({(1, 2): 1, (1, 3): 1, (2, 3): 1, (3, 3): 1}), 3) == []


def test_min_link_and_wide_counts():
    three = {**ONE, (1, 5): 1, (1, 3): 2, (3, 4): 2, **canon({(5, 4): 1})}
    assert call(three, 5) == [] and call(three, 5, 2) == [(1, 4, (2, 3), (7, 6, 2, 2))] and call(three, 5, 3) == []   # a three-way site that min_link prunes into a bubble, then destroys
    assert call(ONE, 4, 2) == [] and call(ONE, 4, 1) != []   # a bubble that min_link destroys
    wide = {(1, 2): BIG + 5, (1, 3): 2 ** 64 - 1, (2, 4): BIG, (3, 4): 3 * BIG + 1}
    assert call(wide, 4, BIG) == [(1, 4, (2, 3), (BIG + 5, BIG, 2 ** 64 - 1, 3 * BIG + 1))] and call(wide, 4, BIG + 1) == []
    assert call(wide, 4, 2 ** 64 - 1) == []


def test_degenerate_sizes():
    assert call({}, 4) == [] and call({}, 1) == [] and call({}, 0) == []
    assert call({(1, 1): 3}, 1) == [] and call({(1, -1): 3}, 1) == [] and call(canon({(1, 1): 3, (1, -1): 2, (-1, 1): 9}), 1) == []   # n_unitigs = 1
    n = B.C.c_uint64(9)
    arr = np.array(K.sorted_links(ONE), dtype=B.LINK_DTYPE)
    assert B.lib().bgr_links_bubbles(0, arr.ctypes.data, 4, 4, 1, None, 0, B.C.byref(n)) == -4 and n.value == 1   # a small cap: BGR_E_CAPACITY and the right n


def _seams():
    """1 500 bubbles on 6 000 unitigs (every unitig in one of them), random orientations and counts; the unitig whose negative id is the last
    oriented id of the first tile is a source"""
    rnd = random.Random(99)
    n = 6000
    last = TILE // 2   # o(-last) = TILE - 1
    rest = [x for x in range(1, n + 1) if x != last]
    rnd.shuffle(rest)
    big = next(i for i, x in enumerate(rest) if x > last)
    quads = [(-last, rest.pop(big) * rnd.choice((1, -1)))]   # (source, sink): |sink| is the larger, so this side is the one reported
    quads[0] += (rest.pop() * rnd.choice((1, -1)), rest.pop() * rnd.choice((1, -1)))
    while rest:
        s, t, b, c = (rest.pop() * rnd.choice((1, -1)) for _ in range(4))
        quads.append((s, t, b, c))
    counts = {}
    for s, t, b, c in quads:
        for l in ((s, b), (s, c), (b, t), (c, t)):
            counts[K.canonical(*l)] = rnd.choice((1, 2, 3, 50, BIG + rnd.randint(0, 9)))
    return n, counts


def test_tile_seams():
    """the oriented ids span twelve tiles: the order, the ranks inside a tile and the offsets across the tiles of the compaction all show"""
    n, counts = _seams()
    assert 2 * n > 11 * TILE
    for min_link in (1, 3):
        got = call(counts, n, min_link)
        assert len(got) == (1500 if min_link == 1 else len(BR.bubbles_of(counts, 3))) and 0 < len(BR.bubbles_of(counts, 3)) < 1500
        tiles = [BR.okey(s)[0] * 2 - 2 + (s < 0) for s, _, _, _ in got]
        assert tiles == sorted(tiles) and len({o // TILE for o in tiles}) == 12   # every tile holds sources
    assert any(s == -(TILE // 2) for s, _, _, _ in call(counts, n))   # the last oriented id of the first tile
    assert sum(1 for s, _, _, _ in call(counts, n) if s < 0) > 500
    # a graph that ends one oriented id behind a tile, with a bubble on its last unitigs
    m = TILE // 2 + 1
    assert call(canon({(m - 3, m - 2): 1, (m - 3, m - 1): 2, (m - 2, -m): 3, (m - 1, -m): 4}), m) == [(m - 3, -m, (m - 2, m - 1), (1, 3, 2, 4))]
    assert call(canon({(-m, m - 2): 1, (-m, m - 1): 2, (m - 2, m - 3): 3, (m - 1, m - 3): 4}), m) == [(-(m - 3), m, (-(m - 2), -(m - 1)), (3, 1, 4, 2))]


def _synth(alleles, k, seed=4):
    s = Synth(3000, 120, alleles, k, seed)
    seqs, offs = s.unitigs()
    rb, ro = s.reads(0, 2000, 150, 2, seed + 1)
    return s, seqs, offs, rb, ro


def _ref_rows(k, seqs, offs, rb, ro):
    if k > 32:
        return W.GreedyRef(k, strings(seqs, offs)).align(strings(rb, ro), 2, 2)[0]
    return W.rows_of(*oracle_py.Oracle(k, seqs, offs).align(rb, ro, m=2, effort=2))


@pytest.mark.parametrize("small_table", [False, True])
@pytest.mark.parametrize("k", [15, 31, 33])
def test_aligner_bubbles(k, small_table):
    """the aligner's live table, filled by several launches: bubbles_ref over bgr_aligner_links and over links_ref of the rows (which are the
    oracle's; wide_greedy_ref's for k = 33); a table of another size holds the links in another slot order"""
    s, seqs, offs, rb, ro = _synth(2, k)
    n_unitigs = len(offs) - 1
    g = B.Graph.build(k, seqs, offs)
    with B.options(**({"test.links_capacity": 256} if small_table else {})):
        al = B.Aligner(g, 0)
        al.links_enable()
    assert (al.links_info()["capacity"] == 256) == small_table
    with pytest.raises(B.BgrError, match="error -1.*min_link"):
        al.bubbles(0)
    assert len(al.bubbles()) == 0   # an empty table
    rows = []
    for lo, hi in ((0, 1), (1, 700), (700, 2000)):   # ragged launches
        rows += W.rows_of(*al.align(rb[int(ro[lo]):int(ro[hi])], ro[lo:hi + 1] - ro[lo], m=2, effort=2))
    assert rows == _ref_rows(k, seqs, offs, rb, ro)
    counts = K.links_of(rows, n_unitigs)
    links = al.links()
    assert {(int(r["from"]), int(r["to"])): int(r["count"]) for r in links} == counts and al.links_info()["overflow"] == 0
    us = [""] + strings(seqs, offs)
    for min_link in (1, 2, 5):
        want = BR.bubbles_of(counts, min_link)
        assert len(want) > 0   # (23 on these graphs at every threshold, all of them SNV-shaped: checked on the CPU)
        got = al.bubbles(min_link)
        assert BR.as_tuples(got) == want, (k, min_link)
        assert all(BR.compare(BR.oriented(us, b), BR.oriented(us, c))[0] == "snv" and len(us[abs(b)]) == 2 * k - 1 for _, _, (b, c), _ in want)
        assert B.links_bubbles(links, n_unitigs, min_link).tobytes() == got.tobytes()   # the list arrives in key order, the table in slot order: the same bytes
    ms = al.bubbles_times()
    assert len(ms) == 4 and all(x > 0 for x in ms)
    assert BR.as_tuples(al.bubbles(10 ** 9)) == [] and al.bubbles_times()[3] == 0   # nothing to emit: three launches
    n = B.C.c_uint64(0)
    buf = np.zeros(3, dtype=B.BUBBLE_DTYPE)
    assert B.lib().bgr_aligner_bubbles(al.h, 1, buf.ctypes.data, 3, B.C.byref(n)) == -4 and n.value == len(BR.bubbles_of(counts)) and not buf["count"].any()


def test_three_alleles_per_site_give_none():
    s, seqs, offs, rb, ro = _synth(3, 31)
    g = B.Graph.build(31, seqs, offs)
    al = B.Aligner(g, 0)
    al.links_enable()
    rows = W.rows_of(*al.align(rb, ro, m=2, effort=2))
    counts = K.links_of(rows, len(offs) - 1)
    assert len(counts) > 100 and BR.bubbles_of(counts) == [] and len(al.bubbles()) == 0 and len(B.links_bubbles(al.links(), len(offs) - 1)) == 0


def test_aligner_refusals():
    s, seqs, offs, rb, ro = _synth(2, 31)
    g = B.Graph.build(31, seqs, offs)
    al = B.Aligner(g, 0)
    with pytest.raises(B.BgrError, match="error -1.*never enabled"):
        al.bubbles()
    with B.options(**{"test.links_capacity": 64}):   # 92 links do not fit: the overflow word is set, the counts are incomplete
        small = B.Aligner(g, 0)
        small.links_enable()
    small.align(rb, ro, m=2, effort=2)
    assert small.links_info()["overflow"] > 0
    with pytest.raises(B.BgrError, match="error -4.*was full"):
        small.bubbles()


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------
def run(args, flags=("bubbles", "gfa"), more=(), timeout=600, check=True):
    """the CLI in a scratch directory -> (return code, stdout, stderr, paths bytes -- the pairs of a split run concatenated --, notAligned bytes,
    bubbles bytes or None, GFA bytes or None)"""
    d = tempfile.mkdtemp()
    try:
        files = [x for f in flags for x in ("--" + f, os.path.join(d, "out." + f))]
        p = subprocess.run([B.CLI_PATH] + list(args) + files + list(more), cwd=d, capture_output=True, text=True, timeout=timeout)
        if check and p.returncode != 0:
            raise RuntimeError("%s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
        def cat(name):
            if os.path.exists(os.path.join(d, name + ".0")):
                return b"".join(open(os.path.join(d, "%s.%d" % (name, i)), "rb").read() for i in range(8) if os.path.exists(os.path.join(d, "%s.%d" % (name, i))))
            return open(os.path.join(d, name), "rb").read() if os.path.exists(os.path.join(d, name)) else None
        return p.returncode, p.stdout, p.stderr, cat("paths") or b"", cat("notAligned.fa") or b"", cat("out.bubbles"), cat("out.gfa")
    finally:
        shutil.rmtree(d)


@pytest.fixture(scope="module")
def synth_files():
    """unitigs and reads of the two-allele graph as files, and what a run without the flag writes"""
    d = tempfile.mkdtemp()
    s = Synth(3000, 120, 2, 31, 4)
    s.write_unitigs(os.path.join(d, "u.fa"))
    s.write_reads(os.path.join(d, "r.fa"), 0, 2000, 150, 2, 5)
    args = ["-r", os.path.join(d, "r.fa"), "-k", "31", "-g", os.path.join(d, "u.fa"), "-m", "2", "-e", "2"]
    _, out, _, paths, na, _, _ = run(args, flags=())
    yield args, G.load_unitigs(os.path.join(d, "u.fa"), 31), out, paths, na
    shutil.rmtree(d)


LANES = ["--gpus", "2", "--set", "test.lanes_on_one_device=1"]


@pytest.mark.parametrize("extra", [[], ["--host-route"], ["-t", "5", "--batch", "37", "--chunk-bytes", "600"], LANES, LANES + ["--split-output"]], ids=["plain", "host", "small", "lanes", "split"])
def test_cli_bubbles_with_gfa(synth_files, extra):
    """the file = bubbles_ref over the L lines of the same run's GFA; paths, notAligned.fa and the counters are those of a run without the flag"""
    args, us, out0, paths0, na0 = synth_files
    _, out, _, paths, na, bub, gfa = run(args + extra)
    _, _, links = K.parse_gfa(gfa)
    want = BR.bubbles_of(links)
    assert len(want) > 10 and bub == BR.bubbles_text(us, want) and b"\tsnv\t30:" in bub
    assert paths == paths0 and na == na0 and parse_counters(out) == parse_counters(out0)
    _, _, _, _, _, bub5, gfa5 = run(args + extra, more=["--min-link", "5"])
    assert gfa5 == gfa and bub5 == BR.bubbles_text(us, BR.bubbles_of(links, 5))
    assert run(args + extra, more=["--min-link", "999999999"])[5] == BR.bubbles_text(us, [])


def test_cli_bubbles_alone_changes_nothing_else(synth_files):
    """without --gfa: the same file; stdout too is what it is without the flag"""
    args, us, out0, paths0, na0 = synth_files
    _, out, _, paths, na, bub, gfa = run(args, flags=("bubbles",))
    both = run(args)
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
    assert gfa is None and bub == both[5] and len(bub.split(b"\n")) > 12 and strip(out) == strip(out0) and paths == paths0 and na == na0


@pytest.mark.parametrize("case", CASES, ids=["%02d-%s" % (c["id"], c["group"]) for c in CASES])
def test_cli_bubbles_on_the_goldens(case):
    """the file = bubbles_ref over links_ref of the oracle's rows (most of these graphs hold no bubble: the header alone); paths, notAligned.fa and
    the counters stay the golden's.  A graph with non-ACGT unitig characters is refused; a run that ends with "bug compaction" writes no file"""
    a, us, H, R, rows = golden_rows(case)
    rc, out, err, paths, na, bub, _ = run(resolve_args(case["args"]), flags=("bubbles",), check=False)
    if a["graph"] in EXC_GRAPHS:
        assert rc == 2 and "--bubbles" in err and "ACGT" in err and bub is None, (case["args"], err[-300:])
        return
    assert rc == 0, err[-500:]
    if not case["counters"]:
        assert bub is None and "bug compaction" in out and parse_counters(out) == {}, case["args"]
        return
    assert bub == BR.bubbles_text(us, BR.bubbles_of(K.links_of(rows, len(us) - 1))), case["args"]
    assert parse_counters(out) == case["counters"] and len(paths) == case["paths_len"] and sha(paths) == case["paths_sha256"], case["args"]
    assert len(na) == case["notaligned_len"] and sha(na) == case["notaligned_sha256"], case["args"]


def test_cli_refusals(tmp_path):
    base = [B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5"]
    f = str(tmp_path / "x.bubbles")
    def cli(graph, *more):
        return subprocess.run(base + ["-g", os.path.join(GOLD, graph)] + list(more), cwd=tmp_path, capture_output=True, text=True, timeout=300)
    pr = cli("deg_unitig.fa", "--bubbles", f, "-b")
    assert pr.returncode == 2 and "--bubbles" in pr.stderr and "-b" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig_exc.fa", "--bubbles", f)
    assert pr.returncode == 2 and "--bubbles" in pr.stderr and "ACGT" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    for bad in ("0", "x", "", "-1", "1.5", "1234567890", "00000000000", " 2"):
        pr = cli("deg_unitig.fa", "--bubbles", f, "--min-link", bad)
        assert pr.returncode == 2 and "--min-link" in pr.stderr and not os.path.exists(f), (bad, pr.stderr[-500:])
    pr = cli("deg_unitig.fa", "--min-link", "2")   # the threshold without --bubbles
    assert pr.returncode == 2 and "--bubbles" in pr.stderr, pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--bubbles", f, "--min-link", "000000002")   # nine digits
    assert pr.returncode == 0 and os.path.exists(f), pr.stderr[-500:]


def test_align_all_keeps_the_bubbles_in_the_graph(synth_files, tmp_path):
    args, us, _, _, _ = synth_files
    g = B.Graph.from_fasta(args[5], 31)
    P, N = str(tmp_path / "p"), str(tmp_path / "n")
    with pytest.raises(B.BgrError):
        g.bubbles()
    g.bubbles_enable(min_link=2)
    B.align_all(g, args[1], P, N, m=2, effort=2, threads=2)
    counts = {(int(r["from"]), int(r["to"])): int(r["count"]) for r in g.links()}   # the switch implies the links
    want = BR.bubbles_of(counts, 2)
    assert len(want) > 10 and BR.as_tuples(g.bubbles()) == want
    B.write_bubbles(str(tmp_path / "b"), g, g.bubbles())
    assert open(tmp_path / "b", "rb").read() == BR.bubbles_text(us, want)
    g.bubbles_enable(False)
    B.align_all(g, args[1], P, N, m=2, effort=2)   # a run with the switch off leaves the records alone
    assert BR.as_tuples(g.bubbles()) == want
    g.bubbles_enable()
    B.align_all(g, args[1] + "," + args[1], P, N, m=2, effort=2, route=1)   # the next such run replaces them
    assert BR.as_tuples(g.bubbles()) == BR.bubbles_of({l: 2 * c for l, c in counts.items()}, 1)
    with pytest.raises(B.BgrError):   # a run that fails leaves none
        B.align_all(g, str(tmp_path / "missing.fa"), P, N)
    with pytest.raises(B.BgrError):
        g.bubbles()
