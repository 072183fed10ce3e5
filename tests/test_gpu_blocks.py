"""Haplotype blocks on the GPU machine: crafted lists of bubbles and phase records (blocks_gen.py) through bgr_phase_blocks, every entry against
blocks_ref.py (the definition in plain Python, which test_blocks_host.py makes check itself); malformed lists, which are refused in ordinary code
paths; `--blocks` through the CLI next to `--bubbles --phase --triples --gfa` of the same run, and the entries bgr_align_all keeps in the graph."""
import os
import random
import subprocess

import numpy as np
import pytest

import bgreat_amd as B
import blocks_gen as G
import blocks_ref as R
import phase_ref as P
from test_gpu_phase import parse_bubbles
from test_gpu_triples import ROUTE_IDS, ROUTES, run, synth_files   # noqa: F401 (synth_files is a fixture)
from util import GOLD, parse_counters

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -4


def mixed(n, rng, longest=70, rings=True):
    """shapes of n bubbles in all: paths of 1 .. longest, now and then a ring"""
    shapes = []
    while n:
        size = min(n, rng.randrange(1, longest + 1))
        shapes.append(("ring" if rings and size >= 2 and rng.random() < 0.15 else "path", size))
        n -= size
    rng.shuffle(shapes)
    return shapes


def check(shapes, seed, min_phases=(1,), **kw):
    """the crafted input through the device against the definition -> the entries of the last threshold"""
    bubbles, phase, n_unitigs = G.make(shapes, seed, **kw)
    ba, pa = G.bubbles_array(B, bubbles), G.phase_array(B, phase)
    for min_phase in min_phases:
        got = B.phase_blocks(ba, pa, n_unitigs, min_phase)
        want = R.blocks_of(bubbles, phase, min_phase)
        assert len(got) == len(bubbles) and R.as_tuples(got) == want, (shapes[:5], seed, min_phase)
    return want


@pytest.mark.parametrize("n", [0, 1, 2, 3, 31, 32, 33, 511, 512, 513, 4099])
def test_wave_and_tile_seams(n):
    """the tile is 1 024 nodes = 512 bubbles, a wave 64 nodes: a mix of paths and rings at every seam; one chain through all bubbles (the deepest
    jumping); chains of 2 only; no links at all"""
    rng = random.Random(n)
    check(mixed(n, rng), n, undecided=0.1)
    if n:
        want = check([("path", n)], n + 1)
        assert want[-1][:3] == (1, n - 1, n)
        want = check([("path", 1)] * n, n + 2)
        assert want[-1][0] == n
    if n >= 2:
        want = check([("path", 2)] * (n // 2) + [("path", 1)] * (n % 2), n + 3)
        assert want[-1][0] == (n + 1) // 2
        check([("ring", n)], n + 4)


@pytest.mark.parametrize("parity", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("length", [2, 3, 64, 1500])
def test_rings(length, parity):
    """one ring and nothing else -- one block, every line, the ring's and its mate ring's order decided by one node index -- and rings among paths;
    the random signs and the permutation put the smallest node into either reading"""
    for seed in range(6 if length < 100 else 1):
        want = check([("ring", length)], 100 * length + seed, ring_parity=parity)
        assert len(want) == length and {e[4] & (R.CIRCULAR | R.CONFLICT) for e in want} == {R.CIRCULAR | (R.CONFLICT if parity else 0)}
    check([("ring", length), ("path", 5), ("ring", length), ("path", 1), ("ring", 2)], length, ring_parity=parity)


def test_undecided_records_and_thresholds():
    """undecided records interleaved with decided ones; min_phase of 1, 2 and above every difference the generator makes (3), where nothing is joined"""
    rng = random.Random(77)
    want = check(mixed(1200, rng), 77, min_phases=(1, 2, 4), undecided=0.4, big=0.1)
    assert [e[:3] for e in want] == [(i + 1, 0, 1) for i in range(1200)]
    check(mixed(700, rng, rings=False), 78, min_phases=(3, 2 ** 64 - 1), undecided=0.5)
    check([("path", 40)], 79, spare=5000)   # a graph much larger than the bubbles' ids


def raw_call(ba, pa, n_unitigs, min_phase, cap):
    out = np.zeros(max(cap, 1), dtype=B.BLOCK_DTYPE)
    n = B.C.c_uint64(12345)
    rc = B.lib().bgr_phase_blocks(0, ba.ctypes.data if len(ba) else None, len(ba), pa.ctypes.data if len(pa) else None, len(pa), n_unitigs, min_phase, out.ctypes.data if cap else None, cap,
                                  B.C.byref(n))
    return rc, int(n.value), out, B.lib().bgr_last_error().decode()


def test_capacity_and_arguments():
    bubbles, phase, n_unitigs = G.make([("path", 9), ("ring", 4)], 5)
    ba, pa = G.bubbles_array(B, bubbles), G.phase_array(B, phase)
    rc, n, out, msg = raw_call(ba, pa, n_unitigs, 1, 12)
    assert rc == E_CAPACITY and n == 13 and not out.view(np.uint32).any() and "13" in msg
    rc, n, out, msg = raw_call(ba, pa, n_unitigs, 1, 0)
    assert rc == E_CAPACITY and n == 13
    rc, n, out, msg = raw_call(ba, pa, n_unitigs, 1, 13)
    assert rc == 0 and n == 13 and R.as_tuples(out[:13]) == R.blocks_of(bubbles, phase)
    t = B.phase_blocks_times()
    assert t["total"] > 0 and t["total"] >= t["link"] + t["rank"] + t["place"] > 0
    rc, n, out, msg = raw_call(ba, pa, n_unitigs, 0, 13)
    assert rc == E_ARG and n == 0 and "min_phase" in msg and not out.view(np.uint32).any()
    rc, n, out, msg = raw_call(ba[:0], pa[:0], n_unitigs, 1, 0)   # no bubbles: no device work
    assert rc == 0 and n == 0 and B.phase_blocks_times() == dict(link=0.0, rank=0.0, place=0.0, total=0.0)


def test_malformed_lists_are_refused_and_the_next_call_passes():
    """each of these is BGR_E_ARG with nothing copied, found by the host's checks or by the index and link passes' own -- and the process goes on"""
    ONES = (1, 1, 1, 1)
    CIS = (5, 0, 0, 5)
    good = [(1, 4, (2, 3), ONES), (4, 7, (5, 6), ONES), (8, 11, (9, 10), ONES)]
    rec = (4, 1, (2, 3), (5, 6), 7, CIS)
    def refused(bubbles, phase, n_unitigs, word):
        rc, n, out, msg = raw_call(G.bubbles_array(B, bubbles), G.phase_array(B, phase), n_unitigs, 1, len(bubbles))
        assert rc == E_ARG and word in msg and not out.view(np.uint32).any(), (rc, msg)
        assert R.as_tuples(B.phase_blocks(G.bubbles_array(B, good), G.phase_array(B, [rec]), 11)) == [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0), (2, 0, 1, 2, 0)]
    # two records with one source: as given (the host's check), and as mates -- (1, 9) and (5, 9) both read (-9, ...) backwards (the index pass)
    refused([good[0], (1, 5, (6, 7), ONES), good[2]], [], 11, "ascending")
    refused([(1, 9, (2, 3), ONES), (5, 9, (6, 7), ONES)], [], 11, "leave one oriented unitig")
    # a phase record whose source has no bubble; one whose `in` does not match; one whose sink does not; two records out of one bubble
    refused(good, [(4, 12, (2, 3), (5, 6), 7, CIS)], 12, "opens no bubble")
    refused(good, [(4, 1, (2, 12), (5, 6), 7, CIS)], 12, "are not those of the bubbles")
    refused(good, [(4, 1, (2, 3), (5, 6), 8, CIS)], 12, "are not those of the bubbles")
    assert R.as_tuples(B.phase_blocks(G.bubbles_array(B, good), G.phase_array(B, [(4, 12, (2, 3), (5, 6), 7, (1, 1, 1, 1))]), 12)) == [(1, 0, 1, 0, 0), (2, 0, 1, 1, 0), (3, 0, 1, 2, 0)]   # (undecided: not looked at)
    # an id beyond n_unitigs, in either list; an id that is none
    refused(good, [rec], 10, "beyond n_unitigs")
    refused(good[:2], [(4, 1, (2, 3), (5, 6), 8, CIS)], 7, "beyond n_unitigs")
    refused([good[0], (4, 7, (0, 6), ONES)], [], 11, "beyond n_unitigs")
    # an unsorted list, a reading that is not canonical, branches out of order, phase records out of order
    refused([good[1], good[0], good[2]], [], 11, "ascending")
    refused([good[0], (7, 4, (5, 6), ONES)], [], 11, "canonical")
    refused([good[0], (4, 7, (6, 5), ONES)], [], 11, "order")
    refused(good, [rec, rec], 11, "ascending")


# ---- the CLI and the run ----------------------------------------------------------------------------------------------------------------------
FLAGS = ("blocks", "bubbles", "phase", "triples", "gfa")


def bubble_records(b):
    return [(k[0], k[1], (k[2], k[3]), v) for k, v in parse_bubbles(b).items()]


def text_of(bubbles_bytes, phase_bytes, min_phase=1):
    bubbles = bubble_records(bubbles_bytes)
    return R.blocks_text(bubbles, R.blocks_of(bubbles, P.parse_text(phase_bytes), min_phase))


@pytest.mark.parametrize("extra", ROUTES, ids=ROUTE_IDS)
def test_cli_blocks_with_bubbles_phase_triples_and_gfa(synth_files, extra):
    """the bytes = blocks_ref over the parsed bubbles and phase files of the same run; paths, notAligned.fa and the counters are those of a run
    without any flag; --min-phase and --min-link reach the run"""
    args, us, plain, rows = synth_files
    r = run(args + extra, flags=FLAGS)
    assert r["blocks"] == text_of(r["bubbles"], r["phase"])
    entries = R.blocks_of(bubble_records(r["bubbles"]), P.parse_text(r["phase"]))
    multi = sum(1 for e in entries if e[1] == 0 and e[2] > 1)
    assert multi >= 2, "the synthetic files yield %d blocks of more than one bubble: the crafted lists (above) are the coverage of the chaining" % multi
    assert r["blocks"].count(b"\n") == 1 + r["bubbles"].count(b"\n") - 1
    assert r["paths"] == plain["paths"] and r["na"] == plain["na"] and parse_counters(r["out"]) == parse_counters(plain["out"])
    r3 = run(args + extra, flags=FLAGS, more=["--min-phase", "3", "--min-link", "2"])
    assert r3["blocks"] == text_of(r3["bubbles"], r3["phase"], 3)
    rn = run(args + extra, flags=FLAGS, more=["--min-phase", "999999999"])
    assert rn["blocks"] == text_of(r["bubbles"], r["phase"], 999999999) and rn["phase"] == r["phase"]
    assert all(ln.split("\t")[2] == "1" for ln in rn["blocks"].decode().splitlines()[1:])


def test_cli_blocks_alone_changes_nothing_else(synth_files):
    """without the other flags: the same file, and stdout too is what it is without the flag"""
    args, us, plain, rows = synth_files
    alone = run(args, flags=("blocks",))
    both = run(args, flags=FLAGS)
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
    assert alone["blocks"] == both["blocks"] and strip(alone["out"]) == strip(plain["out"])
    assert alone["paths"] == plain["paths"] and alone["na"] == plain["na"]
    a3 = run(args, flags=("blocks",), more=["--min-link", "3"])   # alone, the threshold of the bubbles is the blocks' own
    b3 = run(args, flags=FLAGS, more=["--min-link", "3"])
    assert a3["blocks"] == b3["blocks"] == text_of(b3["bubbles"], b3["phase"])
    an = run(args, flags=("blocks",), more=["--min-link", "999999999"])   # no link is supported: no bubble, no block
    assert an["blocks"] == R.HEADER.encode() and an["paths"] == plain["paths"]


def test_cli_refusals(tmp_path):
    base = [B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5"]
    f = str(tmp_path / "x.blocks")
    def cli(graph, *more):
        return subprocess.run(base + ["-g", os.path.join(GOLD, graph)] + list(more), cwd=tmp_path, capture_output=True, text=True, timeout=300)
    pr = cli("deg_unitig.fa", "--blocks", f, "-b")
    assert pr.returncode == 2 and "--blocks" in pr.stderr and "-b" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig_exc.fa", "--blocks", f)
    assert pr.returncode == 2 and "--blocks" in pr.stderr and "ACGT" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--min-phase", "2")   # the threshold alone
    assert pr.returncode == 2 and "--min-phase" in pr.stderr, pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--phase", str(tmp_path / "x.phase"), "--min-phase", "2")   # ... is none of --phase
    assert pr.returncode == 2 and "--min-phase" in pr.stderr and not os.path.exists(tmp_path / "x.phase"), pr.stderr[-500:]
    for bad in ("0", "x", "1234567890", "-1", ""):
        pr = cli("deg_unitig.fa", "--blocks", f, "--min-phase", bad)
        assert pr.returncode == 2 and "--min-phase" in pr.stderr and not os.path.exists(f), (bad, pr.stderr[-500:])
    pr = cli("deg_unitig.fa", "--blocks", f, "--min-link", "0")
    assert pr.returncode == 2 and "--min-link" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--blocks", f, "--min-phase", "2", "--min-link", "2")
    assert pr.returncode == 0 and open(f, "rb").read().startswith(R.HEADER.encode()), pr.stderr[-500:]


def test_align_all_keeps_the_blocks_in_the_graph(synth_files, tmp_path):
    args, us, _, rows = synth_files
    g = B.Graph.from_fasta(args[5], 31)
    PF, NF = str(tmp_path / "p"), str(tmp_path / "n")
    with pytest.raises(B.BgrError):
        g.blocks()
    for kw in (dict(min_phase=0), dict(min_link=0)):
        with pytest.raises(B.BgrError):
            g.blocks_enable(**kw)
    g.blocks_enable(min_link=2, min_phase=2)
    assert g.blocks_enabled() and not g.phase_enabled() and not g.bubbles_enabled() and not g.triples_enabled() and not g.links_enabled()
    B.align_all(g, args[1], PF, NF, m=2, effort=2, threads=2)
    bubbles, phase = g.bubbles(), g.phase()   # the switch implies the phase's, and with it the links, the bubbles and the triples
    import bubbles_ref as BR
    counts = {(int(r["from"]), int(r["to"])): int(r["count"]) for r in g.links()}
    assert BR.as_tuples(bubbles) == BR.bubbles_of(counts, 2) and len(bubbles) > 10 and len(phase) > 10
    want = R.blocks_of(BR.as_tuples(bubbles), P.as_tuples(phase), 2)
    assert R.as_tuples(g.blocks()) == want
    assert R.as_tuples(B.phase_blocks(bubbles, phase, len(us) - 1, 2)) == want   # the library call over what the graph delivers
    B.write_blocks(str(tmp_path / "bl"), g, bubbles, g.blocks())
    cli = run(args, flags=("blocks",), more=["--min-link", "2", "--min-phase", "2"])
    assert open(tmp_path / "bl", "rb").read() == R.blocks_text(BR.as_tuples(bubbles), want) == cli["blocks"]
    bad = g.blocks().copy()
    bad["bubble"][0] = len(bubbles)
    with pytest.raises(B.BgrError, match="error -1.*names no bubble"):
        B.write_blocks(str(tmp_path / "bl2"), g, bubbles, bad)
    g.blocks_enable(False)
    B.align_all(g, args[1], PF, NF, m=2, effort=2)   # a run with the switch off leaves the kept entries alone
    assert R.as_tuples(g.blocks()) == want
    g.blocks_enable()
    with pytest.raises(B.BgrError):   # a run that fails leaves none
        B.align_all(g, str(tmp_path / "missing.fa"), PF, NF)
    with pytest.raises(B.BgrError):
        g.blocks()


def test_a_run_takes_each_threshold_from_the_first_switch_that_is_on(tmp_path):
    """several switches of the chain with different thresholds: the run's bubbles are called with the min_link of the first switch that is on in the
    order bubbles, phase, blocks, haplotypes; its blocks are chained with the blocks' min_phase, or with the haplotypes' when only that switch is on.
    Every run against the bubbles and blocks recomputed from its own links and phase records with the expected thresholds.  The reads are those of two
    planted haplotypes at a depth of four each (the synthetic files' links all have counts beyond 10: no threshold of 1 .. 3 tells on them), where
    min_link 1, 2 and 3 call 55, 37 and 18 bubbles and min_phase 1 and 2 chain different blocks (counted on the CPU, and asserted below)"""
    import bubbles_ref as BR
    from test_gpu_haplotypes import planted
    haps, unitigs, reads = planted(2, coverage=8, genome_len=9000, n_sites=60)
    uf, rf, PF, NF = (str(tmp_path / x) for x in ("u.fa", "r.fa", "p", "n"))
    open(uf, "w").write("".join(">u%d\n%s\n" % (i, u) for i, u in enumerate(unitigs)))
    open(rf, "w").write("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    runs = [   # the switches of the run, the min_link and the min_phase (None: the run chains no blocks) it has to use
        (dict(bubbles=dict(min_link=1), haplotypes=dict(min_link=3, min_phase=2)), 1, 2),
        (dict(phase=dict(min_link=2), blocks=dict(min_link=3)), 2, 1),
        (dict(blocks=dict(min_link=2, min_phase=1), haplotypes=dict(min_link=9, min_phase=2)), 2, 1),
        (dict(haplotypes=dict(min_link=2, min_phase=2)), 2, 2),
        (dict(bubbles=dict(min_link=3), phase=dict(min_link=1)), 3, None),
        (dict(phase=dict(min_link=3)), 3, None),
    ]
    seen = {}
    for switches, min_link, min_phase in runs:
        g = B.Graph.from_fasta(uf, 31)
        for name, kw in switches.items():
            getattr(g, name + "_enable")(**kw)
        B.align_all(g, rf, PF, NF, m=2, effort=2, threads=2)
        bubbles, phase = BR.as_tuples(g.bubbles()), P.as_tuples(g.phase())
        seen[min_link] = BR.as_tuples(B.links_bubbles(g.links(), len(unitigs), min_link=min_link))
        assert bubbles == seen[min_link], (switches, min_link)
        if min_phase is None:
            with pytest.raises(B.BgrError):
                g.blocks()
        else:
            want = R.blocks_of(bubbles, phase, min_phase)
            assert R.as_tuples(g.blocks()) == want, (switches, min_phase)
            assert want != R.blocks_of(bubbles, phase, 3 - min_phase), "min_phase 1 and 2 chain the same blocks: the run cannot tell the rules apart"
        g.close()
    assert [len(seen[m]) for m in (1, 2, 3)] == [55, 37, 18], "min_link 1, 2 and 3 have to call three different lists of bubbles"
