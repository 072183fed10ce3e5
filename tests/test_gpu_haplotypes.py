"""The haplotypes' sequences on the GPU machine: crafted lists of bubbles (blocks_gen.py) with blocks_ref's entries over graphs of random unitigs
through bgr_blocks_haplotypes, every record, byte and the bad-junction count against haplotypes_ref.py (the definition in plain Python, which
test_haplotypes_host.py makes check itself); capacities and malformed input, which are refused in ordinary code paths; two planted haplotypes end to
end -- the one check that does not rest on the Python restatement --; `--haplotypes` through the CLI next to `--bubbles --blocks` of the same run, and
the records bgr_align_all keeps in the graph."""
import os
import random
import subprocess

import numpy as np
import pytest

import bgreat_amd as B
import blocks_gen as G
import blocks_ref as R
import bubbles_ref as BR
import haplotypes_ref as H
import phase_ref as P
from test_gpu_phase import parse_bubbles
from test_gpu_triples import ROUTE_IDS, ROUTES, run, synth_files   # noqa: F401 (synth_files is a fixture)
from util import GOLD, parse_counters

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -4
N_MAX = 513                      # bubbles of the largest crafted list
N_UNITIGS = 4 * N_MAX + 8        # what a list of N_MAX blocks of one names (four ids each), and a few more
LONG = 70001                     # one unitig that spans many output tiles of 16 384 bytes
_graphs = {}


def crafted_graph(k):
    """random unitigs of mixed lengths (none below k: the graph ends at the first shorter one), the long one at id 2 so that every list names it
    -> (graph resident on device 0, unitigs with "" at 0); built once per k"""
    if k not in _graphs:
        rng = random.Random(1000 + k)
        lengths = [x for x in (k, k + 1, 2 * k - 1, 33, 64, 65, 200, 317) if x >= k]
        us = [""] + ["".join(rng.choice("ACGT") for _ in range(LONG if i == 2 else rng.choice(lengths))) for i in range(1, N_UNITIGS + 1)]
        offs = np.cumsum([0] + [len(u) for u in us[1:]]).astype(np.uint64)
        g = B.Graph.build(k, "".join(us).encode(), offs)
        assert g.info()["n_unitigs"] == N_UNITIGS
        g.upload(0)
        _graphs[k] = (g, us)
    return _graphs[k]


def arrays(bubbles, entries):
    ea = np.zeros(len(entries), dtype=B.BLOCK_DTYPE)
    for i, e in enumerate(entries):
        ea[i] = e + (0,)
    return G.bubbles_array(B, bubbles), ea


def piece_bases(us, k, walks):
    """where the reference's pieces begin in the graph's 2-bit store: unitig i's forward strand at F = 2 * (the lengths before it), its reverse
    complement right behind; every unitig of a walk but the first without its first k - 1 bases"""
    F = np.concatenate(([0, 0], 2 * np.cumsum([len(u) for u in us[1:]])))
    out = set()
    for w in walks:
        for j, x in enumerate(w):
            out.add(int(F[abs(x)]) + (len(us[abs(x)]) if x < 0 else 0) + (k - 1 if j else 0))
    return out


def check(k, shapes, seed, min_blocks=(1,), seen=None, **kw):
    """the crafted input through the device against the definition"""
    g, us = crafted_graph(k)
    bubbles, phase, n_unitigs = G.make(shapes, seed, **kw)
    assert n_unitigs <= N_UNITIGS
    entries = R.blocks_of(bubbles, phase)
    ba, ea = arrays(bubbles, entries)
    for min_block in min_blocks:
        want_recs, want_bytes, want_bad, walks = H.haplotypes_of(us, k, bubbles, entries, min_block)
        recs, seq, bad = B.blocks_haplotypes(g, ba, ea, min_block)
        assert H.as_tuples(recs) == want_recs, (k, shapes[:5], seed, min_block)
        assert seq.tobytes() == want_bytes, (k, shapes[:5], seed, min_block)
        assert bad == want_bad, (k, shapes[:5], seed, min_block)
        if seen is not None:
            seen[0] |= {b % 32 for b in piece_bases(us, k, walks)}
            seen[1] |= {r[4] % 16 for r in want_recs}
    return want_recs, want_bad


def mixed(n, rng, longest=40):
    shapes = []
    while n:
        size = min(n, rng.randrange(1, longest + 1))
        shapes.append(("ring" if size >= 2 and rng.random() < 0.2 else "path", size))
        n -= size
    rng.shuffle(shapes)
    return shapes


@pytest.mark.parametrize("k", [15, 31, 33, 64])
def test_crafted_lists(k):
    """blocks of one, one chain through all bubbles, rings of both parities, a mix -- at 0, 1, 2, 33, 512 and 513 bubbles; k - 1 = 14 and 30 compare a
    junction in one word, 32 and 63 in one and two.  The unitigs are random, so nearly every junction is bad and the count is the reference's.  The
    inputs put pieces at every base offset mod 32 and sequences at every byte offset mod 16 (asserted from the reference's own offsets)"""
    seen = [set(), set()]
    total_bad = 0
    for n in (0, 1, 2, 33, 512, N_MAX):
        rng = random.Random(7 * n + k)
        if n == 0:
            assert check(k, [], 1, seen=seen) == ([], 0)
            continue
        recs, bad = check(k, [("path", 1)] * n, n, seen=seen)
        assert len(recs) == 2 * n and bad > 0
        recs, bad = check(k, [("path", n)], n + 1, seen=seen)
        assert len(recs) == 2 and recs[0][2] == n
        total_bad += bad
        check(k, mixed(n, rng), n + 2, seen=seen, undecided=0.1)
        if n >= 2:
            for parity in (0, 1):
                recs, _ = check(k, [("ring", n)], n + 3 + parity, seen=seen, ring_parity=parity)
                assert len(recs) == 2 and recs[0][3] == R.CIRCULAR | (R.CONFLICT if parity else 0)
    assert total_bad > 1000
    assert seen[0] == set(range(32)) and seen[1] == set(range(16)), seen


def test_min_block():
    """1, 2, and one above the largest block: no sequences, no bytes, BGR_OK"""
    shapes = [("path", 1), ("path", 5), ("ring", 3), ("path", 1), ("path", 2), ("ring", 2), ("path", 9)]
    recs, _ = check(31, shapes, 11, min_blocks=(1, 2, 3, 9))
    assert [r[2] for r in recs] == [9, 9]
    recs, bad = check(31, shapes, 11, min_blocks=(10,))
    assert recs == [] and bad == 0
    recs, _ = check(31, shapes, 11, min_blocks=(2,))
    assert sorted(r[2] for r in recs[::2]) == [2, 2, 3, 5, 9]


def raw_call(g, ba, ea, min_block, cap, seq_cap, device=0):
    out = np.zeros(max(cap, 1), dtype=B.HAPLOTYPE_DTYPE)
    seq = np.zeros(max(seq_cap, 1), dtype=np.uint8)
    n, nb, bad = B.C.c_uint64(12345), B.C.c_uint64(12345), B.C.c_uint64(12345)
    rc = B.lib().bgr_blocks_haplotypes(g.h, device, ba.ctypes.data if len(ba) else None, len(ba), ea.ctypes.data if len(ea) else None, len(ea), min_block, out.ctypes.data if cap else None,
                                       cap, B.C.byref(n), seq.ctypes.data if seq_cap else None, seq_cap, B.C.byref(nb), B.C.byref(bad))
    untouched = not out.view(np.uint32).any() and not seq.any()
    return rc, int(n.value), int(nb.value), int(bad.value), out, seq, untouched, B.lib().bgr_last_error().decode()


ZERO_TIMES = dict(items=0.0, spell=0.0, records=0.0, total=0.0)


def test_capacity_and_arguments():
    k = 31
    g, us = crafted_graph(k)
    bubbles, phase, _ = G.make([("path", 9), ("ring", 4), ("path", 1)], 5)
    entries = R.blocks_of(bubbles, phase)
    ba, ea = arrays(bubbles, entries)
    want_recs, want_bytes, want_bad, _ = H.haplotypes_of(us, k, bubbles, entries)
    N, S = len(want_recs), len(want_bytes)
    assert N == 6
    def good():
        rc, n, nb, bad, out, seq, _, msg = raw_call(g, ba, ea, 1, N, S)
        assert rc == 0 and (n, nb, bad) == (N, S, want_bad) and H.as_tuples(out[:N]) == want_recs and seq[:S].tobytes() == want_bytes, msg
    for cap, seq_cap in ((N - 1, S), (N, S - 1), (0, 0)):   # either one too small: the sizes, nothing copied
        rc, n, nb, bad, out, seq, untouched, msg = raw_call(g, ba, ea, 1, cap, seq_cap)
        assert rc == E_CAPACITY and (n, nb, bad) == (N, S, want_bad) and untouched and str(S) in msg, (cap, seq_cap, rc, msg)
        t = B.blocks_haplotypes_times()
        assert t["items"] > 0 and t["spell"] == 0 and t["records"] == 0   # only the first two passes have run
    good()
    t = B.blocks_haplotypes_times()
    assert t["total"] > 0 and t["total"] >= t["items"] + t["spell"] + t["records"] and min(t["items"], t["spell"], t["records"]) > 0, t
    def refused(ba_, ea_, word, graph=g, min_block=1):
        rc, n, nb, bad, out, seq, untouched, msg = raw_call(graph, ba_, ea_, min_block, N, S)
        assert rc == E_ARG and (n, nb, bad) == (0, 0, 0) and untouched and word in msg, (rc, msg)
        assert B.blocks_haplotypes_times() == ZERO_TIMES
    refused(ba, ea, "min_block", min_block=0)
    chain = [i for i, e in enumerate(entries) if e[2] == 9]
    swapped = ea.copy()
    swapped["bubble"][chain[2]], swapped["bubble"][chain[5]] = ea["bubble"][chain[5]], ea["bubble"][chain[2]]
    refused(ba, swapped, "no decided link")
    cut = ea.copy()
    cut["index"][chain[4]] = 0
    refused(ba, cut, "block after block")
    beyond = ba.copy()
    beyond["branch"][3][1] = N_UNITIGS + 1 if beyond["branch"][3][1] > 0 else -(N_UNITIGS + 1)
    refused(beyond, ea, "beyond the graph")
    nobubble = ea.copy()
    nobubble["bubble"][0] = len(ba)
    refused(ba, nobubble, "names no bubble")
    small = B.Graph.build(k, "".join(us[1:5]).encode(), np.cumsum([0] + [len(u) for u in us[1:5]]).astype(np.uint64))   # not uploaded
    assert not small.device_blob(0)
    refused(ba[:0], ea[:0], "not resident", graph=small)
    refused(ba, ea, "not resident", graph=small)
    good()   # the next good call passes
    rc, n, nb, bad, out, seq, untouched, msg = raw_call(g, ba, ea[:0], 1, 0, 0)   # no entries: zeroes, no device work
    assert rc == 0 and (n, nb, bad) == (0, 0, 0) and B.blocks_haplotypes_times() == ZERO_TIMES


# ---- two planted haplotypes, end to end ---------------------------------------------------------------------------------------------------------
def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def planted(seed, k=31, genome_len=3000, n_sites=20, coverage=30, read_len=150):
    """-> (the two haplotypes, the unitigs of their compacted graph in file order, the reads)"""
    rng = random.Random(seed)
    genome = "".join(rng.choice("ACGT") for _ in range(genome_len))
    sites = [rng.randrange(k, 120)]
    while len(sites) < n_sites:
        sites.append(sites[-1] + rng.randrange(40, 101))
    assert sites[0] >= k and sites[-1] + k + 1 <= genome_len
    alt = {p: rng.choice([c for c in "ACGT" if c != genome[p]]) for p in sites}
    haps = [genome, "".join(alt.get(i, c) for i, c in enumerate(genome))]
    unitigs, start = [], 0
    for p in sites:   # the flank before the site, then its two branches of 2 k - 1: k - 1 shared with the flanks on either side
        unitigs.append(genome[start:p])
        unitigs += [h[p - (k - 1):p + k] for h in haps]
        start = p + 1
    unitigs.append(genome[start:])
    assert all(len(u) >= k for u in unitigs) and len(unitigs) == 3 * n_sites + 1
    rng.shuffle(unitigs)
    unitigs = [u if rng.random() < 0.5 else rc(u) for u in unitigs]
    reads = []
    for _ in range(genome_len * coverage // read_len):
        h = haps[rng.randrange(2)]
        at = rng.randrange(0, genome_len - read_len + 1)
        r = h[at:at + read_len]
        reads.append(r if rng.random() < 0.5 else rc(r))
    return haps, unitigs, reads


def test_planted_haplotypes_end_to_end(tmp_path):
    """a run over error-free reads of two planted haplotypes phases all sites into one block, and its two sequences are the haplotypes"""
    k = 31
    haps, unitigs, reads = planted(2024)
    uf, rf, PF, NF = (str(tmp_path / x) for x in ("u.fa", "r.fa", "p", "n"))
    open(uf, "w").write("".join(">u%d\n%s\n" % (i, u) for i, u in enumerate(unitigs)))
    open(rf, "w").write("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    g = B.Graph.from_fasta(uf, k)
    g.haplotypes_enable()
    B.align_all(g, rf, PF, NF, m=2, effort=2)
    bubbles, phase = BR.as_tuples(g.bubbles()), P.as_tuples(g.phase())
    entries = R.blocks_of(bubbles, phase)
    assert len(bubbles) == 20 and [e[:3] for e in entries] == [(1, i, 20) for i in range(20)]   # one block of all sites (the reference says so)
    assert R.as_tuples(g.blocks()) == entries
    recs, seq = g.haplotypes()
    assert len(recs) == 2 and [int(x) for x in recs["length"]] == [3000, 3000] and [int(x) for x in recs["offset"]] == [0, 3000]
    got = {seq[:3000].tobytes().decode(), seq[3000:].tobytes().decode()}
    assert got == set(haps) or got == {rc(h) for h in haps}
    recs2, seq2, bad = B.blocks_haplotypes(g, g.bubbles(), g.blocks())
    assert bad == 0 and recs2.tobytes() == recs.tobytes() and seq2.tobytes() == seq.tobytes()


# ---- the CLI and the run ----------------------------------------------------------------------------------------------------------------------
FLAGS = ("haplotypes", "blocks", "bubbles", "phase", "triples", "gfa")


def bubble_records(b):
    return [(key[0], key[1], (key[2], key[3]), v) for key, v in parse_bubbles(b).items()]


def parse_blocks(b, bubbles):
    """the lines of a `--blocks` file over the records of the `--bubbles` file of the same run -> blocks_ref's entries"""
    lines = b.decode("latin-1").split("\n")
    assert lines[0] + "\n" == R.HEADER and lines[-1] == ""
    out = []
    for ln in lines[1:-1]:
        c = ln.split("\t")
        block, index, size, bubble = (int(x) for x in c[:4])
        s, t, br, _ = bubbles[bubble - 1]
        rev = c[8] == "-"
        hap_a = int(c[6]) * (-1 if rev else 1)
        assert hap_a in br
        flags = (R.REVERSED if rev else 0) | (R.HAP if hap_a == br[1] else 0) | {".": 0, "circular": R.CIRCULAR, "conflict": R.CIRCULAR | R.CONFLICT}[c[9]]
        out.append((block, index, size, bubble - 1, flags))
    assert R.blocks_text(bubbles, out) == b
    return out


def text_of(us, r, min_block=1):
    bubbles = bubble_records(r["bubbles"])
    return H.haplotypes_text(us, 31, bubbles, parse_blocks(r["blocks"], bubbles), min_block)


@pytest.mark.parametrize("extra", ROUTES, ids=ROUTE_IDS)
def test_cli_haplotypes_with_the_other_flags(synth_files, extra):
    """the bytes = haplotypes_ref over the parsed bubbles and blocks files of the same run and the unitig file; --min-block 2 keeps exactly the
    blocks of more than one bubble; paths, notAligned.fa and the counters are those of a run without any flag"""
    args, us, plain, rows = synth_files
    r = run(args + extra, flags=FLAGS)
    assert r["haplotypes"] == text_of(us, r) and r["haplotypes"].count(b">block") == 2 * sum(1 for ln in r["blocks"].split(b"\n")[1:-1] if ln.split(b"\t")[1] == b"0")
    assert r["paths"] == plain["paths"] and r["na"] == plain["na"] and parse_counters(r["out"]) == parse_counters(plain["out"])
    r2 = run(args + extra, flags=FLAGS, more=["--min-block", "2"])
    assert r2["blocks"] == r["blocks"] and r2["haplotypes"] == text_of(us, r, 2)
    heads = [ln.split(b" ")[1] for ln in r2["haplotypes"].split(b"\n") if ln.startswith(b">")]
    multi = sum(1 for ln in r["blocks"].split(b"\n")[1:-1] if ln.split(b"\t")[1] == b"0" and int(ln.split(b"\t")[2]) > 1)
    assert len(heads) == 2 * multi and multi >= 2 and all(int(h.split(b"=")[1]) >= 2 for h in heads)


def test_cli_haplotypes_alone_changes_nothing_else(synth_files):
    """without the other flags: the same file, and stdout too is what it is without the flag; the thresholds reach the run"""
    args, us, plain, rows = synth_files
    alone = run(args, flags=("haplotypes",))
    both = run(args, flags=FLAGS)
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
    assert alone["haplotypes"] == both["haplotypes"] and strip(alone["out"]) == strip(plain["out"])
    assert alone["paths"] == plain["paths"] and alone["na"] == plain["na"]
    a3 = run(args, flags=("haplotypes",), more=["--min-link", "3", "--min-phase", "2", "--min-block", "2"])   # alone, the thresholds are the haplotypes' own
    b3 = run(args, flags=FLAGS, more=["--min-link", "3", "--min-phase", "2", "--min-block", "2"])
    assert a3["haplotypes"] == b3["haplotypes"] == text_of(us, b3, 2)
    an = run(args, flags=("haplotypes",), more=["--min-link", "999999999"])   # no link is supported: no bubble, no block, no sequence
    assert an["haplotypes"] == b"" and an["paths"] == plain["paths"]


def test_cli_refusals(tmp_path):
    base = [B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5"]
    f = str(tmp_path / "x.haplotypes")
    def cli(graph, *more):
        return subprocess.run(base + ["-g", os.path.join(GOLD, graph)] + list(more), cwd=tmp_path, capture_output=True, text=True, timeout=300)
    pr = cli("deg_unitig.fa", "--haplotypes", f, "-b")
    assert pr.returncode == 2 and "--haplotypes" in pr.stderr and "-b" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig_exc.fa", "--haplotypes", f)
    assert pr.returncode == 2 and "--haplotypes" in pr.stderr and "ACGT" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--min-block", "2")   # the threshold alone
    assert pr.returncode == 2 and "--min-block" in pr.stderr, pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--blocks", str(tmp_path / "x.blocks"), "--min-block", "2")   # ... is none of --blocks
    assert pr.returncode == 2 and "--min-block" in pr.stderr and not os.path.exists(tmp_path / "x.blocks"), pr.stderr[-500:]
    for bad in ("0", "x", "1234567890", "-1", ""):
        pr = cli("deg_unitig.fa", "--haplotypes", f, "--min-block", bad)
        assert pr.returncode == 2 and "--min-block" in pr.stderr and not os.path.exists(f), (bad, pr.stderr[-500:])
    pr = cli("deg_unitig.fa", "--min-phase", "2")   # accepted with --haplotypes as with --blocks: the refusal names both
    assert pr.returncode == 2 and "--blocks" in pr.stderr and "--haplotypes" in pr.stderr, pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--haplotypes", f, "--min-phase", "2", "--min-link", "2", "--min-block", "1")
    assert pr.returncode == 0 and os.path.exists(f), pr.stderr[-500:]


def test_align_all_keeps_the_haplotypes_in_the_graph(synth_files, tmp_path):
    args, us, _, rows = synth_files
    g = B.Graph.from_fasta(args[5], 31)
    PF, NF = str(tmp_path / "p"), str(tmp_path / "n")
    with pytest.raises(B.BgrError):
        g.haplotypes()
    for kw in (dict(min_block=0), dict(min_phase=0), dict(min_link=0)):
        with pytest.raises(B.BgrError):
            g.haplotypes_enable(**kw)
    g.haplotypes_enable(min_link=2, min_phase=2, min_block=2)
    assert g.haplotypes_enabled() and not g.blocks_enabled() and not g.phase_enabled() and not g.bubbles_enabled()
    B.align_all(g, args[1], PF, NF, m=2, effort=2, threads=2)
    bubbles, phase = BR.as_tuples(g.bubbles()), P.as_tuples(g.phase())   # the switch implies the blocks', and with it everything before
    entries = R.blocks_of(bubbles, phase, 2)
    assert R.as_tuples(g.blocks()) == entries and len(bubbles) > 10
    want_recs, want_bytes, want_bad, _ = H.haplotypes_of(us, 31, bubbles, entries, 2)
    recs, seq = g.haplotypes()
    assert H.as_tuples(recs) == want_recs and seq.tobytes() == want_bytes and want_bad == 0 and len(want_recs) >= 2
    B.write_haplotypes(str(tmp_path / "h"), g, g.bubbles(), g.blocks(), recs, seq)
    cli = run(args, flags=("haplotypes",), more=["--min-link", "2", "--min-phase", "2", "--min-block", "2"])
    assert open(tmp_path / "h", "rb").read() == H.haplotypes_text(us, 31, bubbles, entries, 2) == cli["haplotypes"]
    bad = recs.copy()
    bad["offset"][1] += 1
    with pytest.raises(B.BgrError, match="error -1.*back to back"):
        B.write_haplotypes(str(tmp_path / "h2"), g, g.bubbles(), g.blocks(), bad, seq)
    g.haplotypes_enable(False)
    B.align_all(g, args[1], PF, NF, m=2, effort=2)   # a run with the switch off leaves the kept records alone
    assert g.haplotypes()[1].tobytes() == want_bytes
    g.haplotypes_enable()
    with pytest.raises(B.BgrError):   # a run that fails leaves none
        B.align_all(g, str(tmp_path / "missing.fa"), PF, NF)
    with pytest.raises(B.BgrError):
        g.haplotypes()
