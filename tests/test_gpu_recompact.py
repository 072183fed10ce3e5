"""bgr_graph_recompact on the device against recompact_ref.py -- every record, every walk int, every sequence byte -- on the smallest shapes at which
each pass can go wrong; the capacity and argument refusals; and the CLI: --recompact end to end on a genome whose answer needs no restatement."""
import os
import random
import subprocess

import numpy as np
import pytest

import bgreat_amd as B
import gaf_cs_ref as CS
import gaf_ref as G
import recompact_gen as RG
import recompact_ref as RR

pytestmark = pytest.mark.gpu

SEEN_PIECE_MOD32, SEEN_SEQ_MOD16 = set(), set()


def _graph(us, k, wide=False):
    if wide:
        with B.options(**{"test.wide_keys": 1}):
            g = B.Graph.build(k, *RG.to_arrays(us))
    else:
        g = B.Graph.build(k, *RG.to_arrays(us))
    g.upload(0)
    return g


def _check(us, keep, k, wide=False, g=None):
    """the device's result == the reference's -> the reference's result"""
    g = g or _graph(us, k, wide)
    want = RR.compact(us, keep, k, check=len(us) <= 200)
    recs, walk, seq = RR.records(want)
    r, w, s = g.recompact(np.array(keep, dtype=np.uint8))
    assert [tuple(int(x) for x in row) for row in r] == recs
    assert w.tolist() == walk
    assert s.tobytes() == seq
    n, n_keys, m = _meta_F(g)
    for so, sl, wo, nu, _ in recs:   # which alignments the spell pass met: a piece's base offset in the 2-bit store mod 32, its place in the output mod 16
        o = so
        for j, x in enumerate(walk[wo:wo + nu]):
            ln, F = int(m[abs(x), 0]), int(m[abs(x)].view(np.uint64)[2])
            skip = (k - 1) if j else 0
            SEEN_PIECE_MOD32.add((F + (ln if x < 0 else 0) + skip) % 32)
            SEEN_SEQ_MOD16.add(o % 16)
            o += ln - skip
    return want


def _meta_F(g):
    blob = g.blob()
    h = blob[:4096].view(np.uint64)
    n, n_keys, off_meta = int(h[3]), int(h[4]), int(h[13])
    return n, n_keys, blob[off_meta:off_meta + 32 * (n + 1)].view(np.uint32).reshape(n + 1, 8)


@pytest.mark.parametrize("pieces", [1, 2, 3, 1500])
def test_chains_in_random_strands_and_id_order(pieces):
    """1 500: longer than a scan tile of 1 024 nodes, 11 jumping rounds and more"""
    us, s = RG.chain_set(pieces, 31, pieces, piece_len=3 if pieces > 3 else None)
    (w, c, q), = _check(us, [1] * len(us), 31)
    assert len(w) == pieces and not c and q in (s, RR.rc(s))


@pytest.mark.parametrize("pieces,first_rc", [(2, False), (3, True), (1025, True)])
def test_rings(pieces, first_rc):
    """first_rc: the ring's smallest-|id| member is stored reverse-complemented -- the ring is still read with +1 first"""
    us, s = RG.chain_set(pieces + 7, 31, pieces, circular=True, piece_len=3 if pieces > 3 else None, first_rc=first_rc)
    (w, c, q), = _check(us, [1] * len(us), 31)
    assert len(w) == pieces and c and w[0] == 1 and q[:30] == q[-30:] and len(q) == len(s) + 30


def test_excluded_links_and_degrees():
    k = 5
    h = "ACGA"
    for us in (["ACGAT" + "TCGT"],                         # a hairpin: ends with the reverse complement of its beginning
               [h + "GG" + h],                             # a self-loop
               ["ACGATTGCA", "ACGATTGCA"],                 # two identical unitigs
               ["GGACGA", h + "TT", h + "CC"],             # a branch with out = 2
               ["TT" + h, "CC" + h, h + "GGT"],            # a join with in = 2
               ["GGACGA", h + "TT", h + "GG" + h]):        # a self-loop next to a link
        _check(us, [1] * len(us), k)


@pytest.mark.parametrize("k", [5, 31])
def test_palindromic_overlap(k):
    rng = random.Random(k)
    half = RG.random_seq(rng, (k - 1) // 2)
    pal = half + RR.rc(half)
    assert pal == RR.rc(pal) and len(pal) == k - 1
    a, b = "GG" + RG.random_seq(rng, 7) + pal, pal + RG.random_seq(rng, 9) + "CC"
    _check([a, b], [1, 1], k)                 # a ends with the palindrome, b and rc(a) begin with it: out(a) = 2
    _check([a, RR.rc(b)], [1, 1], k)
    _check([a], [1], k)                       # a -> -a alone is a hairpin
    _check([a, b, RR.rc(b) + "A"], [1, 1, 0], k)


def test_the_subset():
    us, s = RG.chain_set(11, 31, 5)
    g = _graph(us, 31)
    order = [abs(x) for x in _check(us, [1] * 5, 31, g=g)[0][0]]
    keep = [1] * 5
    keep[order[2] - 1] = 0
    assert sorted(len(w) for w, _, _ in _check(us, keep, 31, g=g)) == [2, 2]   # a dropped unitig in the middle of a chain gives two chains
    r, w, q = g.recompact(np.zeros(5, dtype=np.uint8))
    assert len(r) == 0 and len(w) == 0 and len(q) == 0                          # everything dropped: zero records, zero bytes
    fork = ["GG" + s[:30], s[:30] + "AC", s[:30] + "CA"]
    assert len(_check(fork, [1, 1, 1], 31)) == 3
    assert [w for w, _, _ in _check(fork, [1, 0, 1], 31)] == [[1, 3]]         # a dropped branch turns a fork into a merge
    res = _check(us, [1] * 5, 31, g=g)                                          # an already compact graph reproduces its unitigs
    again = [q for _, _, q in res]
    assert [(w, q) for w, _, q in _check(again, [1], 31)] == [([1], again[0])]


def test_spelling_lengths_and_alignments():
    k = 31
    rng = random.Random(5)
    us = [RG.random_seq(rng, n) for n in (k, k + 1, 2 * k - 1, 33, 64, 65)]
    _check(us, [1] * len(us), k)
    big = RG.random_seq(rng, 70001)             # spans several 16 KiB output tiles
    _check([big[:40], big[10:]], [1, 1], k)
    for seed in range(3):                       # chains of pieces of every length mod 32 behind each other
        us, _ = RG.chain_set(seed, k, 70, piece_len=1 + seed * 2)
        _check(us, [1] * len(us), k)
        us, _ = RG.chain_set(seed + 10, k, 40, piece_len=5 + seed)
        _check(us, [0] + [1] * (len(us) - 1), k)
    assert SEEN_PIECE_MOD32 == set(range(32)) and SEEN_SEQ_MOD16 == set(range(16)), (sorted(SEEN_PIECE_MOD32), sorted(SEEN_SEQ_MOD16))


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_tile_borders(n):
    """2 046 .. 2 050 nodes around two scan tiles: chains of three and single unitigs mixed"""
    us, _ = RG.chain_set(n, 31, n, piece_len=2)
    rng = random.Random(n)
    keep = [0 if rng.random() < 0.25 else 1 for _ in us]
    _check(us, keep, 31)


@pytest.mark.parametrize("k,wide", [(15, False), (31, False), (33, False), (64, False), (31, True)])
def test_k(k, wide):
    us, _ = RG.chain_set(k, k, 9, circular=False)
    us2, _ = RG.chain_set(k + 1, k, 6, circular=True)
    us = us + us2 + [us[0]]                    # a chain, a ring, and a duplicate that splits the chain
    _check(us, [1] * len(us), k, wide)
    _check(us, [1] * (len(us) - 1) + [0], k, wide)


def test_fuzz_small_k():
    for k in (4, 5, 6, 7):
        for seed in range(0, 50):
            us, keep = RG.fuzz_set(seed, k)
            _check(us, keep, k)
            if seed % 10 == 0:
                _check(us, [1] * len(us), k, wide=True)


def test_capacity_and_arguments():
    us, _ = RG.chain_set(2, 31, 4)
    us.append(RG.random_seq(random.Random(1), 40))
    g = _graph(us, 31)
    keep = np.ones(len(us), dtype=np.uint8)
    r, w, s = g.recompact(keep)
    L = B.lib()
    import ctypes as C
    for dn, dw, ds in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):   # each of the three buffers one too small
        out, walk, seq = np.zeros(len(r), dtype=B.CHAIN_DTYPE), np.full(len(w), 77, dtype=np.int32), np.full(len(s), 77, dtype=np.uint8)
        n, nw, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = L.bgr_graph_recompact(g.h, 0, keep.ctypes.data, len(keep), out.ctypes.data, len(r) - dn, C.byref(n), walk.ctypes.data, len(w) - dw, C.byref(nw), seq.ctypes.data, len(s) - ds,
                                   C.byref(nb))
        assert rc == -4 and (n.value, nw.value, nb.value) == (len(r), len(w), len(s))
        assert not out["seq_len"].any() and (walk == 77).all() and (seq == 77).all()   # nothing copied
    for bad_keep in (keep[:-1], np.ones(len(us) + 1, dtype=np.uint8)):
        with pytest.raises(B.BgrError, match="n_keep"):
            g.recompact(bad_keep)
    gn = B.Graph.build(31, *RG.to_arrays([us[0][:20] + "N" + us[0][21:], us[1]]))
    gn.upload(0)
    with pytest.raises(B.BgrError, match="ACGT"):
        gn.recompact(np.ones(2, dtype=np.uint8))
    with pytest.raises(B.BgrError, match="not resident"):
        g.recompact(keep, device=7)
    t = B.recompact_times()
    assert set(t) == {"links", "rank", "place", "spell", "records"}


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
def _genome_case(tmp_path):
    """a random genome of 3 000 characters without a repeated 30-mer, error-free reads of 150 at coverage 30, 20 more with one substitution each at
    distinct positions; the graph: the unitigs of all the reads' k-mers (compacted by the reference from one-k-mer unitigs)"""
    k = 31
    rng = random.Random(2024)
    genome = RG.unique_seq(rng, 3000, k)
    reads = []
    for _ in range(3000 * 30 // 150):
        p = rng.randrange(0, 3000 - 150 + 1)
        r = genome[p:p + 150]
        reads.append(r if rng.random() < 0.5 else RR.rc(r))
    reads += [genome[:150], genome[-150:]]   # (both ends are covered whatever the draw)
    for p in rng.sample(range(200, 2800), 20):
        r = list(genome[p - 75:p + 75])
        r[75] = {"A": "C", "C": "G", "G": "T", "T": "A"}[r[75]]
        reads.append("".join(r))
    kmers = {}
    for r in reads:
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            c = min(w, RR.rc(w))
            kmers[c] = 1
    unitigs = [q for _, _, q in RR.compact(sorted(kmers), [1] * len(kmers), k, check=False)]
    (tmp_path / "unitigs.fa").write_text("".join(">%d\n%s\n" % (i + 1, u) for i, u in enumerate(unitigs)))
    (tmp_path / "reads.fa").write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    return k, genome, unitigs, reads


def _cli(tmp_path, more, ok=0):
    p = subprocess.run([B.CLI_PATH, "-r", "reads.fa", "-g", "unitigs.fa", "-k", "31", "-m", "0"] + more, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == ok, (more, p.returncode, p.stderr[-1000:])
    return p


def test_cli_end_to_end(tmp_path):
    k, genome, unitigs, reads = _genome_case(tmp_path)
    assert len(unitigs) > 40
    outputs = lambda p: [(tmp_path / f).read_bytes() for f in ("paths", "notAligned.fa")] + [p.stdout]
    for more in ([], ["--host-route"], ["--gpus", "2", "--set", "test.lanes_on_one_device=1"], ["--gfa", "x.gfa", "--bubbles", "x.bub"]):
        plain = outputs(_cli(tmp_path, ["--inside"] + more))
        p = _cli(tmp_path, ["--inside", "--recompact", "out.fa", "--min-reads", "2"] + more)
        got = G.load_unitigs(str(tmp_path / "out.fa"), k)[1:]
        assert len(got) == 1 and got[0] in (genome, RR.rc(genome)), (more, len(got))   # ONE sequence: the genome
        assert outputs(p) == plain, more   # the run's own output does not change, on any route
        (tmp_path / "out.fa").unlink()
    _cli(tmp_path, ["--inside", "--recompact", "all.fa", "--min-reads", "0"])
    assert (tmp_path / "all.fa").read_bytes() == RR.fasta_bytes(RR.compact(unitigs, [1] * len(unitigs), k))


def test_cli_second_run_on_the_cleaned_graph(tmp_path):
    """out.fa of a --min-reads 1 run as -g of a second run of the same reads: every read that mapped in the first run maps in the second, and its
    --gaf --cs line rebuilds the read's characters from the NEW graph"""
    k, genome, unitigs, reads = _genome_case(tmp_path)
    _cli(tmp_path, ["--inside", "--gaf", "--recompact", "one.fa", "--min-reads", "1"])
    first = [G.parse_line(l + "\n")["name"] for l in (tmp_path / "paths").read_text().splitlines()]
    assert len(first) >= 600 and len(set(first)) == len(first)
    new = G.load_unitigs(str(tmp_path / "one.fa"), k)
    assert 1 <= len(new) - 1 <= len(unitigs)   # (at -m 0 a read with a substitution maps on its own branch: one read supports it)
    p = subprocess.run([B.CLI_PATH, "-r", "reads.fa", "-g", "one.fa", "-k", "31", "-m", "0", "--inside", "--gaf", "--cs", "--gfa", "two.gfa"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-1000:]
    by_name = {"r%d" % i: r for i, r in enumerate(reads)}
    second = set()
    for line in (tmp_path / "paths").read_text().splitlines():
        body, cs = line.rsplit("\t", 1)
        assert cs.startswith("cs:Z:")
        f = G.parse_line(body + "\n")
        walk = G.spell(new, k, f["segments"])
        assert walk is not None and len(walk) == f["plen"]
        read = by_name[f["name"]]
        assert CS.apply_ops(cs[5:], walk[f["pstart"]:f["pend"]]) == read[f["qstart"]:f["qend"]]   # the same read characters from the new graph
        second.add(f["name"])
    assert set(first) <= second, sorted(set(first) - second)[:5]


def test_cli_refusals(tmp_path):
    _genome_case(tmp_path)
    assert "--min-reads" in _cli(tmp_path, ["--min-reads", "2"], ok=2).stderr
    for bad in ("", "-1", "1x", "1234567890"):
        assert "--min-reads" in _cli(tmp_path, ["--recompact", "o.fa", "--min-reads", bad], ok=2).stderr
    assert "--abundance" in _cli(tmp_path, ["--recompact", "o.fa", "-b"], ok=2).stderr   # refused where --abundance is, in its words
    (tmp_path / "n.fa").write_text(">1\n" + "ACGT" * 10 + "N" + "ACGT" * 10 + "\n")
    p = subprocess.run([B.CLI_PATH, "-r", "reads.fa", "-g", "n.fa", "-k", "31", "--recompact", "o.fa"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "ACGT" in p.stderr


def test_align_all_keeps_the_chains_in_the_graph(tmp_path):
    k, genome, unitigs, reads = _genome_case(tmp_path)
    g = B.Graph.from_fasta(str(tmp_path / "unitigs.fa"), k)
    g.devices_init(0, 1)
    g.recompact_enable(True, 0)
    B.align_all(g, str(tmp_path / "reads.fa"), str(tmp_path / "p"), str(tmp_path / "n"), m=0)
    r, w, s = g.recompact_result()
    recs, walk, seq = RR.records(RR.compact(unitigs, [1] * len(unitigs), k))
    assert [tuple(int(x) for x in row) for row in r] == recs and w.tolist() == walk and s.tobytes() == seq
    with pytest.raises(B.BgrError):   # a failed run keeps none
        B.align_all(g, str(tmp_path / "missing.fa"), str(tmp_path / "p"), str(tmp_path / "n"), m=0)
    with pytest.raises(B.BgrError, match="no chains"):
        g.recompact_result()
