"""The definition of --recompact (recompact_ref.py) checking itself on random unitig sets; the rule the kernels rest on -- (key index, orientation bit)
from the blob's meta are equal exactly when the end (k-1)-mers are equal strings -- verified against the strings on every golden graph and on the
degenerate sets; the host code (flag rules, keep bytes, --min-reads, the writer's bytes) in a stand-alone program under ASan + UBSan.  No device."""
import os
import subprocess

import numpy as np

import bgreat_amd as B
import gaf_ref as G
import recompact_gen as RG
import recompact_ref as RR
from util import GOLD, ROOT

SRC = os.path.join(ROOT, "bgreat_amd", "csrc")
FUZZ_SEEDS = range(500)
FUZZ_KS = (4, 5, 6, 7)


def test_hand_checked_chains():
    # k = 4: 1 -> 2 -> 3 is a chain whatever the strands and the order of the ids
    s = "ACGGTCAATGCC"
    us = [s[3:9], RR.rc(s[0:6]), s[6:12]]   # 2 reversed | 1 | 3
    assert RR.compact(us, [1, 1, 1], 4) == [([-2, 1, 3], False, s)]   # head -2 < -tail = -3
    # dropping the middle one leaves two chains of one, each reported forward
    assert RR.compact(us, [0, 1, 1], 4) == [([2], False, us[1]), ([3], False, us[2])]
    assert RR.compact(us, [0, 0, 0], 4) == []
    # a fork: out = 2, nothing merges; without one branch the rest is one chain
    us = ["AACCGT", "CGTGGA", "CGTTTG"]
    assert [w for w, _, _ in RR.compact(us, [1, 1, 1], 4)] == [[1], [2], [3]]
    assert RR.compact(us, [1, 0, 1], 4) == [([1, 3], False, "AACCGTTTG")]
    # a ring of two, its smallest-id member stored reversed: read with +1 first, opened where +1 is entered
    ring = "ACGGTCAATG"
    a, b = ring[0:5 + 3], (ring + ring[:3])[5:]
    res = RR.compact([RR.rc(a), b], [1, 1], 4)
    assert res == [([1, -2], True, RR.spell_walk([RR.rc(a), b], [1, -2], 4))]
    assert RR.fasta_bytes(res) == b">1 LN:i:13 unitigs=2 ring=circular walk=>1<2\n" + res[0][2].encode() + b"\n"
    assert RR.records(res) == ([(0, 13, 0, 2, 1)], [1, -2], res[0][2].encode())


def test_the_reference_checks_itself_on_random_sets():
    met = {"ring": 0, "hairpin": 0, "self_loop": 0, "palindrome": 0}
    merged = longest = 0
    for k in FUZZ_KS:
        for seed in FUZZ_SEEDS:
            us, keep = RG.fuzz_set(seed, k)
            assert 1 <= len(us) <= 40 and all(k <= len(u) <= 3 * k for u in us)
            st = {}
            res = RR.compact(us, keep, k, stats_out=st)
            for key in met:
                met[key] += st[key]
            merged += sum(1 for w, _, _ in res if len(w) > 1)
            longest = max([longest] + [len(w) for w, _, _ in res])
            recs, walk, seq = RR.records(res)
            assert len(walk) == sum(keep) and len(seq) == sum(r[1] for r in recs)
    assert all(v > 0 for v in met.values()) and merged > 500 and longest >= 6, (met, merged, longest)


def _meta(g):
    blob = g.blob()
    h = blob[:4096].view(np.uint64)
    n, n_keys, off_meta = int(h[3]), int(h[4]), int(h[13])
    m = blob[off_meta:off_meta + 32 * (n + 1)].view(np.uint32).reshape(n + 1, 8)
    return n, n_keys, m


def _end_pairs(m, u):
    """(key index, orientation bit) of first(+u), first(-u), last(+u), last(-u) by the table in include/bgreat_gpu.h (recompact_kernels.hip: end_key)"""
    flags, rec_beg, rec_end = int(m[u, 1]), int(m[u, 2]), int(m[u, 3])
    bit = lambda f: 0 if flags & f else 1
    return [(rec_beg, bit(1)), (rec_end, bit(8)), (rec_end, bit(2)), (rec_beg, bit(4))]


def _check_meta_rule(g, us, k):
    K = k - 1
    n, n_keys, m = _meta(g)
    assert n == len(us)
    by_pair, by_str = {}, {}
    pal = 0
    for u in range(1, n + 1):
        s, r = us[u - 1], RR.rc(us[u - 1])
        for pair, e in zip(_end_pairs(m, u), (s[:K], r[:K], s[-K:], r[-K:])):
            assert pair[0] < n_keys
            assert by_pair.setdefault(pair, e) == e, "one pair, two strings"
            assert by_str.setdefault(e, pair) == pair, "one string, two pairs"
            if e == RR.rc(e):
                pal += 1
                assert pair[1] == 0
    return pal


def test_meta_pairs_are_equal_exactly_when_the_end_strings_are():
    pal = 0
    # every golden graph but deg_unitig_exc.fa, whose non-ACGT characters the feature refuses
    for graph, k in (("deg_unitig.fa", 5), ("deg_unitig.fa", 6), ("long_unitig.fa", 31), ("short_stop_unitig.fa", 5), ("syn_unitig.fa", 25), ("syn_unitig.fa", 31), ("toy_unitig.fa", 4),
                     ("soup_polyA_unitig.fa", 15)):
        us = G.load_unitigs(os.path.join(GOLD, graph), k)[1:]
        assert not any(set(u) - set("ACGT") for u in us), graph   # (deg_unitig.fa at k = 6 is the empty graph: its first unitig is shorter than k)
        pal += _check_meta_rule(B.Graph.from_fasta(os.path.join(GOLD, graph), k), us, k)
        with B.options(**{"test.wide_keys": 1}):
            gw = B.Graph.from_fasta(os.path.join(GOLD, graph), k)
        _check_meta_rule(gw, us, k)
    for k in FUZZ_KS:
        for seed in range(0, 500, 5):
            us, _ = RG.fuzz_set(seed, k)
            pal += _check_meta_rule(B.Graph.build(k, *RG.to_arrays(us)), us, k)
            if seed % 25 == 0:
                with B.options(**{"test.wide_keys": 1}):
                    _check_meta_rule(B.Graph.build(k, *RG.to_arrays(us)), us, k)
    for k, pieces, circ in ((15, 7, True), (31, 5, False), (33, 4, True), (64, 3, False)):
        us, _ = RG.chain_set(3, k, pieces, circ)
        _check_meta_rule(B.Graph.build(k, *RG.to_arrays(us)), us, k)
    assert pal > 50, pal


def _sanitize_exe(tmp_path):
    exe = str(tmp_path / "sanitize_recompact")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-Wall", "-I" + SRC, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "sanitize_recompact.cpp"), "-o", exe])
    return exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_host_code_is_sanitizer_clean_and_writes_the_references_bytes(tmp_path):
    """the flag rules of counts_wanted for the new switch, the keep bytes, --min-reads, the check of a result: asserted inside the program; the writer's
    bytes (the two functions bgr_write_recompact calls, in its order) against recompact_ref.fasta_bytes on random sets"""
    exe, env = _sanitize_exe(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "recompact ok" in p.stdout and "FAIL" not in p.stdout
    assert "ERROR: " not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    n = 0
    for k, seed in ((4, 0), (5, 3), (6, 6), (7, 9), (5, 12)):
        us, keep = RG.fuzz_set(seed, k)
        res = RR.compact(us, keep, k)
        recs, walk, seq = RR.records(res)
        if not recs:
            continue
        inp, outp = tmp_path / "in.txt", tmp_path / "out.fa"
        inp.write_text("%d %d %d %d %d\n" % (len(recs), len(walk), len(seq), len(us), k) + "".join("%d %d %d %d %d\n" % r for r in recs) + " ".join(map(str, walk)) + "\n" + seq.decode() + "\n")
        p = subprocess.run([exe, "write", str(inp), str(outp)], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0 and "ERROR: " not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
        assert outp.read_bytes() == RR.fasta_bytes(res)
        n += 1
    assert n >= 4
    # a result whose walk names a unitig outside the graph is refused
    inp.write_text("1 1 5 3 5\n0 5 0 1 0\n4\nACGTA\n")
    assert subprocess.run([exe, "write", str(inp), str(outp)], env=env, timeout=300).returncode == 3


def test_write_recompact_bytes_and_refusals(tmp_path):
    """bgr_write_recompact itself (host code of the library) against the reference, and what it refuses; the switch and the getter without a run"""
    us, keep = RG.fuzz_set(3, 5)
    g = B.Graph.build(5, *RG.to_arrays(us))
    res = RR.compact(us, keep, 5)
    recs, walk, seq = RR.records(res)
    r = np.array(recs, dtype=B.CHAIN_DTYPE)
    path = str(tmp_path / "out.fa")
    B.write_recompact(path, g, r, np.array(walk, dtype=np.int32), np.frombuffer(seq, dtype=np.uint8))
    assert open(path, "rb").read() == RR.fasta_bytes(res)
    assert G.load_unitigs(path, 5)[1:] == [s for _, _, s in res]   # the file is a unitig file
    B.write_recompact(path, g, r[:0], np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8))
    assert open(path, "rb").read() == b""
    for change in (lambda r, w: w.__setitem__(0, len(us) + 1), lambda r, w: w.__setitem__(0, 0), lambda r, w: r["seq_off"].__setitem__(0, 1), lambda r, w: r["flags"].__setitem__(0, 2)):
        r2, w2 = r.copy(), np.array(walk, dtype=np.int32)
        change(r2, w2)
        try:
            B.write_recompact(path, g, r2, w2, np.frombuffer(seq, dtype=np.uint8))
            assert False
        except B.BgrError as e:
            assert "bgr_write_recompact" in str(e)
    assert not g.recompact_enabled()
    g.recompact_enable(True, 0)
    assert g.recompact_enabled()
    g.recompact_enable(False)
    assert not g.recompact_enabled()
    try:
        g.recompact_result()
        assert False
    except B.BgrError as e:
        assert "no chains" in str(e)
    # a graph with a character that is not ACGT refuses the switch; a graph that is not on a device the call
    gn = B.Graph.build(5, *RG.to_arrays(["ACGTNACGT", "GGGGGCC"]))
    try:
        gn.recompact_enable(True, 1)
        assert False
    except B.BgrError as e:
        assert "ACGT" in str(e)
    try:
        g.recompact(np.ones(len(us), dtype=np.uint8))
        assert False
    except B.BgrError as e:
        assert "not resident" in str(e)
