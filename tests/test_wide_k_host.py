"""Graphs with 32 < k <= 64 (two-word overlap keys), host side: the Python checker of the reference's greedy path (wide_greedy_ref.py) pinned
to the C++ oracle at k <= 32, builds and key lookups at k > 32, wide blobs, and the planner's routing.  No GPU needed."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
import wide_greedy_ref as W
from tools.synth import Synth
from util import GOLD, golden_cases

ACGT = "ACGT"


def strings(buf, offs):
    b = bytes(np.asarray(buf, dtype=np.uint8))
    return [b[int(offs[i]):int(offs[i + 1])].decode() for i in range(len(offs) - 1)]


def pack(strs):
    offs = np.zeros(len(strs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in strs])
    return np.frombuffer("".join(strs).encode(), dtype=np.uint8).copy(), offs


def read_unitigs(path):
    lines = open(path).read().split("\n")
    return [lines[i + 1] for i in range(0, len(lines) - 1, 2)]


def high_degree_graph(k, n, seed, n_ends=6):
    """Unitigs whose ends come from a small pool of (k-1)-mers: up to four unitigs (and the slot-4 overwrite) on a key."""
    r = random.Random(seed)
    pool = ["".join(r.choice(ACGT) for _ in range(k - 1)) for _ in range(n_ends)]
    return [r.choice(pool) + "".join(r.choice(ACGT) for _ in range(r.randrange(1, 3 * k))) + r.choice(pool) for _ in range(n)]


def reads_from(unitigs, n, L, seed, subs=2, with_n=True):
    r = random.Random(seed)
    walk = "".join(unitigs)
    out = []
    for i in range(n):
        p = r.randrange(0, max(1, len(walk) - L))
        s = list(walk[p:p + L])
        for _ in range(r.randrange(0, subs + 1)):
            s[r.randrange(len(s))] = r.choice(ACGT)
        if with_n and i % 7 == 3:
            s[r.randrange(len(s))] = "N"
        s = "".join(s)
        out.append(W.reverse_complements(s) if i % 2 else s)
    return out


def check_pin(k, unitigs, reads, ms=(0, 2, 4), efforts=(0, 1, 2, 5)):
    useqs, uoffs = pack(unitigs)
    rseqs, roffs = pack(reads)
    o = oracle_py.Oracle(k, useqs, uoffs)
    ref = W.GreedyRef(k, unitigs)
    for m in ms:
        for e in efforts:
            rows_o = W.rows_of(*o.align(rseqs, roffs, m=m, effort=e))
            rows_w, _ = ref.align(reads, m, e)
            for i, (a, b) in enumerate(zip(rows_o, rows_w)):
                assert a == b, (k, m, e, i, reads[i], a, b)


@pytest.mark.parametrize("k", [5, 15, 21, 31, 32])
@pytest.mark.parametrize("alleles", [2, 4])
def test_checker_matches_oracle_on_synth(k, alleles):
    s = Synth(8000, 40, alleles, k, 11 + k)
    unitigs = strings(*s.unitigs())
    reads, roffs = s.reads(0, 150, 100, 3, 5 + k)
    check_pin(k, unitigs, strings(reads, roffs) + reads_from(unitigs, 40, 80, k))


@pytest.mark.parametrize("k", [5, 15, 21, 31, 32])
def test_checker_matches_oracle_on_high_degree_graphs(k):
    unitigs = high_degree_graph(k, 60, 3 * k)
    check_pin(k, unitigs, reads_from(unitigs, 120, 3 * k + 10, k))


def test_checker_matches_oracle_on_goldens():
    seen = set()
    for c in golden_cases():
        a = c["args"]
        if not any(x.startswith(("deg_", "edge_", "soup_polyA")) for x in a) or "-b" in a or "-G" in a or "-q" in a:
            continue
        k = int(a[a.index("-k") + 1])
        key = (a[a.index("-r") + 1], a[a.index("-g") + 1], k)
        if key in seen:
            continue
        seen.add(key)
        unitigs = read_unitigs(os.path.join(GOLD, key[1]))
        rb, roffs, _, _ = oracle_py.parse_file(os.path.join(GOLD, key[0]), k)
        check_pin(k, unitigs, strings(rb, roffs)[:400])
    seen.add(("soup", 15))
    unitigs = read_unitigs(os.path.join(GOLD, "soup_polyA_unitig.fa"))
    rb, roffs, _, _ = oracle_py.parse_file(os.path.join(GOLD, "soup_polyA_reads.fa"), 15)
    check_pin(15, unitigs, strings(rb, roffs)[:300], ms=(0, 2), efforts=(1, 5))
    assert len(seen) >= 3


@pytest.mark.parametrize("k", [33, 40, 47, 63, 64])
def test_wide_builds_and_key_lookups(k):
    r = random.Random(k)
    s = Synth(20000, 90, 2, k, 100 + k)
    unitigs = strings(*s.unitigs())
    K1 = k - 1
    # poly-A / poly-T ends (one word of the key all zeros / all ones) and, at an odd k, a palindromic (k-1)-mer
    extra = ["A" * K1 + "CG" + "T" * K1, "T" * (k + 3)]
    if K1 % 2 == 0:
        half = "".join(r.choice(ACGT) for _ in range(K1 // 2))
        pal = half + W.reverse_complements(half)
        extra.append(pal + "GATTACA" + pal)
    unitigs = unitigs + extra
    g = B.Graph.build(k, *pack(unitigs))
    info = g.info()
    assert info["k"] == k and info["n_unitigs"] == len(unitigs)
    ref = W.GreedyRef(k, unitigs)
    members = ref.canonical_keys()
    assert info["n_keys"] == len(members)
    assert W.str2num("A" * K1) in members and min(W.str2num("T" * K1), W.rcb(W.str2num("T" * K1), K1)) in members
    for key in members:
        assert g.key_lookup(key) is not None, hex(key)
    n = 0
    while n < 20000:
        x = r.getrandbits(2 * K1)
        if x in members:
            continue
        assert g.key_lookup(x) is None
        n += 1


def test_k65_is_refused():
    with pytest.raises(B.BgrError, match=r"\[2,64\]"):
        B.Graph.build(65, *pack(["ACGT" * 40]))


def wide_blob(k=47):
    s = Synth(20000, 90, 2, k, 5)
    return B.Graph.build(k, *s.unitigs())


def test_wide_blob_roundtrip():
    g = wide_blob()
    blob = np.array(g.blob())
    g2 = B.Graph.from_blob(blob)
    assert np.array_equal(np.array(g2.blob()), blob)
    assert g2.info() == g.info()
    assert g2.key_lookup(0) == g.key_lookup(0)


def test_wide_blob_validation_refuses_corrupt_headers():
    blob = np.array(wide_blob().blob())
    hdr = blob[:4096].view(np.uint64)
    size, n_keys = int(hdr[2]), int(hdr[4])
    # (u64 word index, new value): blob_bytes, n_keys, n_buckets, total_bases, the slots at the blob's end, and the key section moved so that
    # n_keys entries of 16 bytes would fit behind it but not the 32 of a two-word entry
    for word, val in [(2, size + 256), (4, n_keys * 4), (9, 0), (8, 1 << 40), (12, size - 256), (11, (size - n_keys * 16) // 256 * 256)]:
        b = blob.copy()
        b[:4096].view(np.uint64)[word] = val
        with pytest.raises(B.BgrError):
            B.Graph.from_blob(b)
    # the key layout field: a wide blob at k > 32 must say "two words because of k"
    for v in (0, 2, 3):
        b = blob.copy()
        b[:4096].view(np.uint32)[2 * 22 + 1] = v  # (slot_fill_x100, wide_keys) is u64 word 22
        with pytest.raises(B.BgrError):
            B.Graph.from_blob(b)
    with pytest.raises(B.BgrError):
        B.Graph.from_blob(blob[:-256].copy())


def test_wide_blob_with_k_rewritten_to_31_is_refused():
    blob = np.array(wide_blob().blob())
    b = blob.copy()
    b[:4096].view(np.uint32)[3] = 31  # (version, k) is u64 word 1
    with pytest.raises(B.BgrError):
        B.Graph.from_blob(b)


def test_narrow_blob_bytes_unchanged():
    """The k = 31 blob of a seeded graph hashes as it did before two-word keys existed (recorded at the parent commit)."""
    s = Synth(60000, 75, 2, 31, 77)
    g = B.Graph.build(31, *s.unitigs())
    assert hashlib.sha256(bytes(g.blob())).hexdigest() == "a594eb834eef96466ff5235807cb9dfc247c55cf8e1d5ae65c8a2fe9efc17f8b"


def test_wide_keys_option_builds_the_wide_layout_at_small_k():
    s = Synth(20000, 60, 2, 21, 9)
    seqs, offs = s.unitigs()
    narrow = B.Graph.build(21, seqs, offs)
    with B.options(**{"test.wide_keys": 1}):
        wide = B.Graph.build(21, seqs, offs)
    assert wide.info()["n_keys"] == narrow.info()["n_keys"]
    assert len(wide.blob()) > len(narrow.blob())
    assert int(np.array(wide.blob()[:4096]).view(np.uint32)[2 * 22 + 1]) == 2
    ref = W.GreedyRef(21, strings(seqs, offs))
    for key in ref.canonical_keys():
        assert wide.key_lookup(key) is not None
    slot = ctypes.c_uint32()
    assert B.lib().bgr_graph_key_lookup(wide.h, 0, ctypes.byref(slot)) != 0  # the one-word lookup is refused on a wide graph
    assert B.lib().bgr_graph_key_lookup(narrow.h, 0, ctypes.byref(slot)) == 0


def test_plan_wide_keys_uses_no_greedy16_pass():
    base = dict(k=63, slot_fill_x100=120, table_bytes=40000, graph_bases=2_000_000, n_unitigs=10_000, max_unitig_len=5000, mode=B.MODE_GREEDY,
                max_mismatch=2, max_read_len=150, n_reads=100_000, total_bases=15_000_000)
    assert B.plan_launch(**base)["greedy16"]["used"]
    p = B.plan_launch(wide_keys=1, **base)
    assert not p["greedy16"]["used"] and p["general"]["used"]


def test_anchors_and_filters_refused_at_k_above_32():
    s = Synth(20000, 90, 2, 40, 3)
    seqs, offs = s.unitigs()
    with pytest.raises(B.BgrError, match="k <= 32"):
        B.Graph.build(40, seqs, offs, anchors=True)
    for kind in (1, 2):
        with B.options(build_filter=kind):
            with pytest.raises(B.BgrError):
                B.Graph.build(40, seqs, offs)
