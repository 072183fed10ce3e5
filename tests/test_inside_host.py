"""The inside index as the host builds it (bgreat_amd/csrc/inside_index.cpp) against its definition (inside_ref.py), through the diagnostic
bgr_graph_inside_lookup: every k-mer of every unitig on both strands and k-mers the graph does not hold, at k = 5, 12 (even: palindromes
planted), 31 and 32 (the full word); the duplicate rule on a unitig set that repeats k-mers; the refusals; the table's numbers.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import bgreat_amd as B
import inside_ref as R
from jump_ref import kint, rcb

SEED = 2901


def _rand(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


def _pack(us):
    offs = np.zeros(len(us) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(u) for u in us])
    return np.frombuffer("".join(us).encode(), dtype=np.uint8), offs


def _unitigs(k, rng):
    us = [_rand(rng, int(n)) for n in rng.integers(k, 300, size=40)] + [_rand(rng, k), _rand(rng, k + 1), _rand(rng, 2000)]
    if k % 2 == 0:   # palindromes: a k-mer that is its own reverse complement, inside a unitig, at its start and at its end
        h = _rand(rng, k // 2)
        pal = h + R.rc(h)
        assert kint(pal) == rcb(kint(pal), k)
        us += [_rand(rng, 30) + pal + _rand(rng, 30), pal + _rand(rng, 20), _rand(rng, 20) + pal, pal]
    return us


def _check_table(k, us, g):
    idx = R.index(k, us)
    info = g.inside_info()
    assert info["entries"] == len(idx)
    seen = set()
    for u in us:
        for s in (u, R.rc(u)):
            for j in range(len(s) - k + 1):
                x = kint(s[j:j + k])
                if x in seen:
                    continue
                seen.add(x)
                assert g.inside_lookup(x) == idx.get(R.canonical(x, k)), (k, s[j:j + k])
    return idx, info


@pytest.mark.parametrize("k", [5, 12, 31, 32])
def test_table_is_the_definitions_index(k):
    rng = np.random.default_rng(SEED + k)
    us = _unitigs(k, rng)
    g = B.Graph.build(k, *_pack(us))
    assert g.inside_info() == {"entries": 0, "slots": 0, "bytes": 0, "build_seconds": 0.0}
    with pytest.raises(B.BgrError):
        g.inside_lookup(0)
    blob = bytes(g.blob())
    g.inside_build()
    idx, info = _check_table(k, us, g)
    assert bytes(g.blob()) == blob   # the index is no part of the blob
    # about one k-mer in four is selected (k = 5 has few distinct k-mers: no statement there), palindromes never
    windows = sum(len(u) - k + 1 for u in us)
    if k >= 12:
        assert 0.15 * windows < len(idx) < 0.35 * windows
    for x in idx:
        assert x != rcb(x, k) and R.selected(x, k)
    # k-mers the graph does not hold are not found; at k = 32 the word uses all 64 bits
    held = {R.canonical(kint(u[j:j + k]), k) for u in us for j in range(len(u) - k + 1)}
    n_absent = 0
    for _ in range(2000):
        x = kint(_rand(rng, k))
        if R.canonical(x, k) not in held:
            assert g.inside_lookup(x) is None
            n_absent += 1
    assert n_absent > 1000 or k == 5   # (a few thousand bases hold every 5-mer there is)
    for x in (0, (1 << (2 * k)) - 1):   # A^k and T^k: one canonical form, 0 -- and T^32 is the word of an empty slot
        assert g.inside_lookup(x) == idx.get(0)
    # the table's numbers: 16 bytes per slot, load at most 0.5, sticky
    assert info["bytes"] == 16 * info["slots"] and info["slots"] >= 2 * info["entries"] and info["slots"] >= 16
    assert info["slots"] <= max(16, 2 * windows)
    g.inside_build()
    assert g.inside_info() == info


def test_of_a_repeated_kmer_the_smallest_id_and_offset_wins():
    k = 12
    rng = np.random.default_rng(SEED)
    core = _rand(rng, 60)
    # the same 60 bases in four unitigs at different offsets, once reversed: every k-mer of `core` occurs four times
    us = [_rand(rng, 25) + core + _rand(rng, 10), core, _rand(rng, 5) + R.rc(core) + _rand(rng, 40), _rand(rng, 50) + core[:30], core[20:] + core[:25]]
    g = B.Graph.build(k, *_pack(us))
    g.inside_build()
    idx, _ = _check_table(k, us, g)
    inner = [R.canonical(kint(core[j:j + k]), k) for j in range(len(core) - k + 1)]
    hits = [idx[x] for x in inner if x in idx]
    assert len(hits) >= 5 and all(uid == 1 for uid, _, _ in hits)   # unitig 1 holds them all, at offset 25 + j
    assert {j for _, j, _ in hits} <= set(range(25, 25 + len(core)))
    # a k-mer twice in ONE unitig: the smaller offset
    rep = _rand(rng, k + 3)
    us2 = [_rand(rng, 7) + rep + _rand(rng, 9) + rep + _rand(rng, 4)]
    g2 = B.Graph.build(k, *_pack(us2))
    g2.inside_build()
    idx2, _ = _check_table(k, us2, g2)
    for j in range(4):
        x = R.canonical(kint(rep[j:j + k]), k)
        if x in idx2:
            assert idx2[x][1] == 7 + j


def test_refusals():
    rng = np.random.default_rng(SEED + 1)
    wide = B.Graph.build(33, *_pack([_rand(rng, 80), _rand(rng, 50)]))
    with pytest.raises(B.BgrError, match="k <= 32"):
        wide.inside_build()
    exc = B.Graph.build(15, *_pack([_rand(rng, 40) + "N" + _rand(rng, 40), _rand(rng, 50)]))
    assert exc.info()["has_exceptions"]
    with pytest.raises(B.BgrError, match="ACGT"):
        exc.inside_build()
    for g in (wide, exc):   # nothing was built: the switch of whole runs has nothing to switch on
        assert g.inside_info()["slots"] == 0
        with pytest.raises(B.BgrError, match="no inside index"):
            g.inside_enable()
        assert not g.inside_enabled()
    ok = B.Graph.build(15, *_pack([_rand(rng, 90)]))
    with pytest.raises(B.BgrError, match="no inside index"):
        ok.inside_enable()
    ok.inside_build()
    ok.inside_enable()
    assert ok.inside_enabled() and ok.inside_count() == 0
    ok.inside_enable(False)
    assert not ok.inside_enabled()
    # a graph made from a blob is indexed from its 2-bit store like any other
    us = [_rand(rng, 90), _rand(rng, 40)]
    twin = B.Graph.from_blob(B.Graph.build(15, *_pack(us)).blob())
    twin.inside_build()
    _check_table(15, us, twin)


def test_run_options_keep_their_size_and_the_symbols_are_declared():
    assert C.sizeof(B.RunOptions) == 80
    assert all(s in B.SYMBOLS for s in ("bgr_graph_inside_build", "bgr_graph_inside_info", "bgr_graph_inside_lookup", "bgr_aligner_inside_enable",
                                        "bgr_aligner_inside_count", "bgr_graph_inside_enable", "bgr_graph_inside_enabled", "bgr_graph_inside_count"))
