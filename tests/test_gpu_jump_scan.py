"""The jump in front of the anchor scan of the sixteen-reads-per-wave greedy kernel (key table in LDS; bgreat_amd/csrc/greedy_kernels.hip,
graph_layout.h: jump index), against the oracle, row by row, and with the index ignored (KNOB_GREEDY_JUMP 1) against itself.

  - parity: synthetic graphs of 20-50 kb at k = 31, 32 (one-word keys at their widest), 12 and 5 (windows shorter than a dword), 3 000 reads
    with 0-2 substitutions on both strands, effort 2 and 0 (one position per read), and the same with the builder's drop hook on (a lossy
    index).  At k = 12 and 5 a genome of that size breaks property P (chance repeats of short (k-1)-mers), so those graphs get no index and
    run as before; two small hand-made compacted graphs at k = 12 and 5 do get one.
  - crafted reads on a k = 31 graph with long unitigs: a substitution inside the probed windows, between them and the first anchor, inside
    the anchor's window, behind it, and in the last base of a read that lies wholly inside one unitig; reads that start 0-3 bases in front of
    a junction (k-1)-mer; reads of k-1 .. k+3 bases; a palindromic (k-1)-mer under the probes; reads whose first anchor fails (three
    substitutions behind it) so that the follow-up item jumps from a_pos + 1, at every residue of a_pos + 1 mod 16, in the first and the last
    group of a wave; a 470-base read among short ones.
  - the gate: a unitig set in which an interior (k-1)-mer of one unitig is the end of another has no index, says why, and maps as the oracle does.
Rows are compared through packed planes and through ASCII reads parked on the device."""
import numpy as np
import pytest

import bgreat_amd as B
import jump_ref as J
import oracle_py
from tools.synth import Synth

COMP = bytes.maketrans(b"ACGT", b"TGCA")
SEED = 2301


def _rc(r):
    return r.translate(COMP)[::-1]


def _pack(reads):
    roffs = np.zeros(len(reads) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), roffs


def _concat(units):
    offs = np.zeros(len(units) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(u) for u in units])
    return np.frombuffer(b"".join(units), dtype=np.uint8), offs


def _rand(rng, n):
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=n))


def _sub(r, pos):
    return r[:pos] + bytes([b"CGTA"[b"ACGT".index(r[pos])]]) + r[pos + 1:]


def _keys(units, k1):
    K = set()
    for u in units:
        for x in (u[:k1], u[len(u) - k1:]):
            K.add(x)
            K.add(_rc(x))
    return K


def _anchors(r, K, k1):
    return [j for j in range(len(r) - k1 + 1) if r[j:j + k1] in K]


class _Graph:
    """a graph, its oracle, and two aligners with the key table in LDS: one that jumps, one that ignores the index"""

    def __init__(self, k, seqs, offs, drop=0):
        self.k = k
        B.set_option("test.jump_drop", drop)
        try:
            self.g = B.Graph.build(k, seqs, offs)
        finally:
            B.set_option("test.jump_drop", 0)
        self.info = self.g.jump_info()
        self.o = oracle_py.Oracle(k, seqs, offs)
        self.on, self.off = B.Aligner(self.g, 0), B.Aligner(self.g, 0)
        for al in (self.on, self.off):
            al.configure(lds_mphf=2)
        self.off.set_knob(B.KNOB_GREEDY_JUMP, 1)

    def check(self, reads, efforts=(2,), m=2, ascii_route=True):
        data, roffs = _pack(reads)
        n = len(reads)
        for effort in efforts:
            want = self.o.align(data, roffs, m=m, effort=effort)
            rows = {}
            for name, al in (("jump", self.on), ("no jump", self.off)):
                rows[name] = al.align(data, roffs, m=m, effort=effort)
                info = al.launch_info()
                assert info["mphf_in_lds"] and info["four_reads_per_wave"], (name, info)
            if ascii_route:
                dr, do = B.DeviceBuffer(0, data), B.DeviceBuffer(0, roffs)
                try:
                    self.on.align_device(dr.data_ptr(), do.data_ptr(), n, int(roffs[-1]), max(len(r) for r in reads), m=m, effort=effort)
                    rows["jump, ascii"] = self.on.fetch(n, int(roffs[-1]) + 8 * n + 8)
                finally:
                    dr.free()
                    do.free()
            for name, (p1, po1, st1) in rows.items():
                assert np.array_equal(st1, want[2]), (name, effort, np.nonzero(st1 != want[2])[0][:8])
                assert np.array_equal(po1, want[1]) and np.array_equal(p1, want[0]), (name, effort)
        return want


# ---- parity on synthetic graphs ------------------------------------------------------------------------------------------------------
#       k: (genome, site spacing, read length)
SYNTH = {31: (40000, 140, 150), 32: (30000, 140, 150), 12: (20000, 40, 100), 5: (20000, 25, 60)}
_SYNTH = {}


def _synth(k, drop):
    if (k, drop) not in _SYNTH:
        G, d, L = SYNTH[k]
        s = Synth(G, d, 2, k, SEED + k)
        seqs, offs = s.unitigs()
        base, _ = s.reads(0, 1500, L, 2, SEED + 1)
        fw = [bytes(base[i * L:(i + 1) * L]) for i in range(1500)]
        g = _Graph(k, seqs, offs, drop)
        g.reads = [x for r in fw for x in (r, _rc(r))]
        _SYNTH[(k, drop)] = g
    return _SYNTH[(k, drop)]


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [0, 3])
@pytest.mark.parametrize("k", sorted(SYNTH))
def test_parity_synthetic(k, drop):
    g = _synth(k, drop)
    if k >= 31:
        assert g.info["jump_entries"] > 0 and g.info["jump_absent"] == 0
    g.check(g.reads, efforts=(2, 0))


def _chain(rng, k, lens):
    """unitigs that follow each other with k-1 bases of overlap, cut from one sequence all of whose (k-1)-mers are distinct (canonical forms):
    no interior (k-1)-mer is another unitig's end.  Grown base by base, started again when no base fits."""
    k1 = k - 1
    total = sum(lens) - k1 * (len(lens) - 1)
    while True:
        s = _rand(rng, k1)
        used = {min(s, _rc(s))}
        while len(s) < total:
            for c in rng.permutation(4):
                w = s[len(s) - k1 + 1:] + b"ACGT"[c:c + 1]
                if min(w, _rc(w)) not in used:
                    used.add(min(w, _rc(w)))
                    s += b"ACGT"[c:c + 1]
                    break
            else:
                break
        if len(s) == total:
            break
    units, at = [], 0
    for n in lens:
        units.append(s[at:at + n])
        at += n - k1
    return s, units


@pytest.mark.gpu
@pytest.mark.parametrize("k,lens", [(12, (300, 90, 12, 500, 45)), (5, (30, 9, 22, 5, 14))])
def test_parity_small_k_with_an_index(k, lens):
    rng = np.random.default_rng(SEED + 50 + k)
    s, units = _chain(rng, k, lens)
    g = _Graph(k, *_concat(units))
    assert g.info["jump_entries"] > 0, g.info
    reads = []
    for i in range(400):
        n = int(rng.integers(k - 1, min(len(s), 120) + 1))
        at = int(rng.integers(0, len(s) - n + 1))
        r = s[at:at + n]
        for _ in range(int(rng.integers(0, 3))):
            r = _sub(r, int(rng.integers(0, n)))
        reads += [r, _rc(r)]
    g.check(reads, efforts=(2, 0, 3))


# ---- crafted reads --------------------------------------------------------------------------------------------------------------------
_CRAFT = {}


def _craft():
    if _CRAFT:
        return _CRAFT["g"]
    k, k1, L = 31, 30, 150
    s = Synth(30000, 400, 2, k, SEED + 7)
    seqs, offs = s.unitigs()
    units = J.split(seqs, offs)
    units = [u.encode() for u in units]
    rng = np.random.default_rng(SEED + 8)
    half = _rand(rng, 15)
    lone = _rand(rng, 5) + half + _rc(half) + _rand(rng, 200)   # a palindromic 30-mer at offset 5 of a unitig on its own
    units.append(lone)
    g = _Graph(k, *_concat(units))
    assert g.info["jump_entries"] > 0, g.info
    K = _keys(units, k1)
    base, _ = s.reads(0, 900, L, 0, SEED + 9)
    fw = [bytes(base[i * L:(i + 1) * L]) for i in range(900)]
    long_base, _ = s.reads(0, 6, 470, 0, SEED + 10)
    g.long = [bytes(long_base[i * 470:(i + 1) * 470]) for i in range(6)]
    g.k1, g.K, g.fw, g.lone = k1, K, fw, lone
    g.anch = [_anchors(r, K, k1) for r in fw]
    _CRAFT["g"] = g
    return g


@pytest.mark.gpu
def test_crafted_substitutions_and_starts():
    g = _craft()
    k1 = g.k1
    reads, seen = [], set()
    for r, A in zip(g.fw, g.anch):
        if not A:
            reads += [_sub(r, len(r) - 1), _sub(r, 3), r]               # wholly inside one unitig: the last base, a probed window, untouched
            seen.add("inside")
            continue
        a = A[0]
        reads += [_sub(r, 5), _sub(r, k1 + 8)]                          # inside the probed windows (bases 0 .. k1 + 10)
        if a > k1 + 14:
            reads.append(_sub(r, (k1 + 12 + a) // 2))                   # between them and the first anchor
            seen.add("between")
        reads.append(_sub(r, a + k1 // 2))                              # inside the anchor's window
        if a + k1 + 3 < len(r):
            reads.append(_sub(r, a + k1 + 3))                           # behind it
        if a >= 3:
            reads += [r[a - d:] for d in (0, 1, 2, 3)]                  # the junction (k-1)-mer at position 0, 1, 2, 3
            reads += [r[a - 2:a - 2 + n] for n in range(k1, k1 + 5)]    # k-1 .. k+3 bases, across a junction
            seen.add("starts")
        reads += [r[:n] for n in range(k1, k1 + 5)]                     # ... and inside a unitig
        if len(reads) > 2600:
            break
    assert seen == {"inside", "between", "starts"}
    # the first (k-1)-mer of a unitig on its own, its last one, and the palindrome under each probe lane
    lone = g.lone
    reads += [lone[:150], lone[len(lone) - k1:], lone[len(lone) - 100:], _rc(lone)[:120]] + [lone[o:o + 140] for o in range(0, 9)] + [_rc(lone[o:o + 140]) for o in range(0, 9)]
    reads = [x for r in reads for x in (r, _rc(r))]
    g.check(reads, efforts=(2, 0, 1, 3))


@pytest.mark.gpu
def test_follow_up_items_jump_from_behind_a_failed_anchor():
    g = _craft()
    k1 = g.k1
    picked = {}
    for r, A in zip(g.fw, g.anch):
        if len(A) < 2 or A[0] + k1 + 4 >= len(r):
            continue
        bad = _sub(_sub(_sub(r, A[0] + k1 + 1), A[0] + k1 + 2), A[0] + k1 + 3)   # three substitutions behind the first anchor: it fails at m = 2
        for c in range(0, min(A[0], 16)):
            res = (A[0] - c + 1) % 16
            if res not in picked:
                picked[res] = bad[c:]
    assert set(picked) == set(range(16))
    fill = [r for r, A in zip(g.fw, g.anch) if A][:14]
    reads = []
    for res in range(16):
        reads += [picked[res]] + fill + [picked[res]]          # the first and the last group of a wave
    g.check(reads, efforts=(2, 3, 1))
    g.check([_rc(r) for r in reads], efforts=(2,), ascii_route=False)


@pytest.mark.gpu
def test_a_long_read_among_short_ones():
    g = _craft()
    rng = np.random.default_rng(SEED + 11)
    shorts = [r[o:o + int(rng.integers(31, 41))] for r in g.fw[:60] for o in (0, 50, 100)]
    reads = []
    for j, r in enumerate(g.long):
        at = (0, 15, 7, 1, 8, 14)[j]
        wave = [shorts[(15 * j + q) % len(shorts)] for q in range(15)]
        reads += wave[:at] + [r] + wave[at:]
    g.check(reads, efforts=(2, 3))
    g.check([_rc(r) for r in reads], efforts=(2,), ascii_route=False)


# ---- the gate -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gate_no_index_when_an_interior_kmer_is_a_key():
    k, k1 = 31, 30
    s = Synth(20000, 300, 2, k, SEED + 20)
    seqs, offs = s.unitigs()
    units = [u.encode() for u in J.split(seqs, offs)]
    long_u = max(units, key=len)
    rng = np.random.default_rng(SEED + 21)
    units.append(_rand(rng, 40) + long_u[60:60 + k1])           # ends with an interior (k-1)-mer of another unitig
    g = _Graph(k, *_concat(units))
    assert g.info["jump_entries"] == 0 and g.info["jump_bytes"] == 0 and g.info["jump_absent"] == 5 and "interior" in g.info["jump_absent_why"]
    base, _ = s.reads(0, 500, 150, 2, SEED + 22)
    fw = [bytes(base[i * 150:(i + 1) * 150]) for i in range(500)]
    assert len(long_u) > 250
    reads = fw + [long_u[o:o + 150] for o in range(0, 60, 7) if o + 150 <= len(long_u)]
    g.check([x for r in reads for x in (r, _rc(r))], efforts=(2, 0))
