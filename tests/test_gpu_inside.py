"""The inside pass (bgr_aligner_inside_enable, bgreat_amd/csrc/inside_kernels.hip) against its definition (inside_ref.py), read by read.

What is compared: an aligner without the switch gives the rows of the mapping passes; inside_ref.apply() says what the pass makes of them -- the
reads with status NOANCHOR it maps get [s, +-id] and ALIGNED, every other row stays -- and an aligner with the switch must return exactly
that, from ASCII reads (bgr_align_batch), from host-packed planes (bgr_align_batch_packed) and from reads parked on the device
(bgr_align_device + fetch), for m in {0, 2, 5}.  Its count must be the reference's, its counters those of the aligner without the switch.
  graph 1  three random unitigs of 400, 150 and k + 3 bases (k = 31): reads of 150 at both ends of the long one on both strands, hanging over
           an end by one base, the 150-base unitig itself, 0 .. m + 1 substitutions in the first window / so that every window is hit / in the
           last k characters, an N next to every 16- and 32-character step, and reads of k - 1 .. 300 characters around the packing's borders;
  graph 2  Synth(30000, 400, 2, k) at k = 12, 31, 32 with reads of 100 and 150: unitigs long enough that a fifth of the reads and more lie inside one;
  graph 3  the decoy unitig set of test_gpu_scan_take.py at k = 12, where k-mers repeat: the first hit of a read is often on the wrong unitig."""
import numpy as np
import pytest

import bgreat_amd as B
import inside_ref as R
import oracle_py
from tools.synth import Synth
from wide_greedy_ref import rows_of

MS = (0, 2, 5)
SEED = 3101
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def rc(s):
    return s.encode().translate(COMP)[::-1].decode()


def _rand(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


def _pack(strs):
    offs = np.zeros(len(strs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in strs])
    return np.frombuffer("".join(strs).encode(), dtype=np.uint8), offs


def _split(seqs, offs):
    s = bytes(seqs).decode()
    return [s[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def _sub(read, positions):
    r = list(read)
    for p in positions:
        r[p] = "CGTA"["ACGT".index(r[p])]
    return "".join(r)


# ---- graph 1 ----------------------------------------------------------------------------------------------------------------------------
K1 = 31


def graph1():
    rng = np.random.default_rng(SEED)
    return [_rand(rng, 400), _rand(rng, 150), _rand(rng, K1 + 3)]


def reads1(us, m):
    """-> [(what, read)]"""
    U, V, S = us
    k, L = K1, 150
    out = []
    for off in (0, 1, len(U) - L - 1, len(U) - L):
        out += [("end %d" % off, U[off:off + L]), ("end %d rc" % off, rc(U[off:off + L]))]
    for name, r in (("over left", "G" + U[:L - 1]), ("over right", U[len(U) - L + 1:] + "G"), ("over V left", "C" + V[:L - 1]), ("over V right", V[1:] + "C")):
        out += [(name, r), (name + " rc", rc(r))]
    out += [("V", V), ("V rc", rc(V)), ("S", S), ("S rc", rc(S)), ("S inner", S[1:k + 2]), ("S window", S[2:k + 2])]
    base = U[100:100 + L]
    cover = [30, 60, 90, 120, 15, 45, 75]   # every window of 31 characters holds one of the first four
    for n in range(m + 2):
        out += [("first window %d" % n, _sub(base, [2 * j for j in range(n)])), ("every window %d" % n, _sub(base, cover[:n])),
                ("last window %d" % n, _sub(base, [L - 1 - 2 * j for j in range(n)])), ("last window %d rc" % n, rc(_sub(base, [L - 1 - 2 * j for j in range(n)])))]
    for p in range(16, L, 16):
        for q in (p - 1, p):
            r = base[:q] + "N" + base[q + 1:]
            out += [("N at %d" % q, r), ("N at %d rc" % q, rc(r))]
    out.append(("two N", base[:31] + "N" + base[32:63] + "N" + base[64:]))
    for Lx in (k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300):
        r = U[50:50 + Lx]
        out += [("length %d" % Lx, r), ("length %d rc" % Lx, rc(r))]
        if Lx > k + 1:
            out.append(("length %d one off" % Lx, _sub(r, [Lx // 2])))
    return out


# ---- the cases: a graph, its reference index, an aligner without the switch and one with it ------------------------------------------------
class _Case:
    def __init__(self, k, us):
        self.k, self.us = k, us
        self.idx = R.index(k, us)
        self.cache = {}
        self.g = B.Graph.build(k, *_pack(us))
        self.g.inside_build()
        self.base = B.Aligner(self.g, 0)
        self.al = B.Aligner(self.g, 0)
        self.al.inside_enable()

    def want(self, reads, m):
        rows = rows_of(*self.base.align(*_pack(reads), m=m, effort=2))
        return rows, R.apply(self.k, self.us, self.idx, reads, rows, m, self.cache)

    def check(self, reads, m, routes=("ascii", "packed", "device")):
        """-> (rows without the switch, rows with it, reads mapped inside)"""
        rb, ro = _pack(reads)
        n = len(reads)
        rows, (want, n_in) = self.want(reads, m)
        for route in routes:
            before = self.al.inside_count()
            if route == "ascii":
                got = rows_of(*self.al.align(rb, ro, m=m, effort=2))
            elif route == "packed":
                got = rows_of(*self.al.align_packed(B.pack_reads(rb, ro), m=m, effort=2))
            else:
                d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
                try:
                    self.al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(ro[-1]), max(len(x) for x in reads), m=m, effort=2)
                    got = rows_of(*self.al.fetch(n, int(ro[-1]) + 8 * n + 8))
                finally:
                    d_r.free()
                    d_o.free()
            bad = [(i, reads[i], rows[i], want[i], got[i]) for i in range(n) if got[i] != want[i]]
            assert not bad, (route, m, len(bad), bad[:3])
            assert self.al.inside_count() - before == n_in, (route, m)
        return rows, want, n_in


_CASES = {}


def _case(key, make):
    if key not in _CASES:
        _CASES[key] = _Case(*make())
    return _CASES[key]


def _synth(k):
    s = Synth(30000, 400, 2, k, SEED + k)
    us = _split(*s.unitigs())
    reads = []
    for L in (100, 150):
        reads += _split(*s.reads(0, 300, L, 2, SEED + L))
    return k, us, reads


_SYNTH = {}


def _synth_case(k):
    if k not in _SYNTH:
        _SYNTH[k] = _synth(k)
    return _SYNTH[k]


@pytest.mark.parametrize("k", [12, 31, 32])
def test_a_fifth_of_graph_2s_reads_lie_inside_a_unitig(k):
    """(no GPU) on the oracle's rows: the share of the reads the reference maps inside, at the budget the reads were made with"""
    k, us, reads = _synth_case(k)
    o = oracle_py.Oracle(k, *_pack(us))
    rows = rows_of(*o.align(*_pack(reads), m=2, effort=2))
    _, n_in = R.apply(k, us, R.index(k, us), reads, rows, 2)
    assert 5 * n_in >= len(reads), (k, n_in, len(reads))


def test_graph_1s_reads_are_what_they_claim():
    """(no GPU) the reference on the hand-made reads, as if none had an anchor: the ends and the unitig itself map at their offsets on both strands,
    overhangs never, substitutions up to m, a read whose every window is hit never although it is within the budget, an N costs one difference"""
    us = graph1()
    idx = R.index(K1, us)
    for m in MS:
        got = {what: R.map_read(K1, us, idx, r, m) for what, r in reads1(us, m)}
        for off in (0, 1, 249, 250):
            assert got["end %d" % off] == [off, 1] and got["end %d rc" % off] == [250 - off, -1]
        assert got["V"] == [0, 2] and got["V rc"] == [0, -2]
        assert got["S"] in (None, [0, 3]) and got["S inner"] in (None, [1, 3])   # (four windows, two windows: the hash may select none)
        assert all(v is None for w, v in got.items() if w.startswith("over"))
        for n in range(m + 2):
            assert (got["first window %d" % n] == [100, 1]) == (n <= m) and (got["last window %d" % n] == [100, 1]) == (n <= m)
            assert (got["last window %d rc" % n] == [150, -1]) == (n <= m)
            assert (got["every window %d" % n] == [100, 1]) == (n <= min(m, 3)), (m, n)   # four substitutions leave no window: unmapped within the budget too
        assert all((got["N at %d" % q] == [100, 1]) == (m >= 1) for p in range(16, 150, 16) for q in (p - 1, p))
        assert got["length %d" % (K1 - 1)] is None and got["length 300"] == [50, 1] and got["length 257 rc"] == [400 - 50 - 257, -1]


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
def test_graph_1(m):
    c = _case("g1", lambda: (K1, graph1()))
    named = reads1(c.us, m)
    rows, want, n_in = c.check([r for _, r in named], m)
    by = {w: (rows[i], want[i]) for i, (w, _) in enumerate(named)}
    # the interior reads had no anchor, and the pass mapped them where the reference does
    assert by["first window 0"][0] == (B.ST_NOANCHOR, []) and by["first window 0"][1] == (B.ST_ALIGNED, [100, 1])
    assert by["last window 0 rc"][1] == (B.ST_ALIGNED, [150, -1])
    assert n_in >= 20
    # the reads in another order, and one by one (a launch of one read, a workgroup with one group at work)
    order = np.random.default_rng(SEED + m).permutation(len(named))
    c.check([named[i][1] for i in order], m, routes=("ascii",))
    for i in order[:12]:
        c.check([named[i][1]], m, routes=("ascii", "device"))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [12, 31, 32])
def test_graph_2(k):
    _, us, reads = _synth_case(k)
    c = _case(("g2", k), lambda: (k, us))
    for m in MS:
        rows, want, n_in = c.check(reads, m)
        assert all(w == r for r, w in zip(rows, want) if (r[0] & B.ST_MASK) != B.ST_NOANCHOR)   # rows of reads with an anchor are identical
        if m == 2:
            assert 5 * n_in >= len(reads)
    # the same reads cut into launches of 1, 7 and all give the same rows
    sub = reads[280:340]   # (both lengths)
    _, want, _ = c.check(sub, 2, routes=("ascii",))
    for step in (1, 7):
        got = []
        for i in range(0, len(sub), step):
            got += rows_of(*c.al.align(*_pack(sub[i:i + step]), m=2, effort=2))
        assert got == want, step


@pytest.mark.gpu
def test_graph_3_repeated_kmers():
    from test_gpu_scan_take import _pick_long
    p = _pick_long(12)
    us = _split(p.seqs, p.offs)
    c = _case("g3", lambda: (12, us))
    rng = np.random.default_rng(SEED + 3)
    reads = []
    for u in [u for u in us if len(u) >= 260][:60]:
        off = int(rng.integers(1, len(u) - 151))
        r = _sub(u[off:off + 150], [int(x) for x in rng.choice(150, size=int(rng.integers(0, 4)), replace=False)])
        reads += [r, rc(r)]
    reads += [r.decode() for r in p.noanchor] + [r.decode() for r in p.reads[:8]]
    for m in MS:
        rows, want, n_in = c.check(reads, m)
        assert n_in >= 10, (m, n_in)


@pytest.mark.gpu
def test_a_launch_of_reads_that_all_lie_inside_fills_its_rows():
    """every read of the launch takes a row from the arena through the cursor: 2 ints each, the overflow word stays 0"""
    c = _case("g1", lambda: (K1, graph1()))
    U = c.us[0]
    reads = [U[i:i + 150] for i in range(1, 250)]
    rb, ro = _pack(reads)
    n = len(reads)
    d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
    try:
        for al, inside in ((c.base, False), (c.al, True)):
            al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(ro[-1]), 150, m=0, effort=2)
            got = rows_of(*al.fetch(n, int(ro[-1]) + 8 * n + 8))
            cur = B.device_download(0, al.device_results()[2], 2, np.uint32)
            assert int(cur[1]) == 0
            if inside:
                assert got == [(B.ST_ALIGNED, [i, 1]) for i in range(1, 250)]
                assert int(cur[0]) >= 2 * n
            else:
                assert got == [(B.ST_NOANCHOR, [])] * n
    finally:
        d_r.free()
        d_o.free()


@pytest.mark.gpu
def test_kernel_times_count_and_counters():
    _, us, reads = _synth_case(31)
    g = B.Graph.build(31, *_pack(us))
    off, on = B.Aligner(g, 0), B.Aligner(g, 0)
    with pytest.raises(B.BgrError, match="no inside index"):
        on.inside_enable()
    g.inside_build()
    on.inside_enable()
    rb, ro = _pack(reads)
    rows = rows_of(*off.align(rb, ro, m=2, effort=2))
    want, n_in = R.apply(31, us, R.index(31, us), reads, rows, 2)
    assert rows_of(*on.align(rb, ro, m=2, effort=2)) == want
    assert on.inside_count() == n_in > 0 and off.inside_count() == 0
    assert on.counters() == off.counters()   # no_overlap still counts the reads without an anchor, those mapped inside included
    assert on.counters()["no_overlap"] >= n_in
    names_on, names_off = [n for n, _ in on.kernel_times()[1]], [n for n, _ in off.kernel_times()[1]]
    assert "bgr_align_inside_kernel" in names_on and "bgr_align_inside_kernel" not in names_off
    assert [n for n in names_on if n != "bgr_align_inside_kernel"] == names_off
    # switched off again: the launch of an aligner without the switch
    on.inside_enable(False)
    assert rows_of(*on.align(rb, ro, m=2, effort=2)) == rows and on.inside_count() == n_in
    on.reset_counters()
    assert on.inside_count() == 0
    # an exhaustive launch of an enabled aligner is refused
    on.inside_enable()
    with pytest.raises(B.BgrError, match="exhaustive"):
        on.align(rb, ro, m=2, effort=2, mode=B.MODE_EXHAUSTIVE)
    # anchors mode (-G) maps these reads itself: the pass finds none left, and the rows are those without it
    ga = B.Graph.build(31, *_pack(us), anchors=True)
    ga.inside_build()
    a0, a1 = B.Aligner(ga, 0), B.Aligner(ga, 0)
    a1.inside_enable()
    r0 = rows_of(*a0.align(rb, ro, m=2, effort=2, mode=B.MODE_ANCHORS))
    want_a, n_a = R.apply(31, us, R.index(31, us), reads, r0, 2)
    assert rows_of(*a1.align(rb, ro, m=2, effort=2, mode=B.MODE_ANCHORS)) == want_a and a1.inside_count() == n_a
