"""The far probe and the compare past mismatches of the jump in front of the anchor scan (bgreat_amd/csrc/greedy_kernels.hip, graph_layout.h:
BGR_JUMP_NEAR / BGR_JUMP_FAR), against the oracle, row by row.  An item hashes its first 8 windows and 4 windows that start 8 + (k-1) bases
in (no base shared), probes one of either set, compares the read with the unitig along the diagonal of the entry that hit -- past every
mismatch -- and leaves the scan the range between its first and its last unverified window, with the verified unitig end as a fallback.

Every set runs with the index used, ignored (KNOB_GREEDY_JUMP 1) and lossy (test.jump_drop), through packed planes and through ASCII reads
parked on the device, on a tools.synth graph of 20 kb at k = 31 and on one of 3 kb at k = 12 (both pass property P: asserted).  Shapes:
  1. one substitution that every near window holds (and one in front of, at the edge of and behind them), in reads that lie inside one
     unitig, cross a unitig end in front of the substitution, or cross one behind it: the far window decides;
  2. chimeras: the interior of unitig Y up to position x, then unitig Z from its first base -- window x is Z's first (k-1)-mer, a key among
     the windows the compare cannot verify; x over every residue mod 16; Y's own end in front of x (the read runs to Y's last base),
     straddling x (the window that must not count as verified) and behind x;
  3. the far window in the NEXT unitig (the strand starts above the item's first position), with and without a key below its start;
  4. two substitutions k-2, k-1 and k bases apart (the unverified ranges touch, merge, separate), and three;
  5. short reads, k .. 8 + 2 (k-1) + 8 bases: the far windows absent, partly there, all there;
  6. follow-up items: the first anchor fails (three substitutions right behind it, which every near window of the follow-up item holds:
     picked with the oracle, not aligned forward at effort 1), the resume position over every residue mod 16.
A host-only test checks that the crafted sets are what they claim."""
import pytest

import bgreat_amd as B
import jump_ref as J
import oracle_py
from tools.synth import Synth
from test_gpu_jump_scan import _Graph, _anchors, _keys, _pack, _rc, _sub

SEED = 4101
NEAR = 8  # BGR_JUMP_NEAR: the far windows start NEAR + (k-1) bases in
#    k: (genome, site spacing, read length, substitution positions of shape 1, the chimeras' x)
SETS = {31: (20000, 140, 150, (0, 5, 11, 29, 37), range(40, 111)),
        12: (3000, 150, 90, (0, 3, 8, 10, 18), range(20, 52))}


class _Set:
    pass


_SETS = {}


def _set(k):
    """the graph's unitigs, key set and crafted reads per shape (host only; worked out once)"""
    if k in _SETS:
        return _SETS[k]
    G, d, L, sub_pos, xs = SETS[k]
    k1 = k - 1
    far0 = NEAR + k1
    p = _Set()
    p.k, p.k1, p.L = k, k1, L
    for seed in range(SEED + k, SEED + k + 40):   # (k = 12: a genome of a few kb passes property P for most seeds, not for all)
        s = Synth(G, d, 2, k, seed)
        p.seqs, p.offs = s.unitigs()
        units = J.split(p.seqs, p.offs)
        if J.property_p(k, units):
            break
    else:
        raise AssertionError("no seed gives a graph with property P")
    p.units = [u.encode() for u in units]
    p.K = K = _keys(p.units, k1)
    base, _ = s.reads(0, 400, L, 0, SEED + 1)
    fw = [bytes(base[i * L:(i + 1) * L]) for i in range(400)]
    anch = [_anchors(r, K, k1) for r in fw]
    p.seen = set()
    shapes = {}

    # 1: one substitution, the read inside one unitig / across an end in front of it / across one behind it
    out = []
    for r, A in list(zip(fw, anch))[:70]:
        for q in sub_pos:
            out.append(_sub(r, q))
            p.seen.add("1 inside" if not A else "1 end in front" if A[0] + k1 <= q else "1 end behind" if A[0] > q else "1 end on it")
    shapes[1] = out

    # 2: chimeras
    longs = sorted(p.units, key=len, reverse=True)
    ys = [y for y in longs if len(y) >= xs[-1] + 2 * k1 + 2][:3]
    assert ys, "no unitig long enough for the chimeras"
    zs = [z for z in p.units if z not in ys][:40]
    out, p.chim = [], []
    for n, x in enumerate(xs):
        for gap in (0, 5, k1 + 9):               # Y's last (k-1)-mer would end `gap` bases behind x
            y = ys[n % len(ys)]
            o = len(y) - x - gap
            first = x - k1 if gap == 0 else x    # the read holds Y's own end only when it runs to Y's last base
            # (a Z whose junction with Y makes a key by chance in front of x -- a unitig of k bases in front of Z, at k = 12 -- is passed over)
            for z in zs[(n * 3 + gap) % len(zs):]:
                r = (y[o:o + x] + z)[:L]
                if len(r) >= x + k1 and _anchors(r, K, k1)[0] == first:
                    break
            else:
                continue
            out.append(r)
            p.chim.append((r, first))
            p.seen.add("2 x mod 16 = %d" % (x % 16))
            p.seen.add("2 Y's end %s x" % ("in front of" if gap == 0 else "straddles" if gap < k1 else "behind"))
    shapes[2] = out

    # 3: the far window in the next unitig: the largest key position at or below the first far window is where its strand starts
    out = []
    for r, A in zip(fw, anch):
        below = [a for a in A if a <= far0]
        if not below or below[-1] == 0:
            continue
        kind = "3 key below the strand's start" if len(below) > 1 else "3 no key below the strand's start"
        if sum(1 for x in p.seen if x == kind) and len(out) > 240:
            continue
        p.seen.add(kind)
        out += [r, _sub(r, sub_pos[2]), _sub(r, sub_pos[3])]
    shapes[3] = out[:300]

    # 4: two substitutions k-2, k-1, k apart; three
    out = []
    for r in fw[70:110]:
        for q in (3, far0 + 2, L // 2):
            for dist in (k - 2, k - 1, k):
                if q + dist < L:
                    out.append(_sub(_sub(r, q), q + dist))
        out.append(_sub(_sub(_sub(r, 4), L // 2), L - 5))
        out.append(_sub(_sub(_sub(r, far0 + k1 + 1), far0 + k1 + 3), far0 + k1 + 2 * k))
    shapes[4] = out

    # 5: short reads
    out = []
    for r, A in list(zip(fw, anch))[110:118]:
        for n in range(k, NEAR + 2 * k1 + 8 + 1):
            out += [r[:n], _sub(r[:n], min(sub_pos[2], n - 1))]
    shapes[5] = out

    # 6: reads whose first anchor fails, cut in front so that the follow-up item's resume position takes every residue mod 16
    o = oracle_py.Oracle(k, p.seqs, p.offs)
    cand = []
    for r, A in zip(fw, anch):
        if len(A) < 2 or A[0] + k1 + 4 >= len(r):
            continue
        bad = _sub(_sub(_sub(r, A[0] + k1 + 1), A[0] + k1 + 2), A[0] + k1 + 3)
        cand += [(bad[c:], A[0] - c) for c in range(0, min(A[0], 16))]
    data, roffs = _pack([c[0] for c in cand])
    st = o.align(data, roffs, m=2, effort=1)[2]
    picked = {}
    for (r, a), x in zip(cand, st.tolist()):
        if x != B.ST_ALIGNED and _anchors(r, K, k1)[0] == a:   # the first anchor is still there and does not map the read forward
            picked.setdefault((a + 1) % 16, []).append(r)
    for res, lst in picked.items():
        p.seen.add("6 resume mod 16 = %d" % res)
    fill = [r for r, A in zip(fw, anch) if A][:14]
    out = []
    for res in sorted(picked):
        out += picked[res][:2] + fill + picked[res][:1]          # the first, the second and the last group of a wave
    shapes[6] = out
    p.shapes = shapes
    _SETS[k] = p
    return p


WANT = ({"1 inside", "1 end in front", "1 end behind", "2 Y's end in front of x", "2 Y's end straddles x", "2 Y's end behind x",
         "3 key below the strand's start", "3 no key below the strand's start"}
        | {"2 x mod 16 = %d" % i for i in range(16)} | {"6 resume mod 16 = %d" % i for i in range(16)})


@pytest.mark.parametrize("k", sorted(SETS))
def test_crafted_sets_are_what_they_claim(k):
    p = _set(k)
    assert not (WANT - p.seen), sorted(WANT - p.seen)
    for r, first in p.chim:   # a chimera's first anchor is x, or Y's own end when the read holds it
        assert _anchors(r, p.K, p.k1)[0] == first
    for n, reads in p.shapes.items():
        assert 50 <= len(reads) <= 1300, (n, len(reads))


_GRAPHS = {}


def _graph(k, drop):
    if (k, drop) not in _GRAPHS:
        p = _set(k)
        g = _Graph(k, p.seqs, p.offs, drop)
        assert g.info["jump_entries"] > 0 and g.info["jump_absent"] == 0, g.info
        _GRAPHS[(k, drop)] = g
    return _GRAPHS[(k, drop)]


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [0, 3])
@pytest.mark.parametrize("shape", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("k", sorted(SETS))
def test_far_probe_and_range(k, shape, drop):
    reads = _set(k).shapes[shape]
    g = _graph(k, drop)
    g.check([x for r in reads for x in (r, _rc(r))], efforts=(2, 3) if shape == 6 else (2,))
