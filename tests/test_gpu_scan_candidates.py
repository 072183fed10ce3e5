"""The anchor scan's own key lookup (scan_find_key, device_common.h) on the paths the common step skips.

The scan of bgr_align_greedy_multi_kernel confirms only each lane's FIRST fingerprint candidate in the common case and sends the
rest -- lanes with candidates in both buckets or twice in one bucket -- through a general loop, and only up to the step's first
(effort >= 2: second) hit.  The reads here carry (k-1)-mers chosen on the host by brute force so that those paths are taken:
  - a non-key whose bucket and fingerprint match a key's, placed before the true first anchor of the read;
  - a non-key with fingerprint matches in both of its buckets;
  - a key that sits in its second bucket behind a false match in its first, or behind a false match lower in its own bucket;
  - keys of the sorted fallback list (a graph built with the test hook that sends keys there);
mapped with effort 1, 2 and 3 (the second hit of a step matters from 2 on), forward and reverse-complemented, against the oracle.
The table's hashing is restated from graph_layout.h (bgr_mix64, bgr_tab_bucket, bgr_tab_fp) and read out of the built graph's blob."""
import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
from tools.synth import Synth

K = 31
K1 = K - 1
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def _enc(w):
    x = 0
    for ch in w:
        x = x << 2 | CODE[ch]
    return x


def _dec(x):
    return bytes(b"ACGT"[(x >> (2 * (K1 - 1 - i))) & 3] for i in range(K1))


def _rc(s):
    return bytes({65: 84, 67: 71, 71: 67, 84: 65}[c] for c in reversed(s))


def _rc_int(x):  # numpy uint64 array: reverse complement of K1 bases (bgr_rcb)
    y = x
    for sh, mk in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        y = ((y >> U64(sh)) & U64(mk)) | ((y & U64(mk)) << U64(sh))
    y = (y >> U64(32)) | (y << U64(32))
    return (~y) >> U64(64 - 2 * K1)


def _hash(x, n_buckets):  # -> bucket 1, bucket 2, fingerprint (graph_layout.h)
    with np.errstate(over="ignore"):
        m = (x ^ (x >> U64(32))) * U64(0x9E3779B97F4A7C15)
    nb = U64(n_buckets)
    b1 = ((m & M32) * nb) >> U64(32)
    b2 = ((m >> U64(32)) * nb) >> U64(32)
    fp = (m >> U64(32)) & U64(0xFF)
    fp[fp == 0] = 1
    return b1.astype(np.int64), b2.astype(np.int64), fp.astype(np.uint8)


def _end_keys(seqs, offs):
    keys = set()
    for i in range(len(offs) - 1):
        u = bytes(seqs[int(offs[i]):int(offs[i + 1])])
        for w in (u[:K1], u[-K1:]):
            keys.add(min(_enc(w), _enc(_rc(w))))
    return keys


def _table(g):
    blob = np.array(g.blob())
    hdr = blob[:4096].view(np.uint64)
    n_buckets, off_table = int(hdr[9]), int(hdr[10])
    return n_buckets, blob[off_table:off_table + 4 * n_buckets].reshape(-1, 4)


def _special_kmers(g, seqs, offs, seed):
    """(k-1)-mers (canonical ints) that take the scan off its common path, by category"""
    n_buckets, tab = _table(g)
    keys = _end_keys(seqs, offs)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << (2 * K1), size=1 << 21, dtype=np.uint64)
    x = np.minimum(x, _rc_int(x))
    b1, b2, fp = _hash(x, n_buckets)
    n1 = (tab[b1] == fp[:, None]).sum(axis=1)
    n2 = (tab[b2] == fp[:, None]).sum(axis=1)
    out = {"false_in_bucket1": [], "false_in_both": [], "false_twice": [], "key_behind_false_b1": [], "key_behind_false_same": [], "fallback": []}
    for v, a, b in zip(x.tolist(), n1.tolist(), n2.tolist()):
        if v in keys:
            continue
        if a and b:
            out["false_in_both"].append(v)
        elif a + b >= 2:
            out["false_twice"].append(v)
        elif a and len(out["false_in_bucket1"]) < 400:
            out["false_in_bucket1"].append(v)
    kx = np.array(sorted(keys), dtype=np.uint64)
    b1, b2, fp = _hash(kx, n_buckets)
    for v, c1, c2, f in zip(kx.tolist(), b1.tolist(), b2.tolist(), fp.tolist()):
        slot = g.key_lookup(v)
        if slot >= 4 * n_buckets:
            out["fallback"].append(v)
            continue
        bk, j = divmod(slot, 4)
        if bk == c2 and bk != c1 and (tab[c1] == f).any():
            out["key_behind_false_b1"].append(v)
        elif (tab[bk][:j] == f).any():
            out["key_behind_false_same"].append(v)
    return out


def _reads(s, seqs, offs, special, seed):
    """Per special (k-1)-mer: the special one in front of the start of a unitig (the unitig's first (k-1)-mer is a key: the true first
    anchor, in the same scan step), and the special one written over a sampled read; each also reverse-complemented."""
    rng = np.random.default_rng(seed)
    base, boffs = s.reads(0, 4 * sum(len(v) for v in special.values()) + 64, 150, 2, seed + 1)
    n_u = len(offs) - 1
    out = []
    i = 0
    for cat, vals in special.items():
        for v in vals:
            w = _dec(v)
            if rng.integers(2):
                w = _rc(w)
            u = int(rng.integers(n_u))
            body = bytes(seqs[int(offs[u]):int(offs[u + 1])])[:150 - K1 - 4]
            pre = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=int(rng.integers(0, 5))))
            r1 = pre + w + body
            b = bytearray(base[int(boffs[i]):int(boffs[i + 1])])
            i += 1
            p = int(rng.integers(0, 40))
            b[p:p + K1] = w
            for r in (r1, bytes(b)):
                out.append(r)
                out.append(_rc(r))
    roffs = np.zeros(len(out) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(r) for r in out])
    return np.frombuffer(b"".join(out), dtype=np.uint8), roffs


def _case(no_evictions, seed):
    s = Synth(160000, 50, 3, K, seed)
    seqs, offs = s.unitigs()
    g = B.Graph.build(K, seqs, offs, 1.07 if no_evictions else 0.0, no_evictions=no_evictions)
    special = _special_kmers(g, seqs, offs, seed + 7)
    return s, seqs, offs, g, special


def test_special_kmers_are_what_they_claim():
    """(no GPU) the host restatement of the table agrees with the graph's own lookup: the colliding (k-1)-mers are no keys, the others are"""
    for no_evictions, seed in ((False, 31), (True, 32)):
        s, seqs, offs, g, special = _case(no_evictions, seed)
        n_buckets, tab = _table(g)
        for cat, vals in special.items():
            for v in vals[:200]:
                found = g.key_lookup(v)
                if cat.startswith("false"):
                    assert found is None, cat
                else:
                    assert found is not None, cat
                    assert (found >= 4 * n_buckets) == (cat == "fallback")
        assert len(special["false_in_bucket1"]) >= 100 and special["false_in_both"] and special["false_twice"]
        assert special["key_behind_false_b1"] and special["key_behind_false_same"]
        assert bool(special["fallback"]) == no_evictions


@pytest.mark.gpu
@pytest.mark.parametrize("no_evictions,seed", [(False, 31), (True, 32)])
def test_scan_candidates_match_oracle(no_evictions, seed):
    s, seqs, offs, g, special = _case(no_evictions, seed)
    reads, roffs = _reads(s, seqs, offs, special, seed + 11)
    al = B.Aligner(g, 0)
    al.configure(lds_mphf=2)
    o = oracle_py.Oracle(K, seqs, offs)
    for effort in (1, 2, 3):
        p1, po1, st1 = al.align(reads, roffs, m=2, effort=effort)
        info = al.launch_info()
        assert info["mphf_in_lds"] and info["four_reads_per_wave"]
        p2, po2, st2 = o.align(reads, roffs, m=2, effort=effort)
        assert np.array_equal(st1, st2), effort
        assert np.array_equal(po1, po2) and np.array_equal(p1, p2), effort
