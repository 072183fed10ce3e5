"""Crafted and random unitig sets for the --recompact tests (recompact_ref.py has the definition they are checked against)."""
import random

import numpy as np

from recompact_ref import rc


def to_arrays(unitigs):
    """-> (seqs uint8, offs uint64) as B.Graph.build takes them"""
    seqs = np.frombuffer("".join(unitigs).encode(), dtype=np.uint8).copy()
    offs = np.zeros(len(unitigs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(u) for u in unitigs])
    return seqs, offs


def random_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def unique_seq(rng, n, k, circular=False):
    """n characters without a repeated (k-1)-mer on either strand (and none that is its own reverse complement); circular: also over the wrap"""
    K = k - 1
    while True:
        s = random_seq(rng, n)
        t = s + s[:K] if circular else s
        seen = set()
        ok = True
        for i in range(n if circular else n - K + 1):   # (a ring has n windows: the one over the wrap's end is the first again)
            w = t[i:i + K]
            r = rc(w)
            if w in seen or r in seen or w == r:
                ok = False
                break
            seen.add(w)
        if ok:
            return s


def cut(rng, s, k, pieces, circular=False, strands=True, shuffle=True):
    """s cut into `pieces` unitigs that overlap in k - 1 characters, each of at least k; circular: s is a ring and the last piece runs over the wrap"""
    K = k - 1
    n = len(s)
    t = s + s[:K] if circular else s
    starts = sorted(rng.sample(range(1, n - (0 if circular else K)), pieces - 1)) if pieces > 1 else []
    starts = [0] + starts
    ends = starts[1:] + [n]
    out = [t[a:b + K] if (circular or b < n) else t[a:b] for a, b in zip(starts, ends)]
    out = [u for u in out if len(u) >= k]
    if strands:
        out = [rc(u) if rng.random() < 0.5 else u for u in out]
    if shuffle:
        rng.shuffle(out)
    return out


def chain_set(seed, k, pieces, circular=False, piece_len=None, first_rc=None):
    """a linear or circular sequence without repeated (k-1)-mers, cut into exactly `pieces` unitigs in random strands and random order.  piece_len: the
    new characters per piece (default k + 3).  first_rc: unitig 1 is the piece that holds the sequence's start, stored reverse-complemented or not"""
    rng = random.Random(seed)
    K = k - 1
    step = piece_len or (k + 3)
    n = pieces * step + (0 if circular else K)
    s = unique_seq(rng, n, k, circular)
    t = s + s[:K] if circular else s
    fw = [t[i * step:i * step + step + K] for i in range(pieces)]
    us = [rc(u) if rng.random() < 0.5 else u for u in fw]
    if first_rc is None:
        rng.shuffle(us)
        return us, s
    rest = us[1:]
    rng.shuffle(rest)
    return [rc(fw[0]) if first_rc else fw[0]] + rest, s


def fuzz_set(seed, k):
    """1 .. 40 unitigs of k .. 3k characters; one set in three has a linear or circular sequence cut into overlapping pieces in random strands"""
    rng = random.Random(seed * 7919 + k)
    n = rng.randint(1, 40)
    us = []
    if seed % 3 == 0:
        pieces = rng.randint(2, 12)
        circular = rng.random() < 0.5
        L = rng.randint(pieces * 3 + k, pieces * 2 * k + k)
        s = random_seq(rng, L)
        us = [u for u in cut(rng, s, k, pieces, circular) if len(u) <= 3 * k] or []
    while len(us) < n:
        r = rng.random()
        if r < 0.08 and us:
            us.append(rng.choice(us))                       # a duplicate
        elif r < 0.16:
            h = random_seq(rng, k - 1)
            us.append(h + random_seq(rng, rng.randint(1, k)) + rc(h))   # a hairpin: ends with the reverse complement of its beginning
        elif r < 0.24:
            h = random_seq(rng, k - 1)
            us.append(h + random_seq(rng, rng.randint(1, k)) + h)       # a self-loop
        elif r < 0.40 and us:
            e = rng.choice(us)
            e = e if rng.random() < 0.5 else rc(e)
            us.append(e[-(k - 1):] + random_seq(rng, rng.randint(1, 2 * k)))   # begins with what another ends with
        else:
            us.append(random_seq(rng, rng.randint(k, 3 * k)))
    us = us[:max(n, 1)]
    keep = [1 if rng.random() < 0.8 else 0 for _ in us]
    return us, keep
