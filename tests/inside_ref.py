"""Plain-Python reference of the inside pass (include/bgreat_gpu.h: bgr_aligner_inside_enable): the inside index -- an exact map from a
sample of the canonical k-mers of every unitig to where they lie -- and the pass that maps the reads greedy mode leaves without an anchor
because they lie wholly inside one unitig.  Slow and obvious on purpose; k <= 32.  The hashing is jump_ref.py's (the jump index's rule)."""
from jump_ref import mix64, rcb, selects

ST_NOANCHOR, ST_FAILED, ST_ALIGNED, ST_MASK, ST_RC = 0, 1, 2, 3, 4
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def canonical(x, k):
    return min(x, rcb(x, k))


def selected(x, k):
    """the k-mer word x (either strand) can be in the index: no palindrome, and the hash of its canonical form selects it"""
    r = rcb(x, k)
    return x != r and selects(mix64(min(x, r)))


def windows(s, k):
    """(i, word, word of the reverse complement) of every window s[i:i + k] that holds only ACGT, both words rolled along"""
    mask, top, x, r, good = (1 << (2 * k)) - 1, 2 * (k - 1), 0, 0, 0
    for p, ch in enumerate(s):
        c = CODE.get(ch)
        if c is None:
            good = 0
            continue
        x = ((x << 2) | c) & mask
        r = (r >> 2) | ((3 - c) << top)
        good += 1
        if good >= k:
            yield p - k + 1, x, r


def index(k, unitigs):
    """canonical k-mer -> (id from 1, offset j, the forward window is the canonical one); of a repeated k-mer the smallest (id, j)"""
    idx = {}
    for i, u in enumerate(unitigs):
        for j, x, r in windows(u, k):
            if x != r and selects(mix64(min(x, r))):
                idx.setdefault(min(x, r), (i + 1, j, x < r))
    return idx


def candidates(k, unitigs, idx, read):
    """-> [(s, +-id, characters in which the read differs)] of the candidates that lie on their unitig, in window order"""
    L = len(read)
    out = []
    for i, x, r in windows(read, k):   # (a window with a character outside ACGT is none)
        if x == r or not selects(mix64(min(x, r))):
            continue
        hit = idx.get(min(x, r))
        if hit is None:
            continue
        w = read[i:i + k]
        uid, j, _ = hit
        u = unitigs[uid - 1]
        if w == u[j:j + k]:
            s, ou, sid = j - i, u, uid
        else:
            s, ou, sid = (len(u) - k - j) - i, rc(u), -uid
        if s < 0 or s + L > len(u):
            continue
        out.append((s, sid, sum(1 for a, b in zip(read, ou[s:s + L]) if a != b)))   # (a read character outside ACGT equals no unitig character)
    return out


def map_read(k, unitigs, idx, read, m, cands=None):
    """-> [s, +-id] of the first valid candidate, or None (cands: candidates() of the read, when the caller has them)"""
    for s, sid, nm in candidates(k, unitigs, idx, read) if cands is None else cands:
        if nm <= m:
            return [s, sid]
    return None


def apply(k, unitigs, idx, reads, rows, m, cache=None):
    """rows: [(status, path)] of the mapping passes -> (the rows behind the inside pass, how many reads it mapped); cache: a dict that keeps
    the candidates of a read from call to call (they do not depend on m)"""
    out, n = [], 0
    for read, (st, path) in zip(reads, rows):
        if (st & ST_MASK) == ST_NOANCHOR and len(read) >= k:
            cands = None
            if cache is not None:
                if read not in cache:
                    cache[read] = candidates(k, unitigs, idx, read)
                cands = cache[read]
            row = map_read(k, unitigs, idx, read, m, cands)
            if row is not None:
                out.append((ST_ALIGNED, row))
                n += 1
                continue
        out.append((st, list(path)))
    return out, n
