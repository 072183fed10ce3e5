"""Per-base depth and mismatches on the unitigs (`--pileup`, `--depth`, bgr_pileup_base, bgr_aligner_pileup) in plain Python: the checker of the
product's counts.  Written from the definition in include/bgreat_gpu.h (bgr_pileup_base) on gaf_ref.py's and abundance_ref.py's conventions,
not from bgreat_amd/.

A row is (status, path ints) as the batch API returns it: path[0] = offset of the read in its walk, path[1:] = signed 1-based unitig ids; an
empty path = not mapped.  `unitigs` is the reference's vector: unitigs[0] == "" and unitigs[i] the i-th sequence of the file.

A table is a Pileup: depth[u][pos] and alt[u][pos][c], c = 0..4 for A C G T N, positions 0-based on the strand the unitig file spells, plus
`skipped`, the mapped rows whose path spells no walk (they add nothing)."""
import numpy as np

import abundance_ref as A
import gaf_ref as G
from wide_greedy_ref import ST_RC

LETTERS = "ACGTN"
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i


def codes_of(s):
    """characters -> 0..3 for A C G T, 4 (N) for anything else"""
    return _CODE[np.frombuffer(s.encode("latin-1"), dtype=np.uint8)]


def complement(codes):
    """N stays N"""
    return np.where(codes < 4, 3 - codes, 4).astype(np.uint8)


class Pileup:
    def __init__(self, unitigs):
        self.ref = [codes_of(u) for u in unitigs]
        self.depth = [np.zeros(len(u), dtype=np.int64) for u in unitigs]
        self.alt = [np.zeros((len(u), 5), dtype=np.int64) for u in unitigs]
        self.skipped = 0

    def add(self, other):
        for u in range(len(self.depth)):
            self.depth[u] += other.depth[u]
            self.alt[u] += other.alt[u]
        self.skipped += other.skipped
        return self

    def flat(self):
        """-> (n_bases, 6) int64 = (depth, a, c, g, t, n) in unitig order, as bgr_aligner_pileup delivers"""
        rows = [np.concatenate([self.depth[u][:, None], self.alt[u]], axis=1) for u in range(1, len(self.depth))]
        return np.concatenate(rows, axis=0) if rows else np.zeros((0, 6), dtype=np.int64)


def add_read(p, unitigs, k, read, status, path):
    """one mapped row; -> number of alt adds (the occurrences' mismatches, the shared k-1 characters counted on both neighbours)"""
    w = G.walk_of(unitigs, k, path)
    if w is G.NO_WALK:
        p.skipped += 1
        return 0
    walk, orient = w
    off, L = path[0], len(read)
    cl = min(L, len(walk) - off)
    q = codes_of(read)
    if status & ST_RC:   # the read on the walk's strand
        q = complement(q[::-1])
    lens = A.unitig_lens(unitigs)
    adds = 0
    for j, (s, e) in enumerate(A.extents(lens, k, path)):
        a, b = max(off, s), min(off + cl, e)
        if a >= b:
            continue
        u = abs(path[1 + j])
        x = np.arange(a - s, b - s)
        c = q[a - off:b - off]
        if orient[j]:
            pos = x
        else:
            pos, c = lens[u] - 1 - x, complement(c)
        np.add.at(p.depth[u], pos, 1)
        differs = c != p.ref[u][pos]
        np.add.at(p.alt[u], (pos[differs], c[differs]), 1)
        adds += int(differs.sum())
    return adds


def pileup_of(unitigs, k, reads, rows):
    """-> Pileup over all rows, the reads in the rows' order"""
    p = Pileup(unitigs)
    for r, (st, path) in zip(reads, rows):
        if path:
            add_read(p, unitigs, k, r, st, path)
    return p


def sites_text_of(unitigs, p):
    """the bytes bgr_write_pileup writes"""
    out = ["#unitig\tpos\tref\tdepth\tA\tC\tG\tT\tN\n"]
    for u in range(1, len(unitigs)):
        rows = np.concatenate([p.depth[u][:, None], p.alt[u]], axis=1)
        for pos in np.nonzero(rows.any(axis=1))[0]:
            out.append("%d\t%d\t%s\t%s\n" % (u, pos, unitigs[u][pos], "\t".join(str(int(v)) for v in rows[pos])))
    return "".join(out).encode()


def depth_text_of(unitigs, p):
    """the bytes bgr_write_depth writes: a line per maximal run of equal non-zero depth inside a unitig, 0-based and half-open"""
    out = []
    for u in range(1, len(unitigs)):
        d = p.depth[u]
        pos = 0
        while pos < len(d):
            e = pos + 1
            while e < len(d) and d[e] == d[pos]:
                e += 1
            if d[pos]:
                out.append("%d\t%d\t%d\t%d\n" % (u, pos, e, int(d[pos])))
            pos = e
    return "".join(out).encode()
