"""The pileup per strand (`--strands`, bgr_aligner_pileup_forward, bgr_variant_strand_site) in plain Python, on top of pileup_ref.py and
variants_ref.py: the checker of the product's forward table, of its sites under the strand filter and of both writers' bytes.  Written from the
definition in include/bgreat_gpu.h, not from bgreat_amd/.  Integers only.

Occurrence j of a mapped read is a FORWARD OBSERVATION when the read as given in the input is collinear with the strand the unitig file spells: the
status has no ST_RC and the occurrence is glued on forward, or it has ST_RC and the occurrence is glued on reversed -- orient[j] != bool(status &
ST_RC).  The forward pileup F is pileup_ref's Pileup over the forward observations only; the reverse part is total - F.  Rows that spell no walk add
to neither (F.skipped stays 0).

Allele X passes the strand filter when it passes variants_ref.passing and F.X >= min_alt_strand and total.X - F.X >= min_alt_strand.  A record is
(unitig, pos, depth, a, c, g, t, n, fdepth, fa, fc, fg, ft, fn)."""
import numpy as np

import abundance_ref as A
import gaf_ref as G
import pileup_ref as P
import variants_ref as V
from wide_greedy_ref import ST_RC

LETTERS = "ACGT"


def add_read_forward(f, unitigs, k, read, status, path, combos=None):
    """one mapped row into the forward Pileup f; combos: None or a dict counting the occurrences by (read RC, occurrence forward)"""
    w = G.walk_of(unitigs, k, path)
    if w is G.NO_WALK:
        return
    walk, orient = w
    off, L = path[0], len(read)
    cl = min(L, len(walk) - off)
    rc = bool(status & ST_RC)
    q = P.codes_of(read)
    if rc:
        q = P.complement(q[::-1])
    lens = A.unitig_lens(unitigs)
    for j, (s, e) in enumerate(A.extents(lens, k, path)):
        a, b = max(off, s), min(off + cl, e)
        if a >= b:
            continue
        if combos is not None:
            combos[(rc, bool(orient[j]))] = combos.get((rc, bool(orient[j])), 0) + 1
        if bool(orient[j]) == rc:   # not a forward observation
            continue
        u = abs(path[1 + j])
        x = np.arange(a - s, b - s)
        c = q[a - off:b - off]
        if orient[j]:
            pos = x
        else:
            pos, c = lens[u] - 1 - x, P.complement(c)
        np.add.at(f.depth[u], pos, 1)
        differs = c != f.ref[u][pos]
        np.add.at(f.alt[u], (pos[differs], c[differs]), 1)


def forward_of(unitigs, k, reads, rows, combos=None):
    """-> the forward Pileup over all rows"""
    f = P.Pileup(unitigs)
    for r, (st, path) in zip(reads, rows):
        if path:
            add_read_forward(f, unitigs, k, r, st, path, combos)
    return f


def forward_bases(unitigs, k, reads, rows):
    """-> per unitig, the bases its forward occurrences cover (what F's depths on the unitig must sum to)"""
    lens = A.unitig_lens(unitigs)
    out = [0] * len(unitigs)
    for r, (st, path) in zip(reads, rows):
        if not path:
            continue
        w = G.walk_of(unitigs, k, path)
        if w is G.NO_WALK:
            continue
        walk, orient = w
        off = path[0]
        cl = min(len(r), len(walk) - off)
        for j, (s, e) in enumerate(A.extents(lens, k, path)):
            a, b = max(off, s), min(off + cl, e)
            if a < b and bool(orient[j]) != bool(st & ST_RC):
                out[abs(path[1 + j])] += b - a
    return out


def passing(ref, depth, counts, fcounts, min_depth, min_alt, min_af_ppm, min_alt_strand):
    """the passing allele codes under the strand filter, by total count descending, ties A < C < G < T"""
    assert min_alt_strand >= 0
    return [x for x in V.passing(ref, depth, counts, min_depth, min_alt, min_af_ppm)
            if int(fcounts[x]) >= min_alt_strand and int(counts[x]) - int(fcounts[x]) >= min_alt_strand]


def sites_of(p, f, min_depth, min_alt, min_af_ppm, min_alt_strand):
    """total Pileup p, forward Pileup f -> [(unitig, pos, depth, a, c, g, t, n, fdepth, fa, fc, fg, ft, fn)] in (unitig, pos) order"""
    V.check_params(min_depth, min_alt, min_af_ppm)
    out = []
    for u in range(1, len(p.depth)):
        alt = p.alt[u]
        for pos in np.nonzero(alt[:, :4].any(axis=1))[0]:
            depth = int(p.depth[u][pos])
            if passing(int(p.ref[u][pos]), depth, alt[pos][:4], f.alt[u][pos][:4], min_depth, min_alt, min_af_ppm, min_alt_strand):
                out.append((u, int(pos), depth) + tuple(int(v) for v in alt[pos]) + (int(f.depth[u][pos]),) + tuple(int(v) for v in f.alt[u][pos]))
    return out


def sites_text_of(unitigs, p, f):
    """the bytes bgr_write_pileup_strands writes: bgr_write_pileup's lines (any of the six TOTAL numbers non-zero) with the six forward numbers appended"""
    out = ["#unitig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tdepth+\tA+\tC+\tG+\tT+\tN+\n"]
    for u in range(1, len(unitigs)):
        rows = np.concatenate([p.depth[u][:, None], p.alt[u]], axis=1)
        frows = np.concatenate([f.depth[u][:, None], f.alt[u]], axis=1)
        for pos in np.nonzero(rows.any(axis=1))[0]:
            out.append("%d\t%d\t%s\t%s\n" % (u, pos, unitigs[u][pos], "\t".join(str(int(v)) for v in list(rows[pos]) + list(frows[pos]))))
    return "".join(out).encode()


def vcf_text_of(unitigs, sites, min_depth, min_alt, min_af_ppm, min_alt_strand):
    """the bytes bgr_write_vcf_strands writes for `sites` (records as above) on the unitigs (unitigs[0] == "")"""
    V.check_params(min_depth, min_alt, min_af_ppm)
    out = ["##fileformat=VCFv4.2\n", "##source=bgreat-mi355x\n",
           "##bgreat_thresholds=<min_depth=%d,min_alt=%d,min_af_ppm=%d,min_alt_strand=%d>\n" % (min_depth, min_alt, min_af_ppm, min_alt_strand),
           '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads covering the base">\n',
           '##INFO=<ID=AD,Number=R,Type=Integer,Description="Reads per allele: those that agree with the unitig, then each ALT">\n',
           '##INFO=<ID=ADF,Number=R,Type=Integer,Description="Reads per allele that run along the unitig\'s strand as given">\n',
           '##INFO=<ID=ADR,Number=R,Type=Integer,Description="Reads per allele that run along the unitig\'s other strand as given">\n',
           '##INFO=<ID=NN,Number=1,Type=Integer,Description="Reads with a character outside ACGT at the base">\n']
    for u in sorted({s[0] for s in sites}):
        out.append("##contig=<ID=%d,length=%d>\n" % (u, len(unitigs[u])))
    out.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    for u, pos, depth, a, c, g, t, n, fdepth, fa, fc, fg, ft, fn in sorted(sites):
        ref = unitigs[u][pos]
        counts, fcounts = (a, c, g, t), (fa, fc, fg, ft)
        alts = passing(LETTERS.index(ref), depth, counts, fcounts, min_depth, min_alt, min_af_ppm, min_alt_strand)
        assert alts, (u, pos)
        ad = [depth - (a + c + g + t + n)] + [counts[x] for x in alts]
        adf = [fdepth - (fa + fc + fg + ft + fn)] + [fcounts[x] for x in alts]
        adr = [x - y for x, y in zip(ad, adf)]
        assert all(v >= 0 for v in adf + adr), (u, pos)
        join = lambda v: ",".join(str(x) for x in v)
        out.append("%d\t%d\t.\t%s\t%s\t.\tPASS\tDP=%d;AD=%s;ADF=%s;ADR=%s;NN=%d\n" % (u, pos + 1, ref, ",".join(LETTERS[x] for x in alts), depth, join(ad), join(adf), join(adr), n))
    return "".join(out).encode()
