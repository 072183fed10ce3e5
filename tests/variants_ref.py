"""SNV sites on the unitigs (`--vcf`, bgr_variant_site, bgr_aligner_pileup_sites) in plain Python, on top of pileup_ref.py: the checker of the
product's sites and of its VCF bytes.  Written from the definition in include/bgreat_gpu.h, not from bgreat_amd/.  Integers only.

For a Pileup p and thresholds min_depth >= 1, min_alt >= 1, min_af_ppm in 0 .. 1 000 000 a base (unitig, pos) is a site when its depth >= min_depth
and at least one allele passes; allele X of A C G T, other than the unitig's own letter, passes when its count c >= min_alt and
c * 1 000 000 >= min_af_ppm * depth.  N is never an allele.  A record is (unitig, pos, depth, a, c, g, t, n); records come in (unitig, pos) order."""
import numpy as np

LETTERS = "ACGT"


def check_params(min_depth, min_alt, min_af_ppm):
    assert min_depth >= 1 and min_alt >= 1 and 0 <= min_af_ppm <= 1000000


def passing(ref, depth, counts, min_depth, min_alt, min_af_ppm):
    """counts: (a, c, g, t); ref: the unitig's code 0 .. 3 -> the passing allele codes, by count descending, ties A < C < G < T"""
    if depth < min_depth:
        return []
    ok = [x for x in range(4) if x != ref and int(counts[x]) >= min_alt and int(counts[x]) * 1000000 >= min_af_ppm * int(depth)]
    return sorted(ok, key=lambda x: (-int(counts[x]), x))


def sites_of(p, min_depth, min_alt, min_af_ppm):
    """Pileup -> [(unitig, pos, depth, a, c, g, t, n)]"""
    check_params(min_depth, min_alt, min_af_ppm)
    out = []
    for u in range(1, len(p.depth)):
        alt = p.alt[u]
        for pos in np.nonzero(alt[:, :4].any(axis=1))[0]:   # (a site has an allele with a count >= 1)
            depth = int(p.depth[u][pos])
            if passing(int(p.ref[u][pos]), depth, alt[pos][:4], min_depth, min_alt, min_af_ppm):
                out.append((u, int(pos), depth) + tuple(int(v) for v in alt[pos]))
    return out


def sites_of_rows(flat, lens, refs, min_depth, min_alt, min_af_ppm):
    """the same over a flat table as bgr_aligner_pileup delivers it: flat (n_bases, 6) = (depth, a, c, g, t, n) in unitig order, lens[u] the
    unitigs' lengths (lens[0] == 0), refs[u] their codes"""
    check_params(min_depth, min_alt, min_af_ppm)
    out, b = [], 0
    for u in range(1, len(lens)):
        rows = flat[b:b + lens[u]]
        for pos in np.nonzero(rows[:, 1:5].any(axis=1))[0]:
            depth = int(rows[pos][0])
            if passing(int(refs[u][pos]), depth, rows[pos][1:5], min_depth, min_alt, min_af_ppm):
                out.append((u, int(pos)) + tuple(int(v) for v in rows[pos]))
        b += lens[u]
    return out


def vcf_text_of(unitigs, sites, min_depth, min_alt, min_af_ppm):
    """the bytes bgr_write_vcf writes for `sites` (records as above) on the unitigs (unitigs[0] == "")"""
    check_params(min_depth, min_alt, min_af_ppm)
    out = ["##fileformat=VCFv4.2\n", "##source=bgreat-mi355x\n",
           "##bgreat_thresholds=<min_depth=%d,min_alt=%d,min_af_ppm=%d>\n" % (min_depth, min_alt, min_af_ppm),
           '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads covering the base">\n',
           '##INFO=<ID=AD,Number=R,Type=Integer,Description="Reads per allele: those that agree with the unitig, then each ALT">\n',
           '##INFO=<ID=NN,Number=1,Type=Integer,Description="Reads with a character outside ACGT at the base">\n']
    for u in sorted({s[0] for s in sites}):
        out.append("##contig=<ID=%d,length=%d>\n" % (u, len(unitigs[u])))
    out.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    for u, pos, depth, a, c, g, t, n in sorted(sites):
        ref = unitigs[u][pos]
        counts = (a, c, g, t)
        alts = passing(LETTERS.index(ref), depth, counts, min_depth, min_alt, min_af_ppm)
        assert alts, (u, pos)
        ad = [depth - (a + c + g + t + n)] + [counts[x] for x in alts]
        out.append("%d\t%d\t.\t%s\t%s\t.\tPASS\tDP=%d;AD=%s;NN=%d\n" % (u, pos + 1, ref, ",".join(LETTERS[x] for x in alts), depth, ",".join(str(v) for v in ad), n))
    return "".join(out).encode()


def table_words(p):
    """a Pileup in the device's layout (pileup_kernels.h) -> (alt uint32[4 T], delta uint32[T + n], base_offs): base b = base_offs[u] + pos owns four
    alt words A C G T, the word of the base's own letter holding the Ns; unitig u owns len + 1 delta words from base_offs[u] + u - 1 on, the
    differences of its depths (mod 2^32), the last one bringing the sum back to 0"""
    n = len(p.depth) - 1
    lens = [len(d) for d in p.depth]
    base_offs = np.zeros(n + 2, dtype=np.int64)
    base_offs[2:] = np.cumsum(lens[1:])
    T = int(base_offs[n + 1])
    alt = np.zeros(4 * T, dtype=np.uint32)
    delta = np.zeros(T + n, dtype=np.uint32)
    for u in range(1, n + 1):
        b0, d0 = int(base_offs[u]), int(base_offs[u]) + u - 1
        a = p.alt[u][:, :4].astype(np.uint32).copy()
        a[np.arange(lens[u]), p.ref[u]] = p.alt[u][:, 4].astype(np.uint32)
        alt[4 * b0:4 * (b0 + lens[u])] = a.reshape(-1)
        d = np.concatenate([[0], p.depth[u], [0]]).astype(np.int64)
        delta[d0:d0 + lens[u] + 1] = (np.diff(d) % (1 << 32)).astype(np.uint32)
    return alt, delta, base_offs
