"""The definition of --recompact (bgr_graph_recompact in include/bgreat_gpu.h restates it) over Python strings.

K = k - 1.  An oriented id x is +u or -u (1 <= u <= n); spell(x) is unitig u or its reverse complement; first(x) / last(x) are the first / last K
characters of spell(x); nodes are ordered by (|x|, x < 0).  x -> y is an edge when both are kept and last(x) == first(y); out(x) counts the edges
that leave x, in(x) = out(-x).  x -> y is a merge link when out(x) == 1, in(y) == 1 and |x| != |y|.  The components of the merge links are paths and
rings; a component and its mate are two readings of one chain, reported once, in the reading whose first node is smaller (a ring's first node is its
smallest).  The first unitig goes in whole, every later one without its first K characters.  Chains are ordered by first node and numbered from 1.

Everything here is keyed by the (k-1)-mer strings, never by the graph blob's meta.  compact() asserts the properties the definition promises."""
from collections import Counter, defaultdict

_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


def order_key(x):
    return 2 * (abs(x) - 1) + (1 if x < 0 else 0)


def spell(unitigs, x):
    return unitigs[x - 1] if x > 0 else rc(unitigs[-x - 1])


def canonical_kmers(seqs, k):
    c = Counter()
    for s in seqs:
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            r = rc(w)
            c[w if w <= r else r] += 1
    return c


def merge_links(unitigs, keep, k):
    """-> (succ: dict node -> node over the merge links, out: dict node -> number of edges leaving it, stats of what was met)"""
    K = k - 1
    nodes = [x for u in range(1, len(unitigs) + 1) if keep[u - 1] for x in (u, -u)]
    begins = defaultdict(list)
    for x in nodes:
        begins[spell(unitigs, x)[:K]].append(x)
    out = {x: len(begins.get(spell(unitigs, x)[-K:], ())) for x in nodes}
    succ = {}
    stats = {"hairpin": 0, "self_loop": 0, "palindrome": 0}
    for x in nodes:
        e = spell(unitigs, x)[-K:]
        ys = begins.get(e, ())
        if ys and e == rc(e):
            stats["palindrome"] += 1
        for y in ys:
            if y == x:
                stats["self_loop"] += 1
            if y == -x:
                stats["hairpin"] += 1
        if out[x] == 1:
            y = ys[0]
            if out[-y] == 1 and abs(x) != abs(y):
                succ[x] = y
    for x, y in succ.items():   # closed under mating, one predecessor each
        assert succ.get(-y) == -x
    assert len(set(succ.values())) == len(succ)
    return nodes, succ, stats


def chains_of(unitigs, keep, k):
    """-> (list of (walk, circular) in the reported order, stats)"""
    nodes, succ, stats = merge_links(unitigs, keep, k)
    pred = {y: x for x, y in succ.items()}
    seen = set()
    comps = []   # (walk, circular), every component, both readings
    for x in nodes:
        if x in pred or x in seen:
            continue
        w = [x]
        while w[-1] in succ:
            w.append(succ[w[-1]])
        seen.update(w)
        comps.append((w, False))
    for x in sorted(nodes, key=order_key):   # what is left lies on rings; the smallest node of each is met first
        if x in seen:
            continue
        w = [x]
        while succ[w[-1]] != x:
            w.append(succ[w[-1]])
        assert min(w, key=order_key) == x
        seen.update(w)
        comps.append((w, True))
    stats["ring"] = sum(1 for _, c in comps if c) // 2
    chains = []
    for w, circ in comps:
        assert not (set(w) & {-z for z in w}), "a component holds z and -z"
        mate_first = -w[-1] if not circ else min((-z for z in w), key=order_key)
        assert order_key(w[0]) != order_key(mate_first)
        if order_key(w[0]) < order_key(mate_first):
            chains.append((w, circ))
    chains.sort(key=lambda c: order_key(c[0][0]))
    return chains, stats


def spell_walk(unitigs, walk, k):
    K = k - 1
    s = spell(unitigs, walk[0])
    for x in walk[1:]:
        t = spell(unitigs, x)
        assert s[-K:] == t[:K]
        s += t[K:]
    return s


def compact(unitigs, keep, k, check=True, stats_out=None):
    """-> list of (walk: list of oriented ids, circular: bool, sequence: str) in the reported order"""
    assert all(len(u) >= k for u in unitigs)
    chains, stats = chains_of(unitigs, keep, k)
    res = [(w, c, spell_walk(unitigs, w, k)) for w, c in chains]
    if stats_out is not None:
        stats_out.update(stats)
    K = k - 1
    for w, c, s in res:
        assert len(s) == sum(len(unitigs[abs(x) - 1]) for x in w) - (len(w) - 1) * K
        if c:
            assert s[:K] == s[-K:]
    if check:
        members = sorted(abs(x) for w, _, _ in res for x in w)
        assert members == [u for u in range(1, len(unitigs) + 1) if keep[u - 1]], "every kept unitig lies in exactly one chain"
        assert canonical_kmers((s for _, _, s in res), k) == canonical_kmers((unitigs[u - 1] for u in members), k), "k-mers lost or invented"
        again, _ = chains_of([s for _, _, s in res], [1] * len(res), k)
        assert all(len(w) == 1 for w, _ in again), "the output compacts further"
    return res


def records(res):
    """the result as the device delivers it -> (list of (seq_off, seq_len, walk_off, n_unitigs, flags), walk ints, sequence bytes)"""
    recs, walk, seq = [], [], []
    so = 0
    for w, c, s in res:
        recs.append((so, len(s), len(walk), len(w), 1 if c else 0))
        walk.extend(w)
        seq.append(s)
        so += len(s)
    return recs, walk, "".join(seq).encode()


def fasta_bytes(res):
    """the writer's bytes"""
    out = []
    for i, (w, c, s) in enumerate(res):
        walk = "".join((">" if x > 0 else "<") + str(abs(x)) for x in w)
        out.append(">%d LN:i:%d unitigs=%d ring=%s walk=%s\n%s\n" % (i + 1, len(s), len(w), "circular" if c else ".", walk, s))
    return "".join(out).encode()
