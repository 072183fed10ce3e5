"""The checker of the GAF output (gaf_ref.py) pinned to the reference without the product: over the oracle's rows for the goldens, what a line
says must be what the reference's -c wrote (bytes of tests/golden/expected.json) and what a reader of the line reconstructs from the unitig file.
Plus the C-ABI's new surface as far as a machine without a device gets."""
import ctypes as C
import functools
import os

import pytest

import bgreat_amd as B
import gaf_ref as G
import oracle_py
from util import GOLD, golden_cases, sha

EXC_GRAPHS = ("deg_unitig_exc.fa",)   # non-ACGT unitig characters: GAF output is refused there


def case_args(case):
    """-> dict(files, k, graph, m, e, fastq, anchors, brute, correct) of a golden's command line (bgreat.cpp:56-66 defaults)."""
    a = case["args"]
    val = lambda flag, d: a[a.index(flag) + 1] if flag in a else d
    return {"files": val("-r", "").split(","), "k": int(val("-k", 30)), "graph": val("-g", "unitig.fa"), "m": int(val("-m", 2)), "e": int(val("-e", 2)),
            "fastq": "-q" in a, "anchors": "-G" in a, "brute": "-b" in a, "correct": "-c" in a}


def gaf_cases():
    """the goldens a --gaf run is defined for: no -b, no -c, ACGT-only graph"""
    return [c for c in golden_cases() if not case_args(c)["brute"] and not case_args(c)["correct"] and case_args(c)["graph"] not in EXC_GRAPHS]


@functools.lru_cache(maxsize=None)
def _oracle(graph, k, anchors):
    return oracle_py.Oracle(k, fasta=os.path.join(GOLD, graph), anchors=anchors)


@functools.lru_cache(maxsize=None)
def _unitigs(graph, k):
    return G.load_unitigs(os.path.join(GOLD, graph), k)


@functools.lru_cache(maxsize=None)
def _parsed(path, k, fastq):
    reads, roffs, heads, hoffs = oracle_py.parse_file(os.path.join(GOLD, path), k, fastq)
    n = len(roffs) - 1
    R = [bytes(reads[int(roffs[i]):int(roffs[i + 1])]).decode("latin-1") for i in range(n)]
    H = [bytes(heads[int(hoffs[i]):int(hoffs[i + 1])]).decode("latin-1") for i in range(n)]
    return reads, roffs, R, H


def golden_rows(case):
    """-> (args dict, unitigs, headers, reads, rows) with rows = [(status, path ints)] from the oracle, the files of the list one after the other"""
    a = case_args(case)
    o = _oracle(a["graph"], a["k"], a["anchors"])
    H, R, rows = [], [], []
    for f in a["files"]:
        reads, roffs, r, h = _parsed(f, a["k"], a["fastq"])
        p, po, st = o.align(reads, roffs, m=a["m"], effort=a["e"], mode=2 if a["anchors"] else 0)
        rows += [(int(st[i]), [int(x) for x in p[int(po[i]):int(po[i + 1])]]) for i in range(len(r))]
        H += h
        R += r
    return a, _unitigs(a["graph"], a["k"]), H, R, rows


def test_q_is_what_the_reference_wrote_with_c():
    """header + Q over the mapped reads = the paths file of the reference's -c run, byte for byte: ties Q, and with it the rule for reads mapped
    on their reverse complement, to bytes the reference wrote."""
    n = 0
    for case in golden_cases():
        a = case_args(case)
        if not a["correct"] or a["brute"] or a["graph"] in EXC_GRAPHS:
            continue
        a, us, H, R, rows = golden_rows(case)
        out = []
        for i, (st, path) in enumerate(rows):
            if path:
                s = G.stats(us, a["k"], R[i], st, path)
                assert s is not G.NO_WALK, (case["args"], i)
                out.append(H[i] + "\n" + s["Q"] + "\n")
        got = "".join(out).encode("latin-1")
        assert len(got) == case["paths_len"] and sha(got) == case["paths_sha256"], case["args"]
        n += 1
    assert n == 9


def check_lines(us, k, m, H, R, rows, text):
    """every line of `text` (the GAF stream of rows) read back from the unitigs -> number of lines"""
    lines = text.split("\n")[:-1]
    mapped = [i for i, (_, p) in enumerate(rows) if p]
    assert len(lines) == len(mapped)
    for ln, i in zip(lines, mapped):
        st, path = rows[i]
        s = G.stats(us, k, R[i], st, path)
        f = G.parse_line(ln + "\n")
        assert f["name"] == G.name_of(H[i]) and f["qlen"] == len(R[i])
        walk = G.spell(us, k, f["segments"])
        assert walk is not None and len(walk) == f["plen"], ln
        assert 0 <= f["pstart"] <= f["pend"] <= f["plen"] and 0 <= f["qstart"] <= f["qend"] <= f["qlen"] and f["pend"] - f["pstart"] == f["qend"] - f["qstart"] == f["block"], ln
        q = walk[f["pstart"]:f["pend"]]
        assert q == s["Q"], ln
        piece = R[i][f["qstart"]:f["qend"]]
        assert f["nm"] == sum(1 for x, y in zip(q, piece) if x != y) and f["matches"] == f["block"] - f["nm"], ln
        if set(R[i]) <= set("ACGT"):   # (an N inside the anchor is never compared by the mapper: such reads do exceed the budget)
            assert f["nm"] <= m, (ln, m)
    return len(lines)


def test_every_line_reads_back_from_the_unitig_file():
    n_cases = n_lines = 0
    for case in gaf_cases():
        a, us, H, R, rows = golden_rows(case)
        text, bug = G.gaf_of(us, a["k"], H, R, rows)
        assert bug is None, case["args"]
        assert text.count("\n") == case["counters"]["aligned"], case["args"]
        n_lines += check_lines(us, a["k"], a["m"], H, R, rows, text)
        n_cases += 1
    assert n_cases >= 60 and n_lines >= 7000, (n_cases, n_lines)


def test_issue_examples():
    case = next(c for c in golden_cases() if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    a, us, H, R, rows = golden_rows(case)
    text, _ = G.gaf_of(us, 31, H, R, rows)
    lines = text.split("\n")
    assert rows[0][1] == [8, 363, 364, -366, 367] and lines[0] == "r0\t150\t0\t150\t+\t>363>364<366>367\t162\t8\t158\t150\t150\t255\tNM:i:0"
    assert rows[2][1] == [32, -1009, -1008, -1006, 1005] and rows[2][0] & 4
    assert lines[2] == "r2\t150\t0\t150\t+\t<1005>1006>1008>1009\t208\t26\t176\t148\t150\t255\tNM:i:2"
    assert G.name_of(">") == "*" and G.name_of("@a b") == "a" and G.name_of(">x\ty z") == "x" and G.name_of("") == "*"


def test_cabi_surface(tmp_path):
    L = B.lib()
    assert hasattr(L, "bgr_aligner_path_stats")
    assert C.sizeof(B.PathStat) == 24 and C.sizeof(B.RunOptions) == 80
    g = B.Graph.from_fasta(os.path.join(GOLD, "toy_unitig.fa"), 4)
    p = B.Params(0, 2, 2, 0)
    cnt = (C.c_uint64 * 5)()
    secs = C.c_double(0)
    call = lambda o: L.bgr_align_all(g.h, C.byref(p), C.byref(o), os.path.join(GOLD, "toy_reads.fa").encode(), str(tmp_path / "p").encode(), str(tmp_path / "n").encode(), cnt,
                                     C.byref(secs))
    old = B.RunOptions(72, 1, 1)   # the struct before it gained `gaf`
    assert call(old) == -1 and b"struct_size" in L.bgr_last_error()
    new = B.RunOptions(C.sizeof(B.RunOptions), 1, 1)
    assert new.gaf == 0
    rc = call(new)
    assert rc == 0 or b"struct_size" not in L.bgr_last_error()   # (without a device: BGR_E_HIP from the aligner, not a refusal of the struct)
    # the refusals come before any device work
    new.gaf = 1
    new.correction = 1
    assert call(new) == -1 and b"-c" in L.bgr_last_error()
    new.correction = 0
    pb = B.Params(B.MODE_EXHAUSTIVE, 2, 2, 0)
    assert L.bgr_align_all(g.h, C.byref(pb), C.byref(new), b"x.fa", b"p", b"n", cnt, C.byref(secs)) == -1 and b"-b" in L.bgr_last_error()
    ge = B.Graph.from_fasta(os.path.join(GOLD, "deg_unitig_exc.fa"), 5)
    assert L.bgr_align_all(ge.h, C.byref(p), C.byref(new), b"x.fa", b"p", b"n", cnt, C.byref(secs)) == -1 and b"ACGT" in L.bgr_last_error()
