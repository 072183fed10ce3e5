"""The definition of the cs:Z: field (gaf_cs_ref.py) without the product: hand cases, and its three invariants over the oracle's rows for every
golden a --gaf run is defined for.  Plus the C-ABI's new surface as far as a machine without a device gets: the symbols, the struct, the graph's
switch and the refusal of a run that has the switch on and no GAF output."""
import ctypes as C
import os

import pytest

import bgreat_amd as B
import gaf_cs_ref as CS
import gaf_ref as G
from test_gaf_host import gaf_cases, golden_rows
from util import GOLD


def test_hand_cases():
    P = "ACGT" * 38
    P = P[:150]
    assert CS.ops_of(P, P) == ":150"
    assert CS.ops_of("C" + P[1:], "A" + P[1:]) == "*ca:149"
    assert CS.ops_of("ACGTA", "AATTA") == ":1*ca*gt:2"           # two neighbours: nothing between them
    assert CS.ops_of("AAAA", "AANA") == ":2*an:1"
    assert CS.ops_of("AAAA", "AAaA") == ":2*an:1"                # lower case is outside ACGT
    assert CS.ops_of("", "") == ""
    assert CS.ops_of("ACG", "TGC") == "*at*cg*gc"
    assert CS.ops_of("AC", "AT") == ":1*ct" and CS.ops_of("CA", "TA") == "*ct:1"
    for n in (9, 10, 99, 100):
        run = "G" * n
        assert CS.ops_of("A" + run + "C", "T" + run + "A") == "*at:%d*ca" % n
        assert CS.ops_of(run, run) == ":%d" % n
        assert len(CS.ops_of(run + "A", run + "C")) == 1 + len(str(n)) + 3
    assert CS.with_cs("r\tNM:i:0\n", ":5") == "r\tNM:i:0\tcs:Z::5\n"
    assert CS.with_cs("r\tNM:i:0\tPS:i:1\tHP:i:1\tha:i:1\thb:i:0\tho:i:0\n", "") == "r\tNM:i:0\tPS:i:1\tHP:i:1\tha:i:1\thb:i:0\tho:i:0\tcs:Z:\n"
    assert CS.parse_ops(":3*ca*gt:12") == [("=", 3), ("*", "c", "a"), ("*", "g", "t"), ("=", 12)]
    assert CS.apply_ops(":1*ca*gn:2", "ACGTT") == "AAnTT"
    assert CS.diffs_of("ACGT", "AGNT") == [(1, 1, 2), (2, 2, 4)]
    for bad in (":0", ":3:4", "*aa", "*xa", ":", "*a"):
        with pytest.raises((AssertionError, IndexError)):
            CS.parse_ops(bad)


def test_a_read_on_its_reverse_complement_is_described_in_its_own_direction():
    """the issue's two golden lines (test_gaf_host.test_issue_examples): r0 forward without a difference, r2 on the reverse complement with two"""
    case = next(c for c in gaf_cases() if c["args"] == ["-r", "syn_r150.fa", "-k", "31", "-g", "syn_unitig.fa", "-m", "2", "-e", "2"])
    a, us, H, R, rows = golden_rows(case)
    s0, s2 = G.stats(us, 31, R[0], *rows[0]), G.stats(us, 31, R[2], *rows[2])
    assert CS.cs_of(R[0], s0) == ":150"
    ops = CS.cs_of(R[2], s2)
    assert rows[2][0] & 4 and ops.count("*") == 2
    walk = G.spell(us, 31, s2["segments"])   # the line's segments already are the reversed path
    assert CS.apply_ops(ops, walk[s2["pstart"]:s2["pend"]]) == R[2]
    text, bug = CS.gaf_cs_of(us, 31, H, R, rows)
    assert bug is None and text.split("\n")[0] == G.line_of(H[0], R[0], s0)[:-1] + "\tcs:Z::150"


def test_invariants_over_the_goldens():
    n_cases = n_lines = 0
    by_nm = {0: 0, 1: 0, 2: 0}
    with_n = empty = 0
    for case in gaf_cases():
        a, us, H, R, rows = golden_rows(case)
        for i, (st, path) in enumerate(rows):
            if not path:
                continue
            s = G.stats(us, a["k"], R[i], st, path)
            assert s is not G.NO_WALK
            ops = CS.cs_of(R[i], s)
            CS.check_invariants(us, a["k"], R[i], s, ops)
            assert [(q - s["qstart"], "acgt"[p], "acgtn"[r]) for q, p, r in CS.path_diff_rows(us, a["k"], R[i], st, path)] == \
                [(j, x[1], x[2]) for j, x in positions(CS.parse_ops(ops))]
            by_nm[min(s["nm"], 2)] += 1
            with_n += "n" in ops
            empty += ops == ""
            n_lines += 1
        n_cases += 1
    assert n_cases >= 60 and n_lines >= 7000, (n_cases, n_lines)
    assert by_nm[0] > 1000 and by_nm[1] > 100 and by_nm[2] > 100 and with_n > 0, (by_nm, with_n)   # lines with 0, with 1 and with at least 2 differences


def positions(parsed):
    """-> [(position in the aligned part, op)] of the "*" ops"""
    out, at = [], 0
    for op in parsed:
        if op[0] == "=":
            at += op[1]
        else:
            out.append((at, op))
            at += 1
    return out


def test_symbols_and_struct():
    assert B.PATH_DIFF_DTYPE.itemsize == 8 and B.PATH_DIFF_DTYPE.fields["path_base"][1] == 4 and B.PATH_DIFF_DTYPE.fields["read_base"][1] == 5
    for name in ("bgr_aligner_path_diffs", "bgr_aligner_gaf_cs_enable", "bgr_graph_gaf_cs_enable", "bgr_graph_gaf_cs_enabled"):
        assert name in B.SYMBOLS and hasattr(B.lib(), name)
    assert C.sizeof(B.PathStat) == 24 and C.sizeof(B.RunOptions) == 80   # no existing struct changed


def test_refusals_without_a_device(tmp_path):
    L = B.lib()
    assert L.bgr_graph_gaf_cs_enable(None, 1) == -1 and b"null graph" in L.bgr_last_error()
    assert L.bgr_aligner_gaf_cs_enable(None, 1) == -1 and b"null aligner" in L.bgr_last_error()
    assert L.bgr_graph_gaf_cs_enabled(None) == 0
    n = C.c_uint64(7)
    offs = (C.c_uint64 * 2)()
    assert L.bgr_aligner_path_diffs(None, None, None, 0, offs, None, 0, C.byref(n)) == -1 and b"null argument" in L.bgr_last_error() and n.value == 0
    g = B.Graph.from_fasta(os.path.join(GOLD, "toy_unitig.fa"), 4)
    assert not g.gaf_cs_enabled()
    g.gaf_cs_enable()
    assert g.gaf_cs_enabled()
    p = B.Params(0, 2, 2, 0)
    cnt = (C.c_uint64 * 5)()
    secs = C.c_double(0)
    opt = B.RunOptions(C.sizeof(B.RunOptions), 1, 1)
    call = lambda: L.bgr_align_all(g.h, C.byref(p), C.byref(opt), os.path.join(GOLD, "toy_reads.fa").encode(), str(tmp_path / "p").encode(), str(tmp_path / "n").encode(), cnt,
                                   C.byref(secs))
    assert opt.gaf == 0
    assert call() == -1 and b"cs:Z:" in L.bgr_last_error() and b"--gaf" in L.bgr_last_error()   # the switch on, no GAF output: before any device work
    assert not (tmp_path / "p").exists()
    opt.gaf = 1
    opt.correction = 1
    assert call() == -1 and b"-c" in L.bgr_last_error()   # --gaf's own refusals stand
    g.gaf_cs_enable(False)
    opt.gaf = opt.correction = 0
    assert not g.gaf_cs_enabled()
    rc = call()
    assert rc == 0 or b"cs:Z:" not in L.bgr_last_error()   # (without a device: BGR_E_HIP from the aligner, not this refusal)
