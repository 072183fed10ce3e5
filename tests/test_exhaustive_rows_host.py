"""The view of exhaustive rows (exhaustive_rows_ref; bgr_aligner_exhaustive_paths_enable in include/bgreat_gpu.h) on the oracle's rows of the -b
goldens, on the CPU: every mapped row of a run without -i is a greedy row plus its end offset, the view of it spells a walk that covers the whole
read, and the dropped int follows from what is kept.  The -i goldens hold rows the rule turns into empty rows: why -i is refused."""
import functools
import os

import pytest

import exhaustive_rows_ref as X
import gaf_ref as G
import oracle_py
import wide_greedy_ref as W
from util import GOLD, golden_cases

EXH = [c for c in golden_cases() if "-b" in c["args"]]
WHOLE = [c for c in EXH if "-i" not in c["args"]]
PARTIAL = [c for c in EXH if "-i" in c["args"]]


def _arg(args, flag, default):
    return args[args.index(flag) + 1] if flag in args else default


@functools.lru_cache(maxsize=None)
def oracle_rows(case_id):
    """-> (k, m, unitigs, reads as str, rows) of a -b golden, the rows the oracle's exhaustive mode gives"""
    case = next(c for c in EXH if c["id"] == case_id)
    args = case["args"]
    k, m = int(_arg(args, "-k", "30")), int(_arg(args, "-m", "2"))
    ufile = os.path.join(GOLD, _arg(args, "-g", None))
    o = oracle_py.Oracle(k, fasta=ufile)
    reads, roffs, _, _ = oracle_py.parse_file(os.path.join(GOLD, _arg(args, "-r", None)), k)
    rows = W.rows_of(*o.align(reads, roffs, m=m, effort=int(_arg(args, "-e", "2")), mode=1, partial="-i" in args))
    strs = [bytes(reads[int(roffs[i]):int(roffs[i + 1])]).decode() for i in range(len(roffs) - 1)]
    assert sum(1 for st, p in rows if p) == case["counters"]["aligned"]
    return k, m, G.load_unitigs(ufile, k), strs, rows


def test_the_goldens_are_the_ones_the_definition_was_checked_on():
    assert len(WHOLE) == 9 and sum(c["counters"]["aligned"] for c in WHOLE) == 1770 and len(PARTIAL) >= 3


@pytest.mark.parametrize("case", WHOLE, ids=lambda c: "%02d-%s" % (c["id"], c["group"]))
def test_every_exhaustive_row_is_a_greedy_row_and_its_end_offset(case):
    k, m, us, reads, rows = oracle_rows(case["id"])
    n_mapped = n_over = 0
    for read, (st, path) in zip(reads, rows):
        vst, vpath = X.view_row(st, path)
        assert vst == st
        if not path:
            assert vpath == []
            continue
        n_mapped += 1
        assert st == W.ST_ALIGNED and len(path) >= 3 and vpath == path[:-1]   # no reverse-complement retry in exhaustive mode
        # the view on result words: the same row, one int shorter, the status kept; a row that ends beyond the arena is an empty one
        w = len(path) | (st << 24)
        assert X.view_word(7, w, 7 + len(path)) == (7, (len(path) - 1) | (st << 24))
        assert X.view_word(7, w, 6 + len(path)) == (7, st << 24)
        s = G.stats(us, k, read, vst, vpath)
        assert s is not G.NO_WALK and s["cl"] == len(read) and s["qstart"] == 0 and s["qend"] == len(read)   # a walk, and the whole read lies on it
        assert path[-1] in X.end_offsets(us, k, len(read), vpath)
        if "N" not in read:
            assert s["nm"] <= m
        n_over += s["nm"] > m
    assert n_mapped == case["counters"]["aligned"]
    assert n_over == 0 or k == 5   # (the rolling count of SURVEY Appendix C: reads with an N on the k = 5 goldens)


def test_reads_with_an_n_may_exceed_the_budget_under_the_gaf_definition():
    over = 0
    for case in WHOLE:
        k, m, us, reads, rows = oracle_rows(case["id"])
        over += sum(1 for read, (st, path) in zip(reads, rows) if path and G.stats(us, k, read, *X.view_row(st, path))["nm"] > m)
    assert over == 32


def test_partial_paths_hold_rows_without_an_end_offset():
    """-i: rows of one and two ints (alignerExhaustive.cpp:217-221) -- mapped reads the view turns into empty rows"""
    short = 0
    for case in PARTIAL:
        _, _, _, _, rows = oracle_rows(case["id"])
        for st, path in rows:
            if path and len(path) < 3:
                short += 1
                assert X.view_row(st, path) == (st, [])
    assert short > 0
