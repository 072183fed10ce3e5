"""Triples on the GPU: bgr_aligner_triples behind ragged launches with the default table and small ones, the kernel's lane geometry and its
two-word insert on crafted rows (the method of test_gpu_crafted_rows.py), `--triples` through the CLI on every route -- against triples_ref.py (the
definition in plain Python, which test_triples_host.py makes check itself) over rows of the batch API (pinned to the oracle and to wide_greedy_ref
here), of the oracle (goldens, the synthetic files) or of the same run's GAF."""
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bgreat_amd as B
import gaf_ref as G
import oracle_py
import triples_ref as T
import wide_greedy_ref as W
from test_abundance_host import abundance_cases
from test_gaf_host import EXC_GRAPHS, golden_rows
from test_wide_k_host import strings
from tools.synth import Synth
from util import parse_counters, resolve_args, sha

pytestmark = pytest.mark.gpu

CASES = abundance_cases()
INT32_MIN = -(2 ** 31)


def _synth(k, seed=4):
    s = Synth(3000, 120, 2, k, seed)
    seqs, offs = s.unitigs()
    rb, ro = s.reads(0, 2000, 150, 2, seed + 1)
    return seqs, offs, rb, ro


def _ref_rows(k, seqs, offs, rb, ro):
    if k > 32:
        return W.GreedyRef(k, strings(seqs, offs)).align(strings(rb, ro), 2, 2)[0]
    return W.rows_of(*oracle_py.Oracle(k, seqs, offs).align(rb, ro, m=2, effort=2))


def triples_dict(arr):
    """array of B.TRIPLE_DTYPE -> triples_ref's counts; the order the library delivered them in and the canonical form are checked on the way"""
    out = T.as_tuples(arr)
    assert out == T.sorted_triples({t[:3]: t[3] for t in out}) and len({t[:3] for t in out}) == len(out)
    assert all(T.canonical(*t[:3]) == t[:3] for t in out) and not arr["reserved"].any()
    return {t[:3]: t[3] for t in out}


@pytest.mark.parametrize("capacity", [0, 256], ids=["default", "256"])
@pytest.mark.parametrize("k", [15, 31, 33])
def test_aligner_triples(k, capacity):
    """the aligner's table, filled by ragged launches: triples_ref over the rows, which are the oracle's (wide_greedy_ref's for k = 33); a table
    of another size holds the triples in another slot order"""
    seqs, offs, rb, ro = _synth(k)
    n_unitigs = len(offs) - 1
    g = B.Graph.build(k, seqs, offs)
    with B.options(poison_device_buffers=1, **({"test.triples_capacity": capacity} if capacity else {})):
        al = B.Aligner(g, 0)
        al.triples_enable()
        info = al.triples_info()
        assert info["capacity"] == (capacity or 1024) and info["bound"] == g.triples_bound() and info["overflow"] == 0 and info["used"] == 0, info
        assert len(al.triples()) == 0   # an empty table
        rows = []
        for lo, hi in ((0, 1), (1, 700), (700, 2000)):   # ragged launches
            rows += W.rows_of(*al.align(rb[int(ro[lo]):int(ro[hi])], ro[lo:hi + 1] - ro[lo], m=2, effort=2))
        assert rows == _ref_rows(k, seqs, offs, rb, ro)
        want = T.triples_of(rows, n_unitigs)
        assert 90 <= len(want) <= g.triples_bound() and sum(want.values()) > 1500   # (99 / 100 triples on these graphs, 2 228 / 1 720 traversals: counted on the CPU)
        got = al.triples()
        assert triples_dict(got) == want
        info = al.triples_info()
        assert info["overflow"] == 0 and info["used"] == len(want), info
        # a cap that is too small: BGR_E_CAPACITY, the right n, nothing copied
        n = B.C.c_uint64(0)
        buf = np.zeros(5, dtype=B.TRIPLE_DTYPE)
        assert B.lib().bgr_aligner_triples(al.h, buf.ctypes.data, 5, B.C.byref(n)) == -4 and n.value == len(want) and not buf["count"].any()
        # disabled: launches add nothing, the table stays; reset empties it
        al.triples_enable(False)
        al.align(rb[:int(ro[100])], ro[:101], m=2, effort=2)
        assert al.triples().tobytes() == got.tobytes()
        al.reset_triples()
        assert len(al.triples()) == 0 and al.triples_info()["used"] == 0
        al.triples_enable()
        al.align(rb, ro, m=2, effort=2)   # one launch: the same counts
        assert al.triples().tobytes() == got.tobytes()
        with pytest.raises(B.BgrError, match="error -1.*exhaustive"):
            al.align(rb[:int(ro[10])], ro[:11], m=2, effort=2, mode=B.MODE_EXHAUSTIVE)


def test_aligner_refusals_and_a_table_that_fills():
    seqs, offs, rb, ro = _synth(31)
    g = B.Graph.build(31, seqs, offs)
    with B.options(poison_device_buffers=1):
        al = B.Aligner(g, 0)
        n = B.C.c_uint64(7)
        assert B.lib().bgr_aligner_triples(al.h, None, 0, B.C.byref(n)) == -1 and n.value == 0 and b"never enabled" in B.lib().bgr_last_error()
        with pytest.raises(B.BgrError, match="error -1.*never enabled"):
            al.triples_info()
        al.reset_triples()   # (nothing to reset: fine)
        with B.options(**{"test.triples_capacity": 64}):   # a hundred triples do not fit: the overflow word is set, the counts are incomplete
            small = B.Aligner(g, 0)
            small.triples_enable()
        small.align(rb, ro, m=2, effort=2)
        info = small.triples_info()
        assert info["capacity"] == 64 and info["overflow"] > 0 and info["used"] == 64, info
        n.value = 7
        assert B.lib().bgr_aligner_triples(small.h, None, 0, B.C.byref(n)) == -4 and b"was full" in B.lib().bgr_last_error()
        with pytest.raises(B.BgrError, match="error -4.*was full"):
            small.triples()
        small.reset_triples()
        assert small.triples_info()["overflow"] == 0 and len(small.triples()) == 0


# ---- crafted rows -------------------------------------------------------------------------------------------------------------------------
class Crafted:
    """An aligner whose result buffers one launch has sized; rows of the test's own are written over the launch's through
    bgr_aligner_device_results and counted with test.count_with_path_stats (test_gpu_crafted_rows.py has the method).  Every crafted row lies
    inside the arena's ALLOCATION: the rows that end beyond the arena's last int do so by two ints, inside the 256 bytes and more that every new
    device buffer is given beyond what was asked for -- the kernels that do not check the arena's bound (path stats) read allocated memory."""

    def __init__(self, capacity, n_reads=200):
        k = 31
        seqs, offs, rb, ro = _synth(k)
        self.n_unitigs = len(offs) - 1
        self.n = n_reads
        self.rb, self.ro = rb[:int(ro[n_reads])], ro[:n_reads + 1]
        g = B.Graph.build(k, seqs, offs)
        with B.options(poison_device_buffers=1, **({"test.triples_capacity": capacity} if capacity else {})):
            self.al = B.Aligner(g, 0)
            self.al.triples_enable()
            self.d_r, self.d_o = B.DeviceBuffer(0, self.rb), B.DeviceBuffer(0, self.ro)
            total = int(self.ro[-1])
            self.al.align_device(self.d_r.data_ptr(), self.d_o.data_ptr(), n_reads, total, 150, m=2, effort=2)   # (sizes the result buffers, poisoned too)
            self.al.sync()
        self.arena_ints = self.al.arena_ints()
        assert self.arena_ints >= 2 * (total + 8 * n_reads)

    def count(self, rows):
        """rows: [(path ints, where)] with where = None (packed from the arena's start), "end" (ends on the arena's last int), "beyond" (two ints
        further) or an index into `rows` (shares that row).  -> the table after one pass of the counting kernels over them"""
        assert len(rows) <= self.n
        self.al.reset_triples()
        arena = np.full(self.arena_ints + 2, 0x5A5A5A5A, dtype=np.int32)
        results = np.zeros((self.n, 2), dtype=np.uint32)
        at, where = 0, {}
        for i, (path, w) in enumerate(rows):
            if isinstance(w, int):
                continue
            x = {None: at, "end": self.arena_ints - len(path), "beyond": self.arena_ints + 2 - len(path)}[w]
            if w is None:
                at += len(path) + (i % 3)
            arena[x:x + len(path)] = path
            where[i] = x
        assert at + 64 < self.arena_ints
        for i, (path, w) in enumerate(rows):
            results[i] = (where[w] if isinstance(w, int) else where[i], len(path) | (W.ST_ALIGNED << 24))
        for i in range(len(rows), self.n):
            results[i] = (7 * i, W.ST_FAILED << 24)   # not mapped: np == 0
        d_results, d_arena, _ = self.al.device_results()
        B.device_upload(0, d_results, results)
        B.device_upload(0, d_arena, arena)
        with B.options(**{"test.count_with_path_stats": 1}):
            self.al.path_stats(self.d_r.data_ptr(), self.d_o.data_ptr(), self.n)
        assert np.array_equal(B.device_download(0, d_arena, len(arena), np.int32), arena)   # (nothing writes the rows)
        return self.al.triples()

    def close(self):
        self.d_r.free()
        self.d_o.free()


def test_crafted_rows_lane_geometry():
    """paths of every length around one and two passes of sixteen lanes, ids that are none at each of the three places of a triple, a row on the
    arena's last int, one beyond it, two reads on one row: the table is triples_ref's over the rows that lie in the arena"""
    c = Crafted(4096)   # (crafted triples are no triples of the graph: its bound does not hold for them)
    rnd = random.Random(7)
    nu = c.n_unitigs
    sid = lambda: rnd.choice((1, -1)) * rnd.randint(1, nu)
    path = lambda n: [rnd.randint(0, 40)] + [sid() for _ in range(n)]
    rows = [(path(n), None) for n in (2, 3, 4, 16, 17, 18, 32, 33, 34) for _ in range(2)]
    rows.append(([3], None))   # an offset and no unitig
    for bad in (0, nu + 1, -(nu + 1), INT32_MIN):   # at each place of a triple: first, middle and last id of a row of three, and inside longer rows at both sides of a pass
        for n, p in ((3, 1), (3, 2), (3, 3), (5, 3), (20, 15), (20, 16), (20, 17), (20, 18), (34, 32), (34, 33), (34, 34)):
            q = path(n)
            q[p] = bad
            rows.append((q, None))
    shared = len(rows)
    rows.append((path(19), None))
    rows.append((rows[shared][0], shared))   # two reads share a row: it counts twice
    at_end = path(34)
    beyond = at_end[-4:] + [sid(), sid()]   # (the two rows overlap in the arena: the second one starts on the first one's last four ints)
    rows.append((at_end, "end"))
    rows.append((beyond, "beyond"))
    assert len(rows) <= c.n
    got = triples_dict(c.count(rows))
    inside = [(W.ST_ALIGNED, p) for p, w in rows if w != "beyond"]
    want = T.triples_of(inside, nu)
    assert got == want and sum(want.values()) > 500
    only_end = T.triples_of([(W.ST_ALIGNED, at_end)], nu)
    assert all(got[t] >= n for t, n in only_end.items()) and sum(only_end.values()) == 32
    assert T.triples_of([(W.ST_ALIGNED, p) for p, _ in rows], nu) != want   # (the row beyond the arena would have shown)
    info = c.al.triples_info()
    assert info["overflow"] == 0 and info["used"] == len(want), info
    c.close()


@pytest.mark.parametrize("capacity", [16, 0], ids=["16", "default"])
def test_crafted_rows_many_threads_meet_on_one_first_word(capacity):
    """one (a, b) followed by eight different c, from 64 reads at once -- every thread finds the same k0 and one of eight k1, the case of a slot whose
    two words come from different threads; then a triple and its strand mate in equal numbers: one key, both counted"""
    c = Crafted(capacity, n_reads=128)
    a, b = 5, -9
    cs = [1, -1, 2, -2, 30, -30, c.n_unitigs, -c.n_unitigs]
    rows = [([i, a, b, cs[i % 8]], None) for i in range(64)]
    got = triples_dict(c.count(rows))
    assert got == {T.canonical(a, b, x): 8 for x in cs} and len(got) == 8
    info = c.al.triples_info()
    assert info["capacity"] == (capacity or 1024) and info["overflow"] == 0 and info["used"] == 8, info
    # longer rows through the same pair: (a, b) in the middle of sixteen-lane passes, eight ways in as well
    rows = [([0] + [cs[(i // 8) % 8], a, b, cs[i % 8]], None) for i in range(64)]
    got = triples_dict(c.count(rows))
    want = T.triples_of([(W.ST_ALIGNED, p) for p, _ in rows], c.n_unitigs)
    assert got == want and len(want) == 16 and sum(want.values()) == 128
    # a triple and its strand mate in equal numbers
    t = (7, -3, 12)
    rows = [([0] + list(t), None), ([9, -12, 3, -7], None)] * 20
    got = triples_dict(c.count(rows))
    assert got == {T.canonical(*t): 40}
    c.close()


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------
def run(args, flags=("triples",), more=(), timeout=600, check=True):
    """the CLI in a scratch directory -> dict(rc, out, err, paths -- the pairs of a split run concatenated --, na, and one entry per flag: the
    file's bytes or None)"""
    d = tempfile.mkdtemp()
    try:
        files = [x for f in flags for x in ("--" + f, os.path.join(d, "out." + f))]
        p = subprocess.run([B.CLI_PATH] + list(args) + files + list(more), cwd=d, capture_output=True, text=True, timeout=timeout)
        if check and p.returncode != 0:
            raise RuntimeError("%s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
        def cat(name):
            if os.path.exists(os.path.join(d, name + ".0")):
                return b"".join(open(os.path.join(d, "%s.%d" % (name, i)), "rb").read() for i in range(8) if os.path.exists(os.path.join(d, "%s.%d" % (name, i))))
            return open(os.path.join(d, name), "rb").read() if os.path.exists(os.path.join(d, name)) else None
        r = dict(rc=p.returncode, out=p.stdout, err=p.stderr, paths=cat("paths") or b"", na=cat("notAligned.fa") or b"")
        r.update({f: cat("out." + f) for f in flags})
        return r
    finally:
        shutil.rmtree(d)


@pytest.fixture(scope="module")
def synth_files():
    """unitigs and reads of the two-allele graph as files, what a run without any flag writes, and the oracle's rows"""
    d = tempfile.mkdtemp()
    s = Synth(3000, 120, 2, 31, 4)
    s.write_unitigs(os.path.join(d, "u.fa"))
    s.write_reads(os.path.join(d, "r.fa"), 0, 2000, 150, 2, 5)
    args = ["-r", os.path.join(d, "r.fa"), "-k", "31", "-g", os.path.join(d, "u.fa"), "-m", "2", "-e", "2"]
    seqs, offs, rb, ro = _synth(31)
    rows = _ref_rows(31, seqs, offs, rb, ro)
    yield args, G.load_unitigs(os.path.join(d, "u.fa"), 31), run(args, flags=()), rows
    shutil.rmtree(d)


LANES = ["--gpus", "2", "--set", "test.lanes_on_one_device=1"]
ROUTES = [[], ["--host-route"], ["-t", "5", "--batch", "37", "--chunk-bytes", "600"], LANES, LANES + ["--split-output"]]
ROUTE_IDS = ["plain", "host", "small", "lanes", "split"]


@pytest.mark.parametrize("extra", ROUTES + [["--set", "test.wide_keys=1"]], ids=ROUTE_IDS + ["wide"])
def test_cli_triples_on_the_synthetic_files(synth_files, extra):
    """the file = triples_ref over the oracle's rows on every route; paths, notAligned.fa and the counters are those of a run without the flag"""
    args, us, plain, rows = synth_files
    r = run(args + extra)
    want = T.triples_of(rows, len(us) - 1)
    assert len(want) >= 90 and r["triples"] == T.triples_text(want)
    assert r["paths"] == plain["paths"] and r["na"] == plain["na"] and parse_counters(r["out"]) == parse_counters(plain["out"])
    if not extra:   # stdout too: the flag adds a file and nothing else
        strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
        assert strip(r["out"]) == strip(plain["out"])


@pytest.mark.parametrize("case", CASES, ids=["%02d-%s" % (c["id"], c["group"]) for c in CASES])
def test_cli_triples_on_the_goldens(case):
    """the file = triples_ref over the oracle's rows, on the plain route and with small batches; paths, notAligned.fa and the counters stay the
    golden's; a run that ends with "bug compaction" writes no file.  With --gaf: every three neighbouring segments of every GAF line are a line
    of the file after canonicalisation, and the counts sum to the segments less two over the lines"""
    a, us, H, R, rows = golden_rows(case)
    want = T.triples_of(rows, len(us) - 1)
    for extra in ([], ["-t", "5", "--batch", "37", "--chunk-bytes", "600"]):
        r = run(resolve_args(case["args"]) + extra)
        if not case["counters"]:
            assert r["triples"] is None and "bug compaction" in r["out"] and parse_counters(r["out"]) == {}, (case["args"], extra)
            continue
        assert r["triples"] == T.triples_text(want), (case["args"], extra)
        assert parse_counters(r["out"]) == case["counters"] and len(r["paths"]) == case["paths_len"] and sha(r["paths"]) == case["paths_sha256"], (case["args"], extra)
        assert len(r["na"]) == case["notaligned_len"] and sha(r["na"]) == case["notaligned_sha256"], (case["args"], extra)
    if not case["counters"] or a["correct"] or a["graph"] in EXC_GRAPHS:
        return
    r = run(resolve_args(case["args"]) + ["--gaf"])
    assert r["triples"] == T.triples_text(want), case["args"]
    file_counts = T.parse_text(r["triples"])
    seen, n_triples = {}, 0
    for ln in r["paths"].decode("latin-1").split("\n")[:-1]:
        ids = [i if fwd else -i for fwd, i in G.parse_line(ln + "\n")["segments"]]
        n_triples += max(0, len(ids) - 2)
        for t in zip(ids, ids[1:], ids[2:]):
            t = T.canonical(*t)
            assert t in file_counts, (case["args"], ln)
            seen[t] = seen.get(t, 0) + 1
    assert seen == file_counts and sum(file_counts.values()) == n_triples, case["args"]


def test_the_goldens_hold_triples():
    """(the golden test above is not about empty files)"""
    n = 0
    for case in CASES:
        a, us, H, R, rows = golden_rows(case)
        n += len(T.triples_of(rows, len(us) - 1))
    assert n >= 3000, n


def test_cli_refuses_exhaustive_mode(synth_files, tmp_path):
    args, _, _, _ = synth_files
    r = run(args + ["-b"], check=False)
    assert r["rc"] == 2 and "--triples" in r["err"] and "-b" in r["err"] and r["triples"] is None, r["err"][-500:]
