"""Haplotags on the GPU: bgr_aligner_haplotags on rows the test writes into the result buffers and on rows of the mapper, the tagged instances of
the GAF kernels through bgr_align_fasta_text and through whole runs on every route, two planted haplotypes end to end through the CLI, and the
refusals -- everything exactly what haplotag_ref.py (the definition in plain Python) says, the lines themselves gaf_ref.py's."""
import os
import random
import subprocess

import numpy as np
import pytest

import bgreat_amd as B
import blocks_ref as BR
import gaf_ref as G
import haplotag_ref as H
import wide_greedy_ref as W
from test_gpu_crafted_rows import crafted
from test_gpu_haplotypes import planted, rc
from test_gpu_triples import ROUTE_IDS, ROUTES, run
from test_wide_k_host import pack, strings
from tools.synth import Synth

pytestmark = pytest.mark.gpu

INT32_MIN = -(2 ** 31)
ALIGNED, RC = W.ST_ALIGNED, W.ST_ALIGNED | W.ST_RC


# ---- crafted rows -----------------------------------------------------------------------------------------------------------------------------
N_UNITIGS = 61   # test_gpu_crafted_rows' graph
LOW = N_UNITIGS   # the unitig of block 1, the smallest block: the table's last entry


def crafted_table():
    """blocks 3 (unitigs 1 .. 10), 5 (11 .. 20), 2 (21 .. 24) and 7 (51 .. 60) with the haplotypes alternating, nothing for 25 .. 50, and block 1's
    haplotype B on the last unitig"""
    t = [0] * (N_UNITIGS + 1)
    for lo, hi, block in ((1, 10, 3), (11, 20, 5), (21, 24, 2), (51, 60, 7)):
        for u in range(lo, hi + 1):
            t[u] = block << 1 | (u & 1)
    t[LOW] = 1 << 1 | 1
    return t


def crafted_rows(seed):
    """-> [(name, path or [] for an unmapped read)], the path with an offset in front"""
    rng = random.Random(seed)
    some = lambda n, pool: [rng.choice(pool) * rng.choice((1, -1)) for _ in range(n)]
    anything, quiet, five = list(range(1, N_UNITIGS)), list(range(25, 51)), list(range(11, 21))
    rows = []
    for n in (1, 2, 15, 16, 17, 32, 33, 40):
        rows.append(("random %d" % n, some(n, anything)))
        rows.append(("no vote %d" % n, some(n, quiet)))
    for n, at in ((1, 0), (16, 0), (17, 0), (16, 15), (17, 15), (40, 15), (17, 16), (33, 20), (33, 32), (40, 39)):   # block 1's only vote: lane 0, lane 15, a later pass only
        ids = some(n, anything)
        ids[at] = -LOW if at & 1 else LOW
        rows.append(("low at %d of %d" % (at, n), ids))
    ids = some(16, five) + some(19, quiet) + [22] + some(4, quiet)   # a larger block in the first pass, the smaller one in the third
    rows.append(("smaller block in the third pass", ids))
    rows.append(("a == b", [1, -2, 30, 4, 3]))
    rows.append(("a == b over two passes", some(15, quiet) + [1] + some(3, quiet) + [2]))
    rows.append(("others", [11, 12, 21, 55, -56, 57]))
    rows.append(("all negative", [-x for x in (21, 22, 23, 24, 1, 11, 51)]))
    rows.append(("ids outside", [0, N_UNITIGS + 1, -(N_UNITIGS + 1), INT32_MIN, 2 ** 31 - 1, 5, 0]))
    rows.append(("only ids outside", [0, N_UNITIGS + 1, INT32_MIN]))
    rows.append(("ids outside in the second pass", some(16, quiet) + [INT32_MIN, 0, N_UNITIGS + 1, -7]))
    rows.append(("last entry alone", [LOW]))
    rows.append(("an offset and no unitig", []))   # (np == 1 below: see layout)
    out = [(name, [rng.randrange(0, 50)] + ids) for name, ids in rows]
    out[-1] = ("an offset and no unitig", [7])
    return out


SPECIAL = [5, 11, 12, 21, 55, -56, 57]   # the row at the arena's end, and the one that reaches past it


def layout(rows, n, arena_ints, seed):
    """n reads over `rows` (cycled from a random start), with unmapped reads between mapped ones, two reads on one row, one row ending on the
    arena's last int and one reaching one int past it -> (results, arena, [the path the definition sees per read])"""
    rng = random.Random(seed)
    arena = np.full(arena_ints, 0x5A5A5A5A, dtype=np.int32)
    results = np.zeros((n, 2), dtype=np.uint32)
    seen, at, start = [], 0, rng.randrange(len(rows))
    placed = {}
    for i in range(n):
        if n >= 5 and i % 4 == 1:   # unmapped reads between mapped ones, in the same wave
            results[i] = (rng.randrange(arena_ints), (W.ST_NOANCHOR, W.ST_FAILED)[i % 2] << 24)
            seen.append([])
            continue
        j = (start + i) % len(rows)
        path = rows[j][1]
        status = (ALIGNED, RC)[i % 2] | (0x50 if i % 7 == 0 else 0)
        if n >= 5 and i == n - 1:   # the last read shares the row of the first
            results[i] = (results[0][0], len(seen[0]) | (status << 24))
            seen.append(seen[0])
            continue
        if n >= 3 and i == 2:   # ends on the arena's last int
            path = SPECIAL
            x = arena_ints - len(path)
        elif n >= 4 and i == 3:   # one int past it: zeros, and nothing of it is read
            path = SPECIAL
            x = arena_ints - len(path) + 1
        else:
            x = at
            at += len(path) + rng.randrange(3)
        if not (n >= 4 and i == 3):
            arena[x:x + len(path)] = path
        else:
            arena[x:] = path[:-1]
        placed[i] = x
        results[i] = (x, len(path) | (status << 24))
        seen.append([] if n >= 4 and i == 3 else path)
    assert at + 48 < arena_ints
    return results, arena, seen


@pytest.mark.parametrize("k", [15, 64])
def test_crafted_rows(k):
    """the stand-alone kernel over rows the mapper never writes, at 1, 3, 4, 5, 63, 64 and 65 reads per launch (a group alone, a last wave with one
    group, one more than a wave's four) and over the whole set; then with an all-zero table, and with the table off"""
    c = crafted(k)
    g = B.Graph.build(k, *pack(c["us"][1:]))
    assert g.info()["n_unitigs"] == N_UNITIGS
    al = B.Aligner(g, 0)
    table = crafted_table()
    rows = crafted_rows(k)
    want_all = [H.tag_of(table, p) for _, p in rows]
    assert (2, 1, 0, 16) in want_all and any(t[1] == t[2] > 0 for t in want_all) and any(t[3] for t in want_all) and sum(t[:3] == (1, 0, 1) for t in want_all) >= 10
    al.haplotag_enable(table)
    reads = ["".join(random.Random(i).choice("ACGT") for _ in range(k + 40)) for i in range(len(rows) + 30)]
    for n in (1, 3, 4, 5, 63, 64, 65, len(rows) + 30):
        rb, ro = pack(reads[:n])
        d_r, d_o = B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)
        al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(ro[-1]), k + 40, m=2, effort=2)
        al.sync()
        arena_ints = al.arena_ints()
        assert arena_ints >= 2 * (k + 40)
        results, arena, seen = layout(rows, n, arena_ints, 100 * k + n)
        d_results, d_arena, _ = al.device_results()
        B.device_upload(0, d_results, results)
        B.device_upload(0, d_arena, arena)
        want = [H.tag_of(table, p) for p in seen]
        got = al.haplotags(n)
        assert [tuple(int(x) for x in r) for r in got] == want, (k, n)
        if n >= 3:
            assert want[2] == H.tag_of(table, SPECIAL) != (0, 0, 0, 0)
        if n >= 4:
            assert want[3] == (0, 0, 0, 0)
        if n >= 63:
            assert sum(1 for t in want if t[0]) > n // 4
        if n == len(rows) + 30:
            al.haplotag_enable([0] * (N_UNITIGS + 1))
            assert not al.haplotags(n).view(np.uint32).any()
            last = [0] * N_UNITIGS + [9]   # only table[n_unitigs]
            al.haplotag_enable(last)
            assert [tuple(int(x) for x in r) for r in al.haplotags(n)] == [H.tag_of(last, p) for p in seen]
            al.haplotag_enable(None)
            with pytest.raises(B.BgrError, match="error -1.*no tag table"):
                al.haplotags(n)
            al.haplotag_enable(table)
        d_r.free()
        d_o.free()


# ---- rows of the mapper -----------------------------------------------------------------------------------------------------------------------
def random_table(n_unitigs, seed, blocks=6, p=0.5):
    rng = random.Random(seed)
    return [0] + [(rng.randrange(1, blocks + 1) << 1 | rng.randrange(2)) if rng.random() < p else 0 for _ in range(n_unitigs)]


@pytest.mark.parametrize("k", [31, 40])
def test_mapper_rows(k):
    s = Synth(60000, 90, 2, k, 300 + k)
    seqs, offs = s.unitigs()
    g = B.Graph.build(k, seqs, offs)
    n_unitigs = g.info()["n_unitigs"]
    table = random_table(n_unitigs, k)
    al = B.Aligner(g, 0)
    al.haplotag_enable(table)
    rb, ro = s.reads(0, 3000, 150, 3, k)
    lb, lo = s.reads(0, 8, 5000, 0, k + 1)
    reads = strings(rb, ro) + strings(lb, lo)
    reads = [W.reverse_complements(r) if i % 2 else r for i, r in enumerate(reads)]
    n = len(reads)
    pb, po = pack(reads)
    rows = W.rows_of(*al.align(pb, po, m=2, effort=2))
    want = [H.tag_of(table, p) for _, p in rows]
    assert [tuple(int(x) for x in r) for r in al.haplotags(n)] == want
    assert sum(1 for t in want if t[0]) > 1500 and any(t[3] for t in want) and any(len(p) > 17 for _, p in rows)
    d_r, d_o = B.DeviceBuffer(0, pb), B.DeviceBuffer(0, po)
    for m, e in ((0, 0), (5, 3)):
        al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, int(po[-1]), 5000, m=m, effort=e)
        got = al.haplotags(n)   # (un-waited: the kernel runs behind the launch, on its stream)
        rows = W.rows_of(*al.fetch(n, int(po[-1]) + 8 * n + 8))
        assert [tuple(int(x) for x in r) for r in got] == [H.tag_of(table, p) for _, p in rows], (k, m)
    # the refusals
    with pytest.raises(B.BgrError, match="error -1.*n_reads"):
        al.haplotags(n - 1)
    for bad in (table[:-1], table + [0], [0]):
        with pytest.raises(B.BgrError, match="error -1.*n_rows"):
            al.haplotag_enable(bad)
        with pytest.raises(B.BgrError, match="error -1.*n_rows"):
            g.haplotag_enable(bad)
    assert [tuple(int(x) for x in r) for r in al.haplotags(n)] == [H.tag_of(table, p) for _, p in rows]   # (a refused enable leaves the table alone)
    if k <= 32:   # (a graph with two-word keys maps in the greedy modes only)
        al.align_device(d_r.data_ptr(), d_o.data_ptr(), 50, int(po[50]), 150, mode=B.MODE_EXHAUSTIVE)
        with pytest.raises(B.BgrError, match="error -1.*exhaustive"):
            al.haplotags(50)
    d_r.free()
    d_o.free()
    assert not g.haplotag_enabled()
    g.haplotag_enable(table)
    assert g.haplotag_enabled()
    g.haplotag_enable(None)
    assert not g.haplotag_enabled()


# ---- the bytes of the text call and of a run ----------------------------------------------------------------------------------------------------
def run_inputs(k, tmp):
    """a graph with long paths (k = 8: rows of more than 16 and more than 32 unitigs) or a wide one (k = 48), reads with headers of several shapes,
    the rows of the batch API and a table written as a blocks file -> dict"""
    s = Synth(60000, max(40, 2 * k), 2, k, 900 + k)
    seqs, offs = s.unitigs()
    us = [""] + strings(seqs, offs)
    reads = []
    for L, n in ((k + 1, 20), (150, 400), (251, 60), (450, 40), (1000, 40), (5000, 6)):
        rb, ro = s.reads(0, n, L, 1 if L >= 1000 else 3, 31 * k + L)
        reads += strings(rb, ro)
    reads = [W.reverse_complements(r) if i % 2 else r for i, r in enumerate(reads)]
    random.Random(k).shuffle(reads)
    heads = [">r%d" % i + (" pair/1" if i % 3 == 0 else "\tx" if i % 5 == 0 else "") for i in range(len(reads))]
    uf, rf, bf, zf = (os.path.join(tmp, x) for x in ("u.fa", "r.fa", "blocks.tsv", "zero.tsv"))
    with open(uf, "w") as f:
        f.write("".join(">%d\n%s\n" % (i, u) for i, u in enumerate(us[1:])))
    with open(rf, "w") as f:
        f.write("".join("%s\n%s\n" % (h, r) for h, r in zip(heads, reads)))
    n_unitigs = len(us) - 1
    rng = random.Random(7 * k)
    ids = list(range(1, n_unitigs + 1))
    rng.shuffle(ids)
    ids = ids[:2 * (n_unitigs // 3)]   # two thirds of the unitigs in pairs, in twelve blocks
    lines = ["%d\t0\t1\t1\t1\t2\t%d\t%d\t+\t.\n" % (1 + i % 12, ids[2 * i] * rng.choice((1, -1)), ids[2 * i + 1] * rng.choice((1, -1))) for i in range(len(ids) // 2)]
    data = (BR.HEADER + "".join(lines)).encode()
    open(bf, "wb").write(data)
    open(zf, "wb").write(BR.HEADER.encode())
    table = H.table_of_file(data, n_unitigs)
    g = B.Graph.build(k, seqs, offs)
    al = B.Aligner(g, 0)
    rows = W.rows_of(*al.align(*pack(reads), m=2, effort=2))
    plain, bug = G.gaf_of(us, k, heads, reads, rows)
    assert bug is None
    tags = [H.tag_of(table, p) for _, p in rows if p]
    want = "".join(H.tagged_line(ln + "\n", t) for ln, t in zip(plain.split("\n"), tags))
    assert len(tags) == plain.count("\n") > 150 and sum(1 for t in tags if t[0]) > 100 and want != plain
    if k == 8:   # the rows the write kernel walks again, tagged
        assert any(len(p) - 1 > 32 and H.tag_of(table, p)[0] for _, p in rows) and any(16 < len(p) - 1 <= 32 and H.tag_of(table, p)[0] for _, p in rows)
    return dict(k=k, g=g, al=al, us=us, heads=heads, reads=reads, rows=rows, table=table, plain=plain.encode(), want=want.encode(), uf=uf, rf=rf, bf=bf, zf=zf,
                args=["-r", rf, "-k", str(k), "-g", uf, "-m", "2", "-e", "2", "--gaf"])


@pytest.fixture(scope="module", params=[8, 48], ids=["k8", "k48"])
def inputs(request, tmp_path_factory):
    return run_inputs(request.param, str(tmp_path_factory.mktemp("haplotag")))


def test_text_call(inputs):
    """bgr_align_fasta_text with want_output 3: tagged lines with a table, through the write launch of a second fetch too; the exact untagged bytes
    with an all-zero table and with the table off again"""
    c = inputs
    al = c["al"]
    text = open(c["rf"], "rb").read()
    assert al.align_fasta_text(text, m=2, effort=2, want_output=3)[0] == c["plain"]
    al.haplotag_enable(c["table"])
    p, na, info = al.align_fasta_text(text, m=2, effort=2, want_output=3)
    assert not info["irregular"] and p == c["want"]
    p2, na2, _ = al.align_fasta_text(text, m=2, effort=2, want_output=3, paths_cap=1000)   # BGR_E_CAPACITY, then bgr_aligner_fetch_text
    assert p2 == c["want"] and na2 == na
    al.haplotag_enable([0] * len(c["table"]))
    pz, naz, _ = al.align_fasta_text(text, m=2, effort=2, want_output=3)
    assert pz == c["plain"] and naz == na
    al.haplotag_enable(None)
    assert al.align_fasta_text(text, m=2, effort=2, want_output=3)[0] == c["plain"]
    assert al.align_fasta_text(text, m=2, effort=2)[0].count(b".") > 300   # (the paths format is not tagged)


@pytest.mark.parametrize("extra", ROUTES, ids=ROUTE_IDS)
def test_cli_run_bytes(inputs, extra):
    """--gaf --haplotag on every route: gaf_ref's lines plus the reference suffix, byte for byte; notAligned.fa and the counters those of the run
    without the flag, which writes today's GAF; a file of the header alone tags nothing"""
    c = inputs
    off = run(c["args"] + extra, flags=())
    assert off["paths"] == c["plain"]
    on = run(c["args"] + extra, flags=(), more=["--haplotag", c["bf"]])
    assert on["paths"] == c["want"]
    assert on["na"] == off["na"]
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
    assert strip(on["out"]) == strip(off["out"])
    if not extra or extra == ["--host-route"]:
        zero = run(c["args"] + extra, flags=(), more=["--haplotag", c["zf"]])
        assert zero["paths"] == c["plain"] and zero["na"] == off["na"]


@pytest.mark.parametrize("route", [0, 1], ids=["text", "host"])
def test_align_all_with_the_graphs_switch(inputs, route, tmp_path):
    c = inputs
    g = c["g"]
    PF, NF = str(tmp_path / "p"), str(tmp_path / "n")
    g.haplotag_enable(c["table"])
    try:
        with pytest.raises(B.BgrError, match="error -1.*gaf"):
            B.align_all(g, c["rf"], PF, NF, m=2, effort=2, route=route)
        B.align_all(g, c["rf"], PF, NF, m=2, effort=2, route=route, gaf=True, threads=3)
        assert open(PF, "rb").read() == c["want"]
        with pytest.raises(B.BgrError, match="error -1"):
            B.align_all(g, c["rf"], PF, NF, m=2, effort=2, route=route, gaf=True, mode=B.MODE_EXHAUSTIVE)
    finally:
        g.haplotag_enable(None)
    B.align_all(g, c["rf"], PF, NF, m=2, effort=2, route=route, gaf=True)
    assert open(PF, "rb").read() == c["plain"]


# ---- two planted haplotypes, end to end ---------------------------------------------------------------------------------------------------------
def test_planted_end_to_end(tmp_path):
    """run 1 writes --blocks; run 2 tags the same reads with it at -m 0: every read that lies in only one haplotype carries PS 1, no vote for
    another block, votes for one haplotype only, and the HP of its haplotype's other reads -- the opposite of the other haplotype's"""
    k = 31
    haps, unitigs, reads = planted(2024)
    uf, rf = str(tmp_path / "u.fa"), str(tmp_path / "r.fa")
    open(uf, "w").write("".join(">u%d\n%s\n" % (i, u) for i, u in enumerate(unitigs)))
    open(rf, "w").write("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    args = ["-r", rf, "-k", str(k), "-g", uf, "-e", "2"]
    r1 = run(args + ["-m", "2"], flags=("blocks",))
    bf = str(tmp_path / "blocks.tsv")
    open(bf, "wb").write(r1["blocks"])
    assert r1["blocks"].count(b"\n") == 21
    r2 = run(args + ["-m", "0", "--gaf", "--haplotag", bf], flags=())
    only = [None] * len(reads)   # the haplotype a read occurs in, when it is only one
    for i, r in enumerate(reads):
        inside = [r in h or rc(r) in h for h in haps]
        assert any(inside)
        if inside[0] != inside[1]:
            only[i] = 0 if inside[0] else 1
    assert only.count(0) == 153 and only.count(1) == 183
    hp = [set(), set()]
    tagged = [0, 0]
    for ln in r2["paths"].decode().split("\n")[:-1]:
        c = ln.split("\t")
        i = int(c[0][1:])
        if only[i] is None:
            continue
        assert len(c) == 18 and c[13] == "PS:i:1" and c[17] == "ho:i:0", ln
        h, a, b = int(c[14][5:]), int(c[15][5:]), int(c[16][5:])
        assert c[14].startswith("HP:i:") and c[15].startswith("ha:i:") and c[16].startswith("hb:i:") and (a == 0) != (b == 0) and h == (1 if a else 2), ln
        hp[only[i]].add(h)
        tagged[only[i]] += 1
    assert tagged[0] >= 100 and tagged[1] >= 100, tagged
    assert len(hp[0]) == 1 and len(hp[1]) == 1 and hp[0] != hp[1], hp


# ---- the CLI's refusals -----------------------------------------------------------------------------------------------------------------------
def test_cli_refusals(inputs, tmp_path):
    c = inputs
    base = ["-r", c["rf"], "-k", str(c["k"]), "-g", c["uf"]]

    def cli(*more):
        return subprocess.run([B.CLI_PATH] + base + list(more), cwd=tmp_path, capture_output=True, text=True, timeout=300)

    p = cli("--haplotag", c["bf"])
    assert p.returncode == 2 and "--gaf" in p.stderr
    p = cli("--gaf", "-b", "--haplotag", c["bf"])
    assert p.returncode == 2 and "-b" in p.stderr
    p = cli("--gaf", "--haplotag", str(tmp_path / "missing.tsv"))
    assert p.returncode == 2 and "cannot open" in p.stderr and "The End" not in p.stdout
    bad = tmp_path / "bad.tsv"
    bad.write_bytes(open(c["bf"], "rb").read() + b"1\t0\t1\t1\t1\t2\t0\t3\t+\t.\n")
    n_lines = bad.read_bytes().count(b"\n")
    p = cli("--gaf", "--haplotag", str(bad))
    assert p.returncode == 2 and "line %d" % n_lines in p.stderr and "The End" not in p.stdout and not os.path.exists(tmp_path / "paths")
    bad.write_bytes(b"1\t0\t1\t1\t1\t2\t1\t3\t+\t.\n")
    p = cli("--gaf", "--haplotag", str(bad))
    assert p.returncode == 2 and "line 1" in p.stderr
