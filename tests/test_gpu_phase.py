"""Read-backed phasing on the GPU machine: `--phase` through the CLI on every route, next to `--bubbles --gfa --triples` of the same run, and the
records bgr_align_all keeps in the graph -- against phase_ref.py (the definition in plain Python, which test_triples_host.py makes check itself)
over bubbles_ref of the same run's L lines and the same run's triples file."""
import os
import subprocess

import pytest

import bgreat_amd as B
import bubbles_ref as BR
import links_ref as K
import phase_ref as P
import triples_ref as T
from test_gpu_triples import ROUTE_IDS, ROUTES, run, synth_files   # noqa: F401 (synth_files is a fixture)
from util import GOLD, parse_counters

pytestmark = pytest.mark.gpu

FLAGS = ("phase", "bubbles", "gfa", "triples")


def parse_bubbles(b):
    """the lines of a `--bubbles` file -> {(source, sink, branch1, branch2): (in1, out1, in2, out2)}"""
    lines = b.decode("latin-1").split("\n")
    assert lines[0].startswith("#source\tsink\tbranch1\tbranch2") and lines[-1] == ""
    out = {}
    for ln in lines[1:-1]:
        c = ln.split("\t")
        out[tuple(int(x) for x in c[:4])] = tuple(int(x) for x in c[6:10])
    return out


def link_count(links, a, b):
    return links.get(K.canonical(a, b), 0)


@pytest.mark.parametrize("extra", ROUTES, ids=ROUTE_IDS)
def test_cli_phase_with_bubbles_gfa_and_triples(synth_files, extra):
    """the file = phase_ref over bubbles_ref of the same run's L lines and the same run's triples; its bubbles are lines of the bubbles file; no
    count exceeds the links it passes through; paths, notAligned.fa and the counters are those of a run without any flag"""
    args, us, plain, rows = synth_files
    r = run(args + extra, flags=FLAGS)
    _, _, links = K.parse_gfa(r["gfa"])
    triples = T.parse_text(r["triples"])
    assert triples == T.triples_of(rows, len(us) - 1)
    bubbles = BR.bubbles_of(links)
    want = P.phase_of(bubbles, triples)
    assert r["phase"] == P.phase_text(want) and r["bubbles"] == BR.bubbles_text(us, bubbles)
    recs = P.parse_text(r["phase"])
    assert len(recs) == 22 and sum(P.call(x[5]) != "." for x in recs) >= 10 and any(x[5] == (0, 0, 0, 0) for x in recs)   # (22 neighbour pairs, 14 crossed by a read: counted on the CPU)
    assert [x[0] for x in recs] == sorted(x[0] for x in recs) and all(x[0] > 0 for x in recs)
    in_file = parse_bubbles(r["bubbles"])
    for rec in recs:
        m, s, ins, outs, t, n = rec
        x, y = P.bubbles_of_record(rec)
        assert x in in_file and y in in_file and x != y, rec
        for i in range(2):
            for j in range(2):   # a read that threads (in_i, m, out_j) crosses the four links source -> in_i -> m -> out_j -> sink ... of which the triple holds the middle two
                assert n[2 * i + j] <= min(link_count(links, ins[i], m), link_count(links, m, outs[j])), rec
        assert n[0] + n[1] <= link_count(links, ins[0], m) and n[2] + n[3] <= link_count(links, ins[1], m), rec
        assert n[0] + n[2] <= link_count(links, m, outs[0]) and n[1] + n[3] <= link_count(links, m, outs[1]), rec
    assert r["paths"] == plain["paths"] and r["na"] == plain["na"] and parse_counters(r["out"]) == parse_counters(plain["out"])
    r5 = run(args + extra, flags=FLAGS, more=["--min-link", "5"])
    assert r5["gfa"] == r["gfa"] and r5["triples"] == r["triples"] and r5["bubbles"] == BR.bubbles_text(us, BR.bubbles_of(links, 5))
    assert r5["phase"] == P.phase_text(P.phase_of(BR.bubbles_of(links, 5), triples))
    rn = run(args + extra, flags=FLAGS, more=["--min-link", "999999999"])
    assert rn["phase"] == P.phase_text([]) == b"#via\tsource\tin1\tin2\tout1\tout2\tsink\tn11\tn12\tn21\tn22\tphase\n" and rn["triples"] == r["triples"]


def test_cli_phase_alone_changes_nothing_else(synth_files):
    """without the other flags: the same file, and stdout too is what it is without the flag"""
    args, us, plain, rows = synth_files
    alone = run(args, flags=("phase",))
    both = run(args, flags=FLAGS)
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("Indexing in seconds", "Reads/seconds", "Mapping in seconds"))]
    assert alone["phase"] == both["phase"] and alone["phase"].count(b"\n") == 23 and strip(alone["out"]) == strip(plain["out"])
    assert alone["paths"] == plain["paths"] and alone["na"] == plain["na"]
    a3 = run(args, flags=("phase",), more=["--min-link", "3"])
    _, _, links = K.parse_gfa(both["gfa"])
    assert a3["phase"] == P.phase_text(P.phase_of(BR.bubbles_of(links, 3), T.parse_text(both["triples"])))


def test_cli_refusals(tmp_path):
    base = [B.CLI_PATH, "-r", os.path.join(GOLD, "deg_reads.fa"), "-k", "5"]
    f = str(tmp_path / "x.phase")
    def cli(graph, *more):
        return subprocess.run(base + ["-g", os.path.join(GOLD, graph)] + list(more), cwd=tmp_path, capture_output=True, text=True, timeout=300)
    pr = cli("deg_unitig.fa", "--phase", f, "-b")
    assert pr.returncode == 2 and "--phase" in pr.stderr and "-b" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig_exc.fa", "--phase", f)
    assert pr.returncode == 2 and "--phase" in pr.stderr and "ACGT" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--min-link", "2")   # the threshold alone
    assert pr.returncode == 2 and "--min-link" in pr.stderr, pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--phase", f, "--min-link", "0")
    assert pr.returncode == 2 and "--min-link" in pr.stderr and not os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--triples", str(tmp_path / "x.triples"), "--min-link", "2")   # ... is none of --triples
    assert pr.returncode == 2 and "--min-link" in pr.stderr and not os.path.exists(tmp_path / "x.triples"), pr.stderr[-500:]
    pr = cli("deg_unitig.fa", "--phase", f, "--min-link", "2")
    assert pr.returncode == 0 and os.path.exists(f), pr.stderr[-500:]
    pr = cli("deg_unitig_exc.fa", "--triples", str(tmp_path / "x.triples"))   # triples read no characters: a graph with other letters is fine
    assert pr.returncode == 0 and os.path.exists(tmp_path / "x.triples"), pr.stderr[-500:]


def test_align_all_keeps_triples_and_phase_in_the_graph(synth_files, tmp_path):
    args, us, _, rows = synth_files
    g = B.Graph.from_fasta(args[5], 31)
    PF, NF = str(tmp_path / "p"), str(tmp_path / "n")
    for fetch in (g.triples, g.phase):
        with pytest.raises(B.BgrError):
            fetch()
    g.phase_enable(min_link=2)
    assert g.phase_enabled() and not g.triples_enabled() and not g.bubbles_enabled() and not g.links_enabled()
    B.align_all(g, args[1], PF, NF, m=2, effort=2, threads=2)
    counts = {(int(r["from"]), int(r["to"])): int(r["count"]) for r in g.links()}   # the switch implies the links, the bubbles and the triples
    triples = {t[:3]: t[3] for t in T.as_tuples(g.triples())}
    assert triples == T.triples_of(rows, len(us) - 1)
    bubbles = BR.bubbles_of(counts, 2)
    assert BR.as_tuples(g.bubbles()) == bubbles and len(bubbles) > 10
    want = P.phase_of(bubbles, triples)
    assert P.as_tuples(g.phase()) == want and len(want) > 10
    assert P.as_tuples(B.bubbles_phase(g.bubbles(), g.triples())) == want   # the library call over what the graph delivers
    B.write_phase(str(tmp_path / "ph"), g, g.phase())
    B.write_triples(str(tmp_path / "tr"), g, g.triples())
    assert open(tmp_path / "ph", "rb").read() == P.phase_text(want) and open(tmp_path / "tr", "rb").read() == T.triples_text(triples)
    g.phase_enable(False)
    B.align_all(g, args[1], PF, NF, m=2, effort=2)   # a run with the switches off leaves the kept totals alone
    assert P.as_tuples(g.phase()) == want and {t[:3]: t[3] for t in T.as_tuples(g.triples())} == triples
    g.triples_enable()
    B.align_all(g, args[1] + "," + args[1], PF, NF, m=2, effort=2, route=1)   # the next run with the triples' switch replaces them; the phase records stay
    assert {t[:3]: t[3] for t in T.as_tuples(g.triples())} == {t: 2 * n for t, n in triples.items()} and P.as_tuples(g.phase()) == want
    g.phase_enable()
    with pytest.raises(B.BgrError):   # a run that fails leaves none
        B.align_all(g, str(tmp_path / "missing.fa"), PF, NF)
    for fetch in (g.triples, g.phase):
        with pytest.raises(B.BgrError):
            fetch()
