"""Un-waited consecutive bgr_align_device launches take turns on two streams with two sets of launch buffers (bgreat_amd/csrc/launch_taker.h,
BGR_KNOB_DEVICE_OVERLAP): whatever stream took a launch, fetch / path_stats / pass_counts / launch_info / device_results describe the LAST one,
counters and the counting features' tables hold every launch once, a caller that waits between its launches never leaves the aligner's own
buffers, and the calls that copy on the aligner's stream around their launch (begin / wait, bgr_align_batch) stay on it.  Against the oracle.
The graphs are tools/synth.py's (seeded, as in the other GPU tests) at k = 31 and k = 12; four batches of 3 000 - 6 000 reads of 60 - 200 bp, some
with an N: more than one workgroup's worth of tasks, follow-up items included (asserted below).  Which stream a launch of so small a batch goes
to depends on whether the one before has finished: test_second_buffers_are_used makes sure the second set is taken with a longer launch in front."""
import functools

import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
from tools.synth import Synth

pytestmark = pytest.mark.gpu

SIZES = (3000, 4500, 6000, 5200)
MAXLEN = 200


class Case:
    """graph, four batches (host + device) and what the oracle says of each; made once per (k, mode), never changed"""

    def __init__(self, k, mode, inside=False):
        rng = np.random.default_rng(100 + k)
        # (inside: unitigs of about 400 bases, as in test_gpu_inside.py -- many of the reads then lie inside one and have no anchor -- and the inside index)
        s = Synth(60000, 400 if inside else max(40, 2 * k), 2, k, 700 + k)
        self.seqs, self.offs = s.unitigs()
        self.k, self.mode = k, mode
        self.graph = B.Graph.build(k, self.seqs, self.offs, anchors=(mode == B.MODE_ANCHORS))
        if inside:
            self.graph.inside_build()
        orc = oracle_py.Oracle(k, self.seqs, self.offs, anchors=(mode == B.MODE_ANCHORS))
        self.batches, self.want, self.dev = [], [], []
        self.counters = dict.fromkeys(["reads", "no_overlap", "aligned", "not_aligned", "overlaps"], 0)
        first = 0
        for n in SIZES:
            full, _ = s.reads(first, n, MAXLEN, 2, 31 + k)
            first += n
            lens = rng.integers(60, MAXLEN + 1, size=n)
            ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            rb = np.concatenate([full[i * MAXLEN: i * MAXLEN + lens[i]] for i in range(n)]).astype(np.uint8)
            for i in rng.choice(n, n // 50, replace=False):   # an N somewhere in one read of fifty
                rb[int(ro[i]) + int(rng.integers(0, lens[i]))] = ord("N")
            self.batches.append((rb, ro))
            orc.reset()
            self.want.append(orc.align(rb, ro, m=2, effort=2, mode=mode))
            for key, v in orc.counters().items():
                self.counters[key] += v
            self.dev.append((B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro)))
        # a longer launch (the four batches, four times over) for the tests that need the aligner's stream busy
        rb = np.concatenate([b[0] for b in self.batches] * 4)
        lens = np.concatenate([np.diff(b[1].astype(np.int64)) for b in self.batches] * 4)
        ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.long = (B.DeviceBuffer(0, rb), B.DeviceBuffer(0, ro), len(lens), int(ro[-1]))

    def launch(self, al, i, mode=None):
        rb, ro = self.batches[i]
        al.align_device(self.dev[i][0].data_ptr(), self.dev[i][1].data_ptr(), len(ro) - 1, int(ro[-1]), MAXLEN, m=2, effort=2, mode=self.mode if mode is None else mode)

    def launch_long(self, al):
        d_r, d_o, n, total = self.long
        al.align_device(d_r.data_ptr(), d_o.data_ptr(), n, total, MAXLEN, m=2, effort=2, mode=self.mode)

    def fetch(self, al, i):
        rb, ro = self.batches[i]
        return al.fetch(len(ro) - 1, int(ro[-1]) + 8 * len(ro))

    def aligner(self, overlap=True):
        al = B.Aligner(self.graph, 0)
        if not overlap:
            al.set_knob(B.KNOB_DEVICE_OVERLAP, 1)
        return al


@functools.lru_cache(maxsize=None)
def case(k, mode=B.MODE_GREEDY, inside=False):
    return Case(k, mode, inside)


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("k", [31, 12])
def test_four_unwaited_launches(k):
    """(a) four launches, no wait: fetch gives batch 4, the counters all four, pass_counts and launch_info those of a lone launch of batch 4"""
    c = case(k)
    lone = c.aligner()
    c.launch(lone, 3)
    want_pass, want_info = lone.pass_counts(), lone.launch_info()
    assert want_pass[0] > 0 and want_info["blocks"] > 1, (want_pass, want_info)   # follow-up items; more than one workgroup
    assert same(c.fetch(lone, 3), c.want[3])
    al = c.aligner()
    for i in range(4):
        c.launch(al, i)
    assert same(c.fetch(al, 3), c.want[3])
    assert al.counters() == c.counters
    assert al.pass_counts() == want_pass and al.launch_info() == want_info
    assert al.arena_ints() == lone.arena_ints()


@pytest.mark.parametrize("k", [31, 12])
def test_waited_launches_stay_on_the_primary(k):
    """(b) launch, fetch, launch, fetch: every fetch is the oracle's, and the three device pointers never change (the primary is idle: it takes the launch)"""
    c = case(k)
    al = c.aligner()
    c.launch_long(al)   # (sizes the buffers: nothing grows afterwards)
    al.sync()
    ptrs = al.device_results()
    assert all(ptrs)
    for i in (2, 0, 1, 3):
        c.launch(al, i)
        assert same(c.fetch(al, i), c.want[i])
        assert al.device_results() == ptrs
    c.launch(al, 2)
    al.sync()
    c.launch(al, 1)
    assert al.device_results() == ptrs
    assert same(c.fetch(al, 1), c.want[1])


@pytest.mark.parametrize("k", [31, 12])
def test_second_buffers_are_used(k):
    """a launch right behind a long one that nobody waited for goes to the second set of buffers -- other device pointers -- and path_stats and fetch
    describe it all the same (c); behind a wait the next launch is back on the aligner's own.  With the knob at 1 the pointers never change."""
    c = case(k)
    ref = c.aligner(overlap=False)
    c.launch_long(ref)   # (sizes the buffers: nothing grows afterwards)
    ref.sync()
    ref_own = ref.device_results()
    c.launch_long(ref)
    c.launch(ref, 1)
    assert ref.device_results() == ref_own
    want_stats = ref.path_stats(c.dev[1][0].data_ptr(), c.dev[1][1].data_ptr(), SIZES[1])
    assert same(c.fetch(ref, 1), c.want[1])
    al = c.aligner()
    c.launch_long(al)
    al.sync()
    own = al.device_results()
    c.launch_long(al)
    c.launch(al, 1)
    other = al.device_results()
    assert all(other) and all(o != p for o, p in zip(other, own)), (own, other)
    stats = al.path_stats(c.dev[1][0].data_ptr(), c.dev[1][1].data_ptr(), SIZES[1])
    assert stats.tobytes() == want_stats.tobytes() and stats["aligned"].sum() > 0
    assert same(c.fetch(al, 1), c.want[1])
    assert al.device_results() == other   # (reading the last launch does not move it)
    al.sync()
    c.launch(al, 2)
    assert al.device_results() == own
    assert same(c.fetch(al, 2), c.want[2])


@pytest.mark.parametrize("k", [31, 12])
def test_two_unwaited_launches_describe_the_second(k):
    """(c) launch 1, launch 2, then path_stats and fetch: both are batch 2's"""
    c = case(k)
    ref = c.aligner(overlap=False)
    c.launch(ref, 1)
    want_stats = ref.path_stats(c.dev[1][0].data_ptr(), c.dev[1][1].data_ptr(), SIZES[1])
    al = c.aligner()
    c.launch(al, 0)
    c.launch(al, 1)
    assert al.path_stats(c.dev[1][0].data_ptr(), c.dev[1][1].data_ptr(), SIZES[1]).tobytes() == want_stats.tobytes()
    assert same(c.fetch(al, 1), c.want[1])
    with pytest.raises(B.BgrError, match="error -1.*differs from the last"):
        al.fetch(SIZES[0], 16)


FEATURES = {
    "abundance": (lambda al: al.abundance_enable(), lambda al: al.abundance().tobytes()),
    "links": (lambda al: al.links_enable(), lambda al: al.links().tobytes()),
    "triples": (lambda al: al.triples_enable(), lambda al: al.triples().tobytes()),
    "pileup": (lambda al: al.pileup_enable(), lambda al: al.pileup()[0].tobytes() + al.abundance().tobytes()),
    "strands": (lambda al: al.pileup_strands_enable(), lambda al: al.pileup_forward().tobytes()),
    # (on a graph of its own, with the inside index: what the pass mapped, and the rows of the last batch with those it wrote.  With the reads packed by
    # the pre-pass: behind a launch that stages them from the characters the pass does not map the same reads from run to run at this size, on one stream
    # too -- 47 170 to 47 304 of the long launch's 74 800 reads in five runs, 48 788 every time from the planes -- so that form has nothing to compare)
    "inside": (lambda al: (al.set_knob(B.KNOB_GREEDY_PREPASS, 1), al.inside_enable()),
               lambda al: al.inside_count().to_bytes(8, "little") + b"".join(x.tobytes() for x in al.fetch(SIZES[3], SIZES[3] * (MAXLEN + 8) + 8))),
}


@pytest.mark.parametrize("feature", sorted(FEATURES))
@pytest.mark.parametrize("k", [31, 12])
def test_counting_features(k, feature):
    """(d) the feature's table behind un-waited launches (a long one in front, so that both streams count) is, byte for byte, that of an aligner
    that keeps every launch on its own stream; enabled on an aligner whose twin already exists"""
    c = case(k, inside=(feature == "inside"))
    enable, read = FEATURES[feature]
    ref = c.aligner(overlap=False)
    enable(ref)
    al = c.aligner()
    c.launch_long(al)
    c.launch(al, 0)   # (the twin exists from here on)
    al.sync()
    enable(al)
    for x in (ref, al):
        c.launch_long(x)
        for i in range(4):
            c.launch(x, i)
    want = read(ref)
    assert read(al) == want and any(want)
    assert al.counters()["reads"] == ref.counters()["reads"] + SIZES[0] + c.long[2]
    if feature == "inside":
        assert ref.inside_count() > 0


def _twin_in_place(c, al):
    """-> the aligner's own device pointers; its twin exists from here on and both streams are idle"""
    c.launch_long(al)   # (sizes the buffers: nothing grows afterwards)
    al.sync()
    own = al.device_results()
    c.launch_long(al)
    c.launch(al, 0)
    al.sync()
    return own


@pytest.mark.parametrize("k", [31, 12])
def test_switching_off_after_the_twin_exists(k):
    """links and the pileup enabled, the launch sequence, both disabled, the sequence again: the tables stay as they were after the first sequence, and
    they and the abundance (which stays on) are, byte for byte, those of an aligner that keeps every launch on its own stream and did the same"""
    c = case(k)

    def tables(x):
        return x.links().tobytes(), x.pileup()[0].tobytes(), x.abundance().tobytes()

    got = []
    for x in (c.aligner(overlap=False), c.aligner()):
        _twin_in_place(c, x)
        snaps = []
        for on in (True, False):
            x.links_enable(on)
            x.pileup_enable(on)
            c.launch_long(x)
            for i in range(4):
                c.launch(x, i)
            snaps.append(tables(x))
        got.append(snaps)
    ref, al = got
    assert al[0] == ref[0] and all(any(t) for t in ref[0])
    assert al[1] == ref[1]
    assert al[1][:2] == al[0][:2] and al[1][2] != al[0][2]   # (switched off: nothing added to links and pileup; the abundance went on counting)


@pytest.mark.parametrize("k", [31, 12])
def test_a_knob_set_after_the_twin_exists_reaches_the_twin(k):
    """BGR_KNOB_GREEDY_FAST set on an aligner whose twin exists: the launch the twin takes is the lone aligner's with the same knob -- the general
    kernel alone, another geometry than the default's -- and its rows are the oracle's"""
    c = case(k)
    default = c.aligner()
    c.launch(default, 1)
    lone = c.aligner()
    lone.set_knob(B.KNOB_GREEDY_FAST, 1)
    c.launch(lone, 1)
    want_pass, want_info = lone.pass_counts(), lone.launch_info()
    assert want_info != default.launch_info(), want_info   # (the knob shows in what is compared below)
    al = c.aligner()
    own = _twin_in_place(c, al)
    al.set_knob(B.KNOB_GREEDY_FAST, 1)
    c.launch_long(al)
    c.launch(al, 1)
    other = al.device_results()
    assert all(other) and all(o != p for o, p in zip(other, own)), (own, other)   # (the twin took the launch)
    assert al.launch_info() == want_info and al.pass_counts() == want_pass
    assert same(c.fetch(al, 1), c.want[1])


def test_anchors_mode():
    """(e) anchors mode, as (a)"""
    c = case(31, B.MODE_ANCHORS)
    al = c.aligner()
    c.launch_long(al)
    for i in range(4):
        c.launch(al, i)
    assert same(c.fetch(al, 3), c.want[3])
    got = al.counters()
    assert {key: got[key] - 4 * c.counters[key] for key in got} == c.counters   # (the long launch is the four batches four times)


def test_exhaustive_launch_between_greedy_ones():
    """(f) an exhaustive launch between two greedy ones stays on the aligner's own stream: its fetch is the oracle's and last_pass_runs reports it"""
    c = case(31)
    rb, ro = c.batches[0]
    n = 600
    want = oracle_py.Oracle(31, c.seqs, c.offs).align(rb[:int(ro[n])], ro[:n + 1], m=2, effort=2, mode=B.MODE_EXHAUSTIVE)
    al = c.aligner()
    c.launch_long(al)
    c.launch(al, 1)
    al.align_device(c.dev[0][0].data_ptr(), c.dev[0][1].data_ptr(), n, int(ro[n]), MAXLEN, m=2, effort=2, mode=B.MODE_EXHAUSTIVE)
    assert same(al.fetch(n, int(ro[n]) + 8 * n + 8), want)
    runs, memo_cap = al.last_pass_runs()
    assert runs >= 1 and memo_cap > 0
    c.launch(al, 2)
    assert same(c.fetch(al, 2), c.want[2])
    assert al.last_pass_runs() == (0, 0)


def test_internal_callers_stay_on_their_stream():
    """(g) begin / wait and bgr_align_batch on an aligner whose twin exists, behind device launches that nobody waited for -- the aligner's stream busy
    and the twin's idle (where the public form would go to the twin), and both busy: the oracle's rows.  Their copies to the device are on the
    aligner's stream, so their launch has to be there too."""
    c = case(31)
    al = c.aligner()
    c.launch_long(al)
    c.launch(al, 0)   # (the twin exists from here on)
    al.sync()
    for i in (1, 2):
        rb, ro = c.batches[i]
        c.launch_long(al)
        assert same(al.align_wait(al.align_begin(rb, ro, m=2, effort=2)), c.want[i])
        c.launch_long(al)
        assert same(al.align(rb, ro, m=2, effort=2), c.want[i])
        c.launch_long(al)
        c.launch(al, 3)   # (both streams busy)
        assert same(al.align_wait(al.align_begin(rb, ro, m=2, effort=2)), c.want[i])
        c.launch_long(al)
        c.launch(al, 3)
        assert same(al.align(rb, ro, m=2, effort=2), c.want[i])
    al.sync()
    got = al.counters()
    assert got["reads"] == 9 * c.long[2] + SIZES[0] + 4 * SIZES[3] + 4 * (SIZES[1] + SIZES[2])   # (every launch above, once)


@pytest.mark.parametrize("k", [31, 12])
def test_fetch_again_after_capacity(k):
    """(h) two un-waited launches, a fetch into too small a buffer: BGR_E_CAPACITY; the fetch into a larger one gives batch 2"""
    c = case(k)
    al = c.aligner()
    c.launch_long(al)
    c.launch(al, 1)
    with pytest.raises(B.BgrError, match="error -4"):
        al.fetch(SIZES[1], 4)
    assert same(c.fetch(al, 1), c.want[1])
    al2 = c.aligner()
    c.launch(al2, 0)
    c.launch(al2, 1)
    with pytest.raises(B.BgrError, match="error -4"):
        al2.fetch(SIZES[1], 4)
    assert same(c.fetch(al2, 1), c.want[1])
