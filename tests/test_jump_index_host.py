"""The jump index of the greedy anchor scan, host side (no GPU): the builder against the plain-Python reference tests/jump_ref.py on tiny
hand-made unitig sets and a synthetic compacted graph -- property P true and false, the sampled offsets, palindromes left out, the entry
content and placement --, the lossy table of the drop hook, blobs without the section, and the header check of the section's extent."""
import numpy as np
import pytest

import bgreat_amd as B
import jump_ref as J
from tools.synth import Synth


def pack(unitigs):
    seqs = np.frombuffer("".join(unitigs).encode(), dtype=np.uint8).copy()
    offs = np.zeros(len(unitigs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(u) for u in unitigs])
    return seqs, offs


def rc(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def rnd(n, seed):
    r = np.random.RandomState(seed)
    return "".join("ACGT"[i] for i in r.randint(0, 4, n))


# k = 5: a chain a -> b (they overlap in k-1 = 4 bases), b carries the palindromes ACGT and CATG; and one unitig on its own
K = 5
A1 = "GATTACAGGC"
B1 = "AGGC" + "ACGTCCATG"
LONE = "CCCTGAGAAGTTTC"
COMPACTED = [A1, B1, LONE]
# the same, but a third unitig ENDS with an interior 4-mer of LONE (TGAG): property P does not hold
NOT_COMPACTED = [A1, B1, LONE, "GGGTATGAG"]


@pytest.fixture
def options():
    yield
    B.set_option("build_jump", 1)
    B.set_option("test.jump_drop", 0)
    B.set_option("test.wide_keys", 0)


def test_reference_sets():
    assert J.property_p(K, COMPACTED)
    assert not J.property_p(K, NOT_COMPACTED)
    # the sample: the (k-1)-mers whose hash selects them, about one in four, at any offset; never a palindrome
    u = rnd(6000, 11)
    s = J.sampled(12, [u])
    assert 0.22 < len(s) / (len(u) - 10) < 0.28 and {t % 4 for _, _, t, _ in s} == {0, 1, 2, 3}
    assert all(J.selects(J.mix64(key)) and key == min(J.kint(u[t:t + 11]), J.rcb(J.kint(u[t:t + 11]), 11)) for key, _, t, _ in s)
    pal = J.kint("ACGT")
    assert B1[4:8] == "ACGT" and J.rcb(pal, 4) == pal
    assert all(key != pal for key, _, _, _ in J.sampled(K, COMPACTED, stride=1)) and len(J.sampled(K, [B1], stride=1)) == len(B1) - 4 + 1 - 2  # (and CATG)


@pytest.mark.parametrize("k,unitigs", [(K, COMPACTED), (K, [A1]), (3, ["ACCA", "CATG"]), (12, [rnd(300, 1), rnd(41, 2), rnd(12, 3)])])
def test_builder_equals_reference(k, unitigs, options):
    if not J.property_p(k, unitigs):
        pytest.fail("the test's own unitig set must have property P")
    g = B.Graph.build(k, *pack(unitigs))
    info = g.jump_info()
    ref = J.table(k, unitigs)
    if not ref:  # (a set so small that the hash selects none of its (k-1)-mers: no index)
        assert g.jump_index() is None and info["jump_entries"] == 0 and info["jump_absent"] == 5
        return
    assert g.jump_index().shape == (J.n_buckets(k, unitigs), 4) and info["jump_stride"] == J.STRIDE
    assert J.graph_table(g) == ref
    n = sum(len(v) for v in ref.values())
    assert info["jump_entries"] == n and info["jump_bytes"] == 16 * J.n_buckets(k, unitigs)
    assert info["jump_absent"] == 0 and info["jump_absent_why"] == ""
    wanted = len(J.sampled(k, unitigs))
    assert info["jump_dropped_x1000"] == 1000 * (wanted - n) // wanted


def test_synthetic_graph_entries(options):
    """a compacted graph of a few hundred unitigs: the table is the reference's, entry for entry, and the drop rate is what two-entry buckets
    at one bucket per sample give (about one in ten)"""
    s = Synth(20000, 75, 2, 31, 99)
    seqs, offs = s.unitigs()
    unitigs = J.split(seqs, offs)
    assert J.property_p(31, unitigs)
    g = B.Graph.build(31, seqs, offs)
    assert J.graph_table(g) == J.table(31, unitigs)
    assert 0 < g.jump_info()["jump_dropped_x1000"] < 200


def test_drop_hook_gives_a_subset(options):
    unitigs = [rnd(400, 5), rnd(90, 6)]
    assert J.property_p(12, unitigs)
    full = {e for v in J.table(12, unitigs).values() for e in v}
    B.set_option("test.jump_drop", 3)
    g = B.Graph.build(12, *pack(unitigs))
    got = {e for v in J.graph_table(g).values() for e in v}
    every = {(uid | (J.FWD_CANON if fc else 0), t << 8 | J.tag_of(J.mix64(key))) for key, uid, t, fc in J.sampled(12, unitigs)}
    assert got and got <= every and len(got) < len(full)


def test_gate_and_byte_identical_blobs(options):
    seqs, offs = pack(NOT_COMPACTED)
    g = B.Graph.build(K, seqs, offs)
    info = g.jump_info()
    assert g.jump_index() is None
    assert info["jump_entries"] == 0 and info["jump_bytes"] == 0 and info["jump_absent"] == 5 and "interior" in info["jump_absent_why"]
    # the blob a caller sees is the same bytes with the index built, not built, and compiled out of the build: the index lies behind it
    c1 = B.Graph.build(K, *pack(COMPACTED))
    assert c1.jump_index() is not None and J.header_fields(c1.blob())["jump_buckets"] == 0
    B.set_option("build_jump", 0)
    g0, c0 = B.Graph.build(K, seqs, offs), B.Graph.build(K, *pack(COMPACTED))
    assert bytes(g.blob()) == bytes(g0.blob()) and bytes(c1.blob()) == bytes(c0.blob())
    assert c0.jump_index() is None and c0.jump_info()["jump_absent"] == 5
    B.set_option("build_jump", 1)
    # exception bases, two-word keys: no index, and the reason
    ge = B.Graph.build(K, *pack([A1, B1, "CCCTGANAAGTTTC"]))
    assert ge.jump_info()["jump_absent"] == 2 and ge.jump_index() is None
    B.set_option("test.wide_keys", 1)
    gw = B.Graph.build(K, *pack(COMPACTED))
    assert gw.jump_info()["jump_absent"] == 1 and gw.jump_index() is None


def test_header_check_rejects_a_section_outside_the_blob(options):
    g = B.Graph.build(12, *pack([rnd(300, 1), rnd(41, 2), rnd(12, 3)]))
    good = J.blob_with_index(g)
    g2 = B.Graph.from_blob(good)
    assert g2.jump_info()["jump_entries"] == g.jump_info()["jump_entries"] and g2.jump_info()["jump_absent"] == 0
    h = J.header_fields(good)

    def with_u64(off, v):
        b = good.copy()
        b[off:off + 8] = np.frombuffer(np.uint64(v).tobytes(), dtype=np.uint8)
        return b

    for bad in (with_u64(J.OFF_OFF_JUMP, h["blob_bytes"]),                      # starts at the blob's end
                with_u64(J.OFF_OFF_JUMP, h["off_jump"] + 256),                  # ends behind it
                with_u64(J.OFF_OFF_JUMP, h["off_jump"] + 8),                    # not aligned
                with_u64(J.OFF_OFF_JUMP, 0),                                    # inside the header
                with_u64(J.OFF_JUMP_BUCKETS, h["jump_buckets"] + 16),           # more buckets than fit
                with_u64(J.OFF_JUMP_BUCKETS, (1 << 64) - 1),                    # count * size overflows
                with_u64(J.OFF_JUMP_BUCKETS, 0)):                               # no buckets, but an offset
        with pytest.raises(B.BgrError):
            B.Graph.from_blob(bad)
