"""haplotag_ref.py, the definition of haplotags in plain Python, checked on cases small enough to do by hand; the library's two table builders
(bgr_blocks_tag_table, bgr_read_blocks_tags) against it on blocks_gen's crafted lists, the round trip through bgr_write_blocks, and every refusal.
CPU only: the builders are host code."""
import random

import numpy as np
import pytest

import bgreat_amd as B
import blocks_gen as G
import blocks_ref as BR
import haplotag_ref as H
from test_wide_k_host import pack

ONES = (1, 1, 1, 1)
BUBBLES = [(1, 4, (2, 3), ONES), (4, 7, (5, 6), ONES)]
HEADER = BR.HEADER.encode()


def entries_array(entries):
    a = np.zeros(len(entries), dtype=B.BLOCK_DTYPE)
    for i, e in enumerate(entries):
        a[i] = tuple(e) + (0,)
    return a


def test_two_bubbles_cis_and_trans():
    cis = [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0)]
    assert H.table_of(BUBBLES, cis, 7) == [0, 0, 2, 3, 0, 2, 3, 0]   # 2 and 5 on A of block 1, 3 and 6 on B
    trans = [(1, 0, 2, 0, 0), (1, 1, 2, 1, BR.HAP)]
    t = H.table_of(BUBBLES, trans, 7)
    assert t == [0, 0, 2, 3, 0, 3, 2, 0] and H.n_tagged(t) == 4
    # a read along haplotype A of the trans block crosses 2 and 6, in either strand; one that crosses 2 and 5 switches haplotypes
    assert H.tag_of(t, [0, 1, 2, 4, 6, 7]) == (1, 2, 0, 0) == H.tag_of(t, [3, -7, -6, -4, -2, -1])
    assert H.tag_of(t, [0, 1, 3, 4, 5, 7]) == (1, 0, 2, 0) and H.tag_of(t, [0, 1, 2, 4, 5]) == (1, 1, 1, 0)
    assert H.tag_of(t, [5, 1, 4, 7]) == (0, 0, 0, 0) == H.tag_of(t, []) == H.tag_of(t, [0, 0, 8, -8, -2 ** 31])
    # the reversed reading and the ring flags do not matter
    assert H.table_of(BUBBLES, [(1, 0, 2, 1, BR.REVERSED | BR.CIRCULAR), (1, 1, 2, 0, BR.REVERSED | BR.CONFLICT | BR.HAP)], 7) == [0, 0, 3, 2, 0, 2, 3, 0]


def test_a_block_of_one_and_min_block():
    entries = [(1, 0, 1, 0, 0), (2, 0, 1, 1, 0)]
    t = H.table_of(BUBBLES, entries, 9)
    assert t == [0, 0, 2, 3, 0, 4, 5, 0, 0, 0]
    assert H.tag_of(t, [0, 1, 2, 4, 5, 7]) == (1, 1, 0, 1) and H.tag_of(t, [0, 4, 6]) == (2, 0, 1, 0)   # the smallest block; the other one's vote in `others`
    assert H.table_of(BUBBLES, entries, 9, min_block=2) == [0] * 10
    mixed = [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0), (2, 0, 1, 2, 0)]
    bubbles = BUBBLES + [(10, 13, (11, 12), ONES)]
    assert H.table_of(bubbles, mixed, 13, min_block=2) == [0, 0, 2, 3, 0, 2, 3] + [0] * 7
    assert H.table_of(bubbles, mixed, 13)[11:13] == [4, 5]


def test_suffix():
    assert H.suffix_of((0, 0, 0, 0)) == ""
    assert H.suffix_of((3, 2, 0, 1)) == "\tPS:i:3\tHP:i:1\tha:i:2\thb:i:0\tho:i:1"
    assert H.suffix_of((2 ** 31 - 1, 0, 12, 0)) == "\tPS:i:2147483647\tHP:i:2\tha:i:0\thb:i:12\tho:i:0"
    assert H.suffix_of((1, 4, 4, 0)).startswith("\tPS:i:1\tHP:i:0\t")
    assert H.tagged_line("r\t1\tNM:i:0\n", (1, 1, 0, 0)) == "r\t1\tNM:i:0\tPS:i:1\tHP:i:1\tha:i:1\thb:i:0\tho:i:0\n" and H.tagged_line("x\n", (0, 0, 0, 0)) == "x\n"


def test_file_form_by_hand():
    text = BR.blocks_text(BUBBLES, [(1, 0, 2, 0, 0), (1, 1, 2, 1, BR.HAP | BR.REVERSED)])
    assert text.endswith(b"1\t1\t2\t2\t-7\t-4\t-6\t-5\t-\t.\n")
    assert H.table_of_file(text, 7) == [0, 0, 2, 3, 0, 3, 2, 0] == H.table_of_file(text[:-1], 7)   # (the last newline may be missing)
    assert H.table_of_file(HEADER, 3) == [0, 0, 0, 0]


CRAFTED = [([("path", 1)], 1), ([("path", 5), ("ring", 3), ("path", 1), ("ring", 2)], 2), ([("path", 40), ("ring", 17), ("path", 2), ("path", 1), ("path", 1)], 3)]


@pytest.mark.parametrize("shapes,seed", CRAFTED, ids=["one", "mixed", "long"])
def test_the_builders_against_the_reference_and_the_round_trip(shapes, seed, tmp_path):
    bubbles, phase, n_unitigs = G.make(shapes, seed, undecided=0.2, spare=3)
    entries = BR.blocks_of(bubbles, phase)
    ba, ea = G.bubbles_array(B, bubbles), entries_array(entries)
    for min_block in (1, 2, 3, 100):
        want = H.table_of(bubbles, entries, n_unitigs, min_block)
        table, n = B.blocks_tag_table(ba, ea, n_unitigs, min_block)
        assert table.tolist() == want and n == H.n_tagged(want)
    assert H.n_tagged(H.table_of(bubbles, entries, n_unitigs)) == 2 * len(bubbles)
    # bgr_write_blocks, then bgr_read_blocks_tags: the table of min_block 1 (the writer wants a graph that has the unitigs)
    rng = random.Random(seed)
    g = B.Graph.build(9, *pack(["".join(rng.choice("ACGT") for _ in range(12)) for _ in range(n_unitigs)]))
    path = str(tmp_path / "blocks.tsv")
    B.write_blocks(path, g, ba, ea)
    data = open(path, "rb").read()
    assert data == BR.blocks_text(bubbles, entries)
    table, n = B.read_blocks_tags(path, n_unitigs)
    assert table.tolist() == H.table_of(bubbles, entries, n_unitigs) == H.table_of_file(data, n_unitigs) and n == 2 * len(bubbles)


def line(block, a, b, fields=None):
    f = fields or [str(block), "0", "1", "1", "1", "4", str(a), str(b), "+", "."]
    return ("\t".join(f) + "\n").encode()


REFUSED_FILES = {
    "id 0": HEADER + line(1, 0, 3),
    "id beyond": HEADER + line(1, 2, 8),
    "negative id beyond": HEADER + line(1, -8, 2),
    "block 0": HEADER + line(0, 2, 3),
    "block 2^31": HEADER + line(2 ** 31, 2, 3),
    "negative block": HEADER + line(-1, 2, 3),
    "same unitig": HEADER + line(1, 2, -2),
    "two tags": HEADER + line(1, 2, 3) + line(2, 5, 2),
    "two haplotypes": HEADER + line(1, 2, 3) + line(1, 3, 5),
    "no header": line(1, 2, 3),
    "empty": b"",
    "header without newline": HEADER[:-1],
    "another header": HEADER.replace(b"hapA", b"hapa") + line(1, 2, 3),
    "nine fields": HEADER + line(0, 0, 0, ["1", "0", "1", "1", "1", "4", "2", "3", "+"]),
    "eleven fields": HEADER + line(0, 0, 0, ["1", "0", "1", "1", "1", "4", "2", "3", "+", ".", "x"]),
    "empty line": HEADER + line(1, 2, 3) + b"\n" + line(1, 5, 6),
    "truncated line": HEADER + line(1, 2, 3) + line(1, 5, 6)[:9],
    "block not a number": HEADER + line("1x", 2, 3),
    "hapA with a plus": HEADER + line(1, "+2", 3),
    "hapB empty": HEADER + line(1, 2, ""),
    "hapB a minus alone": HEADER + line(1, 2, "-"),
    "hapA with a space": HEADER + line(1, " 2", 3),
    "overlong block": HEADER + line("1" * 40, 2, 3),
    "overlong id": HEADER + line(1, "9" * 30, 3),
}


@pytest.mark.parametrize("name", sorted(REFUSED_FILES))
def test_file_refusals(name, tmp_path):
    data = REFUSED_FILES[name]
    with pytest.raises(H.Refused):
        H.table_of_file(data, 7)
    path = tmp_path / "bad.tsv"
    path.write_bytes(data)
    with pytest.raises(B.BgrError, match="error -1") as e:
        B.read_blocks_tags(path, 7)
    first_bad = 1 if not data.startswith(HEADER) else 2 + (name in ("two tags", "two haplotypes", "empty line", "truncated line")) * 1
    assert "line %d" % first_bad in str(e.value), str(e.value)


def test_accepted_files_and_io(tmp_path):
    ok = HEADER + line(1, 2, 3) + line(1, -6, 5) + line(1, 2, 3) + line(7, 1, 7)[:-1]   # a repeated line gives the same tags; other fields may hold anything
    ok = ok.replace(b"\t+\t.\n", b"\tanything\t\n", 1)
    path = tmp_path / "ok.tsv"
    path.write_bytes(ok)
    table, n = B.read_blocks_tags(path, 7)
    assert table.tolist() == H.table_of_file(ok, 7) == [0, 14, 2, 3, 0, 3, 2, 15] and n == 6
    path.write_bytes(HEADER)
    table, n = B.read_blocks_tags(path, 7)
    assert not table.any() and n == 0
    with pytest.raises(B.BgrError, match="cannot open"):
        B.read_blocks_tags(tmp_path / "missing.tsv", 7)


def test_struct_refusals():
    ba = G.bubbles_array(B, BUBBLES)

    def refused(bubbles, entries, n_unitigs, word, min_block=1):
        with pytest.raises(H.Refused):
            H.table_of(bubbles, entries, n_unitigs, min_block)
        with pytest.raises(B.BgrError, match="error -1") as e:
            B.blocks_tag_table(G.bubbles_array(B, bubbles), entries_array(entries), n_unitigs, min_block)
        assert word in str(e.value), str(e.value)

    good = [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0)]
    assert B.blocks_tag_table(ba, entries_array(good), 7)[0].tolist() == H.table_of(BUBBLES, good, 7)
    refused(BUBBLES, good, 5, "entry 1")                                        # 6 is beyond n_unitigs
    refused([(1, 4, (0, 3), ONES)], [(1, 0, 1, 0, 0)], 7, "entry 0")            # id 0
    refused([(1, 4, (2, -2 ** 31), ONES)], [(1, 0, 1, 0, 0)], 7, "entry 0")     # INT32_MIN is merely beyond the graph
    refused(BUBBLES, [(0, 0, 2, 0, 0)], 7, "block 0")
    refused(BUBBLES, [(2 ** 31, 0, 2, 0, 0)], 7, "block")
    refused([(1, 4, (2, -2), ONES)], [(1, 0, 1, 0, 0)], 7, "both haplotypes")
    refused(BUBBLES + [(7, 9, (2, 8), ONES)], good + [(2, 0, 1, 2, 0)], 9, "two different tags")
    refused(BUBBLES, [(1, 0, 2, 2, 0)], 7, "no bubble")
    # a block below min_block is not looked at, whatever it names
    assert B.blocks_tag_table(ba, entries_array([(1, 0, 1, 9, 0)]), 7, 2)[0].tolist() == [0] * 8 == H.table_of(BUBBLES, [(1, 0, 1, 9, 0)], 7, 2)
    assert B.blocks_tag_table(np.zeros(0, dtype=B.BUBBLE_DTYPE), np.zeros(0, dtype=B.BLOCK_DTYPE), 0)[0].tolist() == [0]


def test_symbols_and_struct():
    assert B.READ_TAG_DTYPE.itemsize == 16
    for name in ("bgr_blocks_tag_table", "bgr_read_blocks_tags", "bgr_aligner_haplotag_enable", "bgr_aligner_haplotags", "bgr_graph_haplotag_enable", "bgr_graph_haplotag_enabled"):
        assert name in B.SYMBOLS and hasattr(B.lib(), name)
