"""Haplotags (`--haplotag`, bgr_read_tag, bgr_blocks_tag_table, bgr_read_blocks_tags, bgr_aligner_haplotags, the PS / HP fields of a GAF line) in
plain Python: the checker of the product's tables, tags and line suffixes.  Written from the definition in include/bgreat_gpu.h over bubbles_ref's
records and blocks_ref's entries, not from bgreat_amd/.

The table has n_unitigs + 1 entries, table[0] == 0; table[u] = block << 1 | hap (hap 0 = the branch on haplotype A) or 0.  A row is the path as
the batch API returns it: [off, id_1 .. id_n] or [] for an unmapped read.  A tag is (block, a, b, others)."""
import blocks_ref


class Refused(ValueError):
    """what the library answers with BGR_E_ARG"""


def _put(table, unitig, tag, where):
    if not 1 <= unitig < len(table):
        raise Refused("%s: unitig %d is not one of 1 .. %d" % (where, unitig, len(table) - 1))
    if table[unitig] not in (0, tag):
        raise Refused("%s: unitig %d would receive two tags" % (where, unitig))
    table[unitig] = tag


def _pair(table, block, a, b, where):
    if not 1 <= block < 2 ** 31:
        raise Refused("%s: block %d" % (where, block))
    if abs(a) == abs(b):
        raise Refused("%s: one unitig on both haplotypes" % where)
    _put(table, abs(a), block << 1, where)
    _put(table, abs(b), block << 1 | 1, where)


def table_of(bubbles, entries, n_unitigs, min_block=1):
    """the table from the structs: bubbles as bubbles_ref has them (s, t, (b0, b1), counts), entries as blocks_ref (block, index, size, bubble, flags)"""
    table = [0] * (n_unitigs + 1)
    for i, (block, _, size, bubble, flags) in enumerate(entries):
        if size < min_block:
            continue
        if not 0 <= bubble < len(bubbles):
            raise Refused("entry %d names no bubble" % i)
        br = bubbles[bubble][2]
        h = (flags >> 1) & 1
        _pair(table, block, br[h], br[1 - h], "entry %d" % i)
    return table


def _dec(field, where):
    """a decimal integer as the parser reads it: an optional '-', then digits only"""
    digits = field[1:] if field.startswith(b"-") else field
    if not digits or not digits.isdigit():
        raise Refused("%s: %r is no decimal integer" % (where, field))
    return int(field)


def table_of_file(data, n_unitigs):
    """the table from the bytes of a --blocks file; every block of the file tags"""
    header = blocks_ref.HEADER.encode("latin-1")
    if not data.startswith(header):
        raise Refused("line 1: not the header of a blocks file")
    table = [0] * (n_unitigs + 1)
    rest = data[len(header):]
    lines = rest.split(b"\n")
    if lines and lines[-1] == b"":   # (the last line may or may not end with a newline)
        lines.pop()
    for n, line in enumerate(lines, 2):
        f = line.split(b"\t")
        where = "line %d" % n
        if len(f) != 10:
            raise Refused("%s: %d fields" % (where, len(f)))
        block, a, b = _dec(f[0], where), _dec(f[6], where), _dec(f[7], where)
        if abs(a) > 2 ** 31 or abs(b) > 2 ** 31:
            raise Refused("%s: an id beyond the graph" % where)
        _pair(table, block, a, b, where)
    return table


def n_tagged(table):
    return sum(1 for x in table if x)


def tag_of(table, row):
    """-> (block, a, b, others) of one row"""
    votes = [table[abs(x)] for x in row[1:] if 1 <= abs(x) < len(table) and table[abs(x)]]
    if not votes:
        return (0, 0, 0, 0)
    block = min(v >> 1 for v in votes)
    a = sum(1 for v in votes if v == block << 1)
    b = sum(1 for v in votes if v == block << 1 | 1)
    return (block, a, b, len(votes) - a - b)


def suffix_of(tag):
    """what a GAF line gains in front of its newline"""
    block, a, b, others = tag
    if not block:
        return ""
    return "\tPS:i:%d\tHP:i:%d\tha:i:%d\thb:i:%d\tho:i:%d" % (block, 1 if a > b else 2 if b > a else 0, a, b, others)


def tagged_line(line, tag):
    assert line.endswith("\n")
    return line[:-1] + suffix_of(tag) + "\n"
