"""The view through which the readers of greedy rows read the rows of exhaustive mode (bgr_aligner_exhaustive_paths_enable, include/bgreat_gpu.h), in
plain Python: the checker of bgr_exhaustive_rows_kernel and of everything that is counted or formatted behind an exhaustive launch.  Written from the
reference's row layout (alignerExhaustive.cpp:96-104, 193-201, 249-257), not from bgreat_amd/.

A row of exhaustive mode is [begin offset, +-u_1 .. +-u_n, end offset]: a row of the greedy modes with one more int behind it -- |readLeft| + k - 1 in
the last unitig, or 0 when the read ends with the anchor.  Rows are (status, path ints) as the batch API returns them (wide_greedy_ref.rows_of)."""
from wide_greedy_ref import ST_ALIGNED

ST_MASK = 3


def view_word(off, w, arena_ints):
    """one entry of the view from one result pair {off, w}: -> (off, w')"""
    n, st = w & 0xFFFFFF, w >> 24
    if (st & ST_MASK) == ST_ALIGNED and n >= 3 and off + n <= arena_ints:
        return off, (n - 1) | (st << 24)
    return off, st << 24


def view_row(status, path):
    """the same on a row that lies in the arena: the row without its end offset, or an empty row -- the status as stored either way"""
    if (status & ST_MASK) == ST_ALIGNED and len(path) >= 3:
        return status, list(path[:-1])
    return status, []


def view_rows(rows):
    return [view_row(st, p) for st, p in rows]


def end_offsets(unitigs, k, L, path):
    """the int the view drops, from what it keeps: path = [begin, ids ..] of a read of L characters -> the values it can have.  Where the read ends in
    the last unitig: e = begin + L - (walk length - last unitig's length); a read that ends with the last unitig's last character has e = that
    unitig's length, and alignerExhaustive.cpp writes e there or -- the search ended on the anchor -- 0: one position, spelled two ways"""
    lens = [len(unitigs[abs(x)]) for x in path[1:]]
    walk_len = sum(lens) - (k - 1) * (len(lens) - 1)
    e = path[0] + L - (walk_len - lens[-1])
    return {e, 0} if e == lens[-1] else {e}
