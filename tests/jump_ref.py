"""Plain-Python reference of the jump index of the greedy anchor scan (bgreat_amd/csrc/graph_layout.h): property P, the sampled
(k-1)-mers, the entries and their buckets, and readers of a built graph's index.  Slow and obvious on purpose; k <= 32."""
import struct

M64 = (1 << 64) - 1
STRIDE = 4
FWD_CANON = 0x40000000
MAX_T = 0x00FFFFFF
CAP_BYTES = 64 << 20
# byte offsets of the header's jump fields (behind anc_levels) and of the fields the tests corrupt
OFF_BLOB_BYTES, OFF_OFF_JUMP, OFF_JUMP_ENTRIES, OFF_JUMP_BUCKETS, OFF_JUMP_STRIDE, OFF_JUMP_DROPPED = 16, 1096, 1104, 1112, 1120, 1124
CODE = {"A": 0, "C": 1, "G": 2}


def kint(s):  # str2num: A0 C1 G2, anything else 3
    x = 0
    for c in s:
        x = x << 2 | CODE.get(c, 3)
    return x


def rcb(x, n):
    r = 0
    for _ in range(n):
        r = r << 2 | (3 - (x & 3))
        x >>= 2
    return r


def mix64(x):
    x ^= x >> 32
    return (x * 0x9E3779B97F4A7C15) & M64


def tag_of(m):
    return ((m >> 32) & 0xFF) or 1


def bucket_of(m, n_buckets):
    return ((m & 0xFFFFFFFF) * n_buckets) >> 32


def split(seqs, offs):
    s = bytes(seqs).decode()
    return [s[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def overlap_keys(k, unitigs):
    keys = set()
    for u in unitigs:
        for w in (u[:k - 1], u[len(u) - (k - 1):]):
            x = kint(w)
            keys.add(min(x, rcb(x, k - 1)))
    return keys


def property_p(k, unitigs):
    """No (k-1)-mer at an interior offset 0 < t < len - (k-1) of a unitig is an overlap key (canonical form: either strand)."""
    K1, keys = k - 1, overlap_keys(k, unitigs)
    for u in unitigs:
        for t in range(1, len(u) - K1):
            x = kint(u[t:t + K1])
            if min(x, rcb(x, K1)) in keys:
                return False
    return True


def selects(m, stride=STRIDE):
    return ((m >> 40) & (stride - 1)) == 0


def sampled(k, unitigs, stride=STRIDE):
    """(canonical key, unitig id from 1, offset t, forward window is canonical) of the (k-1)-mers whose hash selects them (one in `stride`),
    palindromes left out, in unitig order."""
    K1, out = k - 1, []
    for i, u in enumerate(unitigs):
        for t in range(0, len(u) - K1 + 1):
            if t > MAX_T:
                break
            x = kint(u[t:t + K1])
            r = rcb(x, K1)
            if x != r and selects(mix64(min(x, r)), stride):
                out.append((min(x, r), i + 1, t, x < r))
    return out


def n_buckets(k, unitigs, stride=STRIDE):
    return (sum(len(u) - (k - 1) + 1 for u in unitigs) + stride - 1) // stride


def table(k, unitigs, stride=STRIDE):
    """bucket -> [(idc, t_tag), ...]: at most two per bucket, first come first served."""
    nb, tab = n_buckets(k, unitigs, stride), {}
    for key, uid, t, fc in sampled(k, unitigs, stride):
        m = mix64(key)
        b = tab.setdefault(bucket_of(m, nb), [])
        if len(b) < 2:
            b.append((uid | (FWD_CANON if fc else 0), t << 8 | tag_of(m)))
    return tab


def header_fields(blob):
    b = bytes(blob[:4096])
    off, ent, nb = struct.unpack_from("<QQQ", b, OFF_OFF_JUMP)
    stride, dropped = struct.unpack_from("<II", b, OFF_JUMP_STRIDE)
    return {"off_jump": off, "jump_entries": ent, "jump_buckets": nb, "jump_stride": stride, "jump_dropped_x1000": dropped,
            "blob_bytes": struct.unpack_from("<Q", b, OFF_BLOB_BYTES)[0]}


def graph_table(graph):
    """The jump index of a built graph (Graph.jump_index(): uint32[buckets, 4]) in table()'s form, empty entries left out; {} when it has none."""
    t = graph.jump_index()
    tab = {}
    if t is None:
        return tab
    for b in range(t.shape[0]):
        ents = [(int(t[b, j]), int(t[b, j + 1])) for j in (0, 2) if t[b, j + 1]]
        if ents:
            tab[b] = ents
    return tab


def blob_with_index(graph):
    """A blob that carries the graph's jump index as a section of its own, named by the header: the blob, the section behind it (256-byte
    aligned), the header's four fields and blob_bytes set -- what a device copy holds, and what bgr_graph_from_blob accepts."""
    import numpy as np
    blob = np.array(graph.blob(), dtype=np.uint8, copy=True)
    t = graph.jump_index()
    info = graph.jump_info()
    off = (len(blob) + 255) & ~255
    out = np.zeros(off + t.size * 4, dtype=np.uint8)
    out[:len(blob)] = blob
    out[off:] = t.reshape(-1).view(np.uint8)
    struct.pack_into("<QQQII", out, OFF_OFF_JUMP, off, info["jump_entries"], t.shape[0], info["jump_stride"], info["jump_dropped_x1000"])
    struct.pack_into("<Q", out, OFF_BLOB_BYTES, len(out))
    return out
