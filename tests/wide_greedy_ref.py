"""An independent restatement of the reference's greedy path (BGREAT: aligner.cpp, alignerGreedy.cpp, utils.cpp) over Python ints,
so that its k-mer arithmetic holds for any k: `kmer` is an unsigned integer of 2(k-1) bits here, not the reference's uint64_t.  Written
from the reference alone (not from bgreat_amd/), it is the yardstick of graphs with 32 < k <= 64, which the reference cannot load.

Reads and unitigs are Python str.  align() returns rows (status, path ints) with status = BGR_ST_* (include/bgreat_gpu.h)."""

ST_NOANCHOR, ST_FAILED, ST_ALIGNED, ST_RC = 0, 1, 2, 4
_RC = {"A": "T", "C": "G", "G": "C"}


def reverse_complements(s):  # utils.cpp:52-73 (revCompChar: anything but A/C/G -> 'A')
    return "".join(_RC.get(c, "A") for c in reversed(s))


def str2num(s):  # utils.cpp:117-129 (anything but A/C/G -> 3)
    res = 0
    for c in s:
        res = (res << 2) + (0 if c == "A" else 1 if c == "C" else 2 if c == "G" else 3)
    return res


def nuc2int(c):  # utils.cpp:132-140 (anything but C/G/T -> 0)
    return 1 if c == "C" else 2 if c == "G" else 3 if c == "T" else 0


def nuc2intrc(c):  # utils.cpp:143-151 (anything but A/C/G -> 0)
    return 3 if c == "A" else 2 if c == "C" else 1 if c == "G" else 0


def rcb(x, n):  # utils.cpp:182-192
    res, offset = 0, 1 << (2 * n - 2)
    for _ in range(n):
        res += (3 - (x % 4)) * offset
        x >>= 2
        offset >>= 2
    return res


def missmatch_number(seq1, seq2, n):  # utils.cpp:154-168 (seq1 may be shorter: a position past its end never equals)
    miss = 0
    for i, c in enumerate(seq2):
        if i >= len(seq1) or c != seq1[i]:
            miss += 1
            if miss > n:
                return miss
    return miss


def compaction_end(seq1, seq2, k):  # utils.cpp:171-179
    if not seq1 or not seq2:
        return ""
    rc2, end1 = reverse_complements(seq2), seq1[len(seq1) - k:]
    if end1 == seq2[:k]:
        return seq1 + seq2[k:]
    if end1 == rc2[:k]:
        return seq1 + rc2[k:]
    return ""


class GreedyRef:
    def __init__(self, k, unitigs):
        self.k = k
        self.K1 = k - 1
        self.offset_update = 1 << (2 * (k - 1))  # aligner.h:101-102
        self.unitigs = [""]
        for u in unitigs:  # aligner.cpp:415-420: loading stops at the first sequence shorter than k
            if len(u) < k:
                break
            self.unitigs.append(u)
        # aligner.cpp:466-533: leftIndices / rightIndices, filled in unitig order, first free of indice1..3, else indice4 is overwritten
        self.left, self.right = {}, {}
        K1 = self.K1
        for i in range(1, len(self.unitigs)):
            line = self.unitigs[i]
            beg = str2num(line[:K1])
            rc_beg = rcb(beg, K1)
            if beg <= rc_beg:
                self._fill(self.left, beg, i)
            else:
                self._fill(self.right, rc_beg, i)
            end = str2num(line[len(line) - K1:])
            rc_end = rcb(end, K1)
            if end <= rc_end:
                self._fill(self.right, end, i)
            else:
                self._fill(self.left, rc_end, i)

    @staticmethod
    def _fill(table, key, i):  # aligner.cpp:481-489
        ind = table.setdefault(key, [0, 0, 0, 0])
        for j in range(3):
            if ind[j] == 0:
                ind[j] = i
                return
        ind[3] = i

    def is_overlap(self, rep):  # aligner.cpp:353-366: a member of the left or of the right key set
        return rep in self.left or rep in self.right

    def canonical_keys(self):
        return set(self.left) | set(self.right)

    def _oriented(self, ind, bin_, prefix):  # aligner.cpp:171-203 / 233-264: the nested ifs stop at the first empty indice
        out = []
        for u in ind:
            if u == 0:
                break
            s = self.unitigs[u]
            part = s[:self.K1] if prefix else s[len(s) - self.K1:]
            if str2num(part) == bin_:
                out.append((s, u))
            else:
                out.append((reverse_complements(s), -u))
        return out

    def get_end(self, bin_):  # aligner.cpp:147-206
        rc = rcb(bin_, self.K1)
        ind = self.right.get(bin_) if bin_ <= rc else self.left.get(rc)
        return self._oriented(ind, bin_, False) if ind else []

    def get_begin(self, bin_):  # aligner.cpp:209-267
        rc = rcb(bin_, self.K1)
        ind = self.left.get(bin_) if bin_ <= rc else self.right.get(rc)
        return self._oriented(ind, bin_, True) if ind else []

    def update(self, x, c):  # aligner.cpp:305-309
        return ((x << 2) + nuc2int(c)) % self.offset_update

    def update_rc(self, x, c):  # aligner.cpp:312-315
        return (x >> 2) + (nuc2intrc(c) << (2 * self.k - 4))

    def get_n_overlap(self, read, n):  # aligner.cpp:345-378
        k, K1 = self.k, self.K1
        # (a read shorter than k-1 has no window: the reference looks its shorter number up at position 0, and a hit there could only
        # end in checkEndGreedy's substr past the read's end, alignerGreedy.cpp:323 -- std::out_of_range; such a read has no anchor here)
        if len(read) < K1:
            return []
        out = []
        num = str2num(read[:K1])
        rcnum = rcb(num, K1)
        rep = min(num, rcnum)
        i = 0
        while True:
            if self.is_overlap(rep):
                out.append((num, i))
            if len(out) >= n:
                return out
            if i + k - 1 < len(read):
                num = self.update(num, read[i + k - 1])
                rcnum = self.update_rc(rcnum, read[i + k - 1])
                rep = min(num, rcnum)
            else:
                return out
            i += 1

    # ---- the walks (alignerGreedy.cpp:167-364) ----------------------------------------------------------------------------
    def map_on_left_end(self, read, path, ov, errors):  # alignerGreedy.cpp:167-218
        k = self.k
        if ov[1] == 0:
            path.append(0)
            return 0
        read_left = read[:ov[1]]
        rng = self.get_end(ov[0])
        mini, mini_i, ended, offset, next_u, next_ov = errors + 1, 9, False, 0, "", 0
        for i, (u, sid) in enumerate(rng):
            if len(u) - k + 1 >= len(read_left):
                miss = missmatch_number(u[len(u) - len(read_left) - k + 1:][:len(read_left)], read_left, errors)
                if miss == 0:
                    path.append(sid)
                    path.append(len(u) - len(read_left) - k + 1)
                    return 0
                if miss < mini:
                    mini, mini_i, ended, offset = miss, i, True, len(u) - len(read_left) - k + 1
            else:
                miss = missmatch_number(u[:len(u) - k + 1], read_left[len(read_left) - (len(u) - k + 1):], errors)
                if miss == 0:
                    path.append(sid)
                    return self.map_on_left_end(read, path, (str2num(u[:k - 1]), ov[1] - (len(u) - k + 1)), errors)
                if miss < mini:
                    ended, mini, mini_i, next_u, next_ov = False, miss, i, u, str2num(u[:k - 1])
        if mini <= errors:
            path.append(rng[mini_i][1])
            if ended:
                path.append(offset)
                return mini
            return mini + self.map_on_left_end(read, path, (next_ov, ov[1] - (len(next_u) - k + 1)), errors - mini)
        return mini

    def map_on_right_end(self, read, path, ov, errors):  # alignerGreedy.cpp:221-265
        k = self.k
        read_left = read[ov[1]:]
        if len(read_left) < k:
            return 0
        rng = self.get_begin(ov[0])
        mini, mini_i, ended, next_u, next_ov = errors + 1, 9, False, "", 0
        for i, (u, sid) in enumerate(rng):
            if len(u) - k + 1 >= len(read_left):
                miss = missmatch_number(u[:len(read_left)], read_left, errors)
                if miss == 0:
                    path.append(sid)
                    return 0
                if miss < mini:
                    mini, mini_i, ended = miss, i, True
            else:
                miss = missmatch_number(u, read[ov[1]:ov[1] + len(u)], errors)
                if miss == 0:
                    path.append(sid)
                    return self.map_on_right_end(read, path, (str2num(u[len(u) - k + 1:]), ov[1] + (len(u) - k + 1)), errors)
                if miss < mini:
                    ended, mini, mini_i, next_u, next_ov = False, miss, i, u, str2num(u[len(u) - k + 1:])
        if mini <= errors:
            path.append(rng[mini_i][1])
            if ended:
                return mini
            return mini + self.map_on_right_end(read, path, (next_ov, ov[1] + (len(next_u) - k + 1)), errors - mini)
        return mini

    def check_begin(self, read, ov, path, errors):  # alignerGreedy.cpp:268-319
        k = self.k
        if ov[1] == 0:
            path.append(0)
            return 0
        read_left = read[:ov[1]]
        rng = self.get_end(ov[0])
        mini, mini_i, ended, offset, next_u, next_ov = errors + 1, 9, False, 0, "", 0
        for i, (u, sid) in enumerate(rng):
            if len(u) - k + 1 >= len(read_left):
                miss = missmatch_number(u[len(u) - len(read_left) - k + 1:][:len(read_left)], read_left, errors)
                if miss == 0:
                    path.append(sid)
                    path.append(len(u) - len(read_left) - k + 1)
                    return 0
                if miss < mini:
                    mini, mini_i, ended, offset = miss, i, True, len(u) - len(read_left) - k + 1
            else:
                miss = missmatch_number(u[:len(u) - k + 1], read_left[len(read_left) + k - 1 - len(u):], errors)
                if miss == 0:
                    path.append(sid)
                    return self.map_on_left_end(read, path, (str2num(u[:k - 1]), ov[1] - (len(u) - k + 1)), errors)
                if miss < mini:
                    ended, mini, mini_i, next_u, next_ov = False, miss, i, u, str2num(u[:k - 1])
        if mini <= errors:
            path.append(rng[mini_i][1])
            if ended:
                path.append(offset)
                return mini
            return mini + self.map_on_left_end(read, path, (next_ov, ov[1] - (len(next_u) - k + 1)), errors - mini)
        return mini

    def check_end(self, read, ov, path, errors):  # alignerGreedy.cpp:322-364
        k = self.k
        read_left = read[ov[1] + k - 1:]
        if not read_left:
            return 0
        rng = self.get_begin(ov[0])
        mini, mini_i, ended, next_u, next_ov = errors + 1, 9, False, "", 0
        for i, (u, sid) in enumerate(rng):
            if len(u) - k + 1 >= len(read_left):
                miss = missmatch_number(u[k - 1:k - 1 + len(read_left)], read_left, errors)
                if miss == 0:
                    path.append(sid)
                    return 0
                if miss < mini:
                    mini, mini_i, ended = miss, i, True
            else:
                miss = missmatch_number(u[k - 1:], read_left[:len(u) - k + 1], errors)
                if miss == 0:
                    path.append(sid)
                    return self.map_on_right_end(read, path, (str2num(u[len(u) - k + 1:]), ov[1] + (len(u) - k + 1)), errors)
                if miss < mini:
                    mini, mini_i, next_ov, next_u, ended = miss, i, str2num(u[len(u) - k + 1:]), u, False
        if mini <= errors:
            path.append(rng[mini_i][1])
            if ended:
                return mini
            return mini + self.map_on_right_end(read, path, (next_ov, ov[1] + (len(next_u) - k + 1)), errors - mini)
        return mini

    def align_read(self, read, errors, effort):  # alignerGreedy.cpp:35-57 -> (status, path); its retry ladder written as a loop
        rc = False
        while True:
            overlaps = self.get_n_overlap(read, effort)
            if not overlaps:
                return (ST_NOANCHOR | (ST_RC if rc else 0)), []
            for ov in overlaps:
                begin = []
                e_begin = self.check_begin(read, ov, begin, errors)
                if e_begin <= errors:
                    end = []
                    e_end = self.check_end(read, ov, end, errors - e_begin)
                    if e_end + e_begin <= errors:
                        return (ST_ALIGNED | (ST_RC if rc else 0)), begin[::-1] + end
            if rc:
                return ST_FAILED | ST_RC, []
            rc = True
            read = reverse_complements(read)

    def get_unitig(self, position):  # aligner.cpp:293-301
        return self.unitigs[position] if position > 0 else reverse_complements(self.unitigs[-position])

    def recover_path(self, numbers, size):  # aligner.cpp:270-290 (None: "bug compaction")
        path = self.get_unitig(numbers[1])
        for x in numbers[2:]:
            inter = compaction_end(path, self.get_unitig(x), self.k - 1)
            if not inter:
                return None
            path = inter
        return path[numbers[0]:numbers[0] + size]

    def corrected(self, read, status, path):  # alignerGreedy.cpp:394-400
        c = self.recover_path(path, len(read))
        return reverse_complements(c) if status & ST_RC else c

    def align(self, reads, m, effort):
        """-> rows [(status, path)] and the aligner.h:68 counters (reads, no overlap, aligned, not aligned)."""
        rows = [self.align_read(r, m, effort) for r in reads]
        c = {"reads": len(rows), "no_overlap": 0, "aligned": 0, "not_aligned": 0}
        for st, _ in rows:
            c[["no_overlap", "not_aligned", "aligned"][st & 3]] += 1
        return rows, c


def rows_of(paths, poffs, status):
    """(paths, path_offsets, status) as the batch API returns them -> rows [(status, path)]"""
    return [(int(status[i]), [int(x) for x in paths[int(poffs[i]):int(poffs[i + 1])]]) for i in range(len(status))]
