"""Instruction counts per basic block of a compiler listing (hipcc -S), lines [start, end):
python tools/isa_blocks.py LISTING.s START END [--weighted]

--weighted adds, per block, the vector instructions weighted by their measured issue cost (profiles/r03_valu_rates.txt, >= 2 waves per
SIMD): 2 cycles for plain add/sub/and/or/xor/mov/not/32-bit right shift (e32 and e64 forms), 2.5 for v_bitop3, 4 for every other vector
opcode.  Lane reads and writes (readlane, writelane, readfirstlane) are counted apart, as before, and carry no weight."""
import re, sys
args = [a for a in sys.argv[1:] if a != '--weighted']
weighted = '--weighted' in sys.argv[1:]
lines = open(args[0]).read().split('\n')
start, end = int(args[1]), int(args[2])
CHEAP = re.compile(r'^v_(add_u32|add_co_u32|addc_co_u32|sub_u32|sub_co_u32|subb_co_u32|subrev_u32|subrev_co_u32|subbrev_co_u32|and_b32|or_b32|xor_b32|'
                   r'mov_b32|not_b32|lshrrev_b32)(_e32|_e64)?$')
def cost(ins):
    op = ins.split()[0]
    if CHEAP.match(op): return 2.0
    if op.startswith('v_bitop3'): return 2.5
    return 4.0
blocks = []  # (label, first_line, insts)
cur = ('entry', start, [])
for n in range(start, end):
    l = lines[n]
    m = re.match(r'^(\.LBB\d+_\d+):', l)
    if m:
        blocks.append(cur); cur = (m.group(1), n + 1, [])
        continue
    t = l.strip()
    if not t or t.startswith(';') or t.startswith('.'): continue
    cur[2].append(t)
blocks.append(cur)
idx = {b[0]: i for i, b in enumerate(blocks)}
# back edges
loops = []
for i, b in enumerate(blocks):
    for ins in b[2]:
        m = re.match(r's_cbranch\w*\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)', ins)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in idx and idx[tgt] <= i: loops.append((idx[tgt], i))
depth = [0] * len(blocks)
for a, b in loops:
    for i in range(a, b + 1): depth[i] += 1
tot = {}
for i, b in enumerate(blocks):
    valu = [x for x in b[2] if x.startswith('v_') and not x.startswith('v_readlane') and not x.startswith('v_writelane') and not x.startswith('v_readfirstlane')]
    v = len(valu)
    rl = sum(1 for x in b[2] if x.startswith('v_readlane')); wl = sum(1 for x in b[2] if x.startswith('v_writelane')); rf = sum(1 for x in b[2] if x.startswith('v_readfirstlane'))
    s = sum(1 for x in b[2] if x.startswith('s_') and not x.startswith('s_waitcnt') and not x.startswith('s_nop'))
    mem = sum(1 for x in b[2] if x.startswith('global_') or x.startswith('buffer_') or x.startswith('scratch_') or x.startswith('flat_'))
    sc = sum(1 for x in b[2] if x.startswith('scratch_'))
    lds = sum(1 for x in b[2] if x.startswith('ds_'))
    w = sum(cost(x) for x in valu)
    wtxt = f" valu_cycles {w:6.1f}" if weighted else ""
    print(f"{b[0]:12s} line {b[1]:5d} depth {depth[i]} valu {v:3d}{wtxt} readlane {rl:2d} writelane {wl:2d} rfl {rf:2d} salu {s:3d} mem {mem:2d} scratch {sc:2d} lds {lds:2d}")
    d = depth[i]
    t = tot.setdefault(d, [0,0,0,0,0] + ([0.0] if weighted else [])); t[0]+=v; t[1]+=rl; t[2]+=wl; t[3]+=s; t[4]+=sc
    if weighted: t[5] += w
print(tot)
