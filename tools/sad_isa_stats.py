#!/usr/bin/env python3
"""Instruction mix of sad_strip_kernel<B,R> in a hipcc -save-temps .s file: counts by mnemonic class, registers, LDS, scratch,
and the same counts per basic block along the path an interior strip takes.
  python tools/sad_isa_stats.py <file.s> [B R] [--blocks]     (default 8 32: BASELINE configs[3])

The interior path (a strip the frame does not clip, every block inside the frame) is found from the code, not from names: the
walk of an interior strip is the one basic block that holds SPLIT passes' worth of packed SADs at once, and a strip takes either
that block or the clipped chunks.  Blocks are split at labels and behind every conditional branch.  From the entry to the walk a
branch is followed to the side that reaches the walk through the fewest packed SADs (none: no clipped chunk on the way; of two
equal sides the fall-through, i.e. the body of an `if` such as a staging step), behind the walk to the side that carries work
(what hipcc shares between both forms of the walk, the last dy's key builds, is counted).  --blocks prints one row per block of
that path."""
import collections
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
show_blocks = "--blocks" in sys.argv
path = args[0]
B, R = (int(args[1]), int(args[2])) if len(args) > 2 else (8, 32)
name = f"_ZN12_GLOBAL__N_116sad_strip_kernelILi{B}ELi{R}EEEvNS_9SadParamsEii"
txt = open(path).read()
start = txt.index(name + ":")
end = txt.index(".Lfunc_end", start)
body = txt[start:end]
ops = collections.Counter()


def is_insn(ln):
    return bool(ln) and not ln.startswith((";", ".", "_Z", "s_nop")) and not ln.endswith(":")


for ln in body.splitlines():
    ln = ln.strip()
    if not is_insn(ln) or ln.startswith("BB"):
        continue
    ops[ln.split()[0]] += 1


def tot(pred, o=ops):
    return sum(v for k, v in o.items() if pred(k))


SADS = ("v_qsad_pk_u16_u8", "v_sad_u8")
valu = tot(lambda k: k.startswith("v_"))
print(f"{path}: sad_strip_kernel<{B},{R}>")
print("  VALU", valu, " of which qsad", ops["v_qsad_pk_u16_u8"], " sad_u8", ops["v_sad_u8"], " other", valu - ops["v_qsad_pk_u16_u8"] - ops["v_sad_u8"])
print("  SALU", tot(lambda k: k.startswith("s_") and not k.startswith(("s_waitcnt", "s_cbranch", "s_branch", "s_barrier"))),
      " branches", tot(lambda k: k.startswith(("s_cbranch", "s_branch"))), " s_waitcnt", ops["s_waitcnt"])
print("  LDS", tot(lambda k: k.startswith("ds_")), {k: v for k, v in ops.items() if k.startswith("ds_")})
print("  VMEM", tot(lambda k: k.startswith(("global_", "buffer_", "scratch_", "flat_"))),
      {k: v for k, v in ops.items() if k.startswith(("global_", "buffer_", "scratch_", "flat_"))})
keys = ["v_min3_u32", "v_min_u32", "v_lshl_or_b32", "v_and_or_b32", "v_add_u32", "v_mov_b32", "v_cndmask_b32", "v_or_b32", "v_and_b32",
        "v_lshlrev_b32", "v_lshrrev_b32", "v_bfi_b32", "v_perm_b32", "v_or3_b32", "v_readlane_b32", "v_writelane_b32", "s_mov_b32", "s_cselect_b32",
        "s_movk_i32", "v_accvgpr_write_b32", "v_accvgpr_read_b32"]
print("  ", {k: ops[k] for k in keys if ops[k]})
other = {k: v for k, v in ops.most_common() if k.startswith("v_") and k not in keys and k not in SADS}
print("   other VALU:", dict(list(other.items())[:14]))
# the resource comments hipcc writes behind the function: registers, scratch, occupancy, LDS
tail = txt[end:end + 4000]
res = {k: int(v) for k, v in re.findall(r";\s*(NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", tail[:tail.find(".text") if ".text" in tail else None])}
print("  ", res)

# ---- basic blocks and the interior path
blocks, order, cur = {}, [], "entry"
blocks[cur] = {"ops": collections.Counter(), "succ": [], "fall": True}
order.append(cur)
for ln in body.splitlines()[1:]:
    ln = ln.strip()
    m = re.match(r"^(\.LBB\d+_\d+):", ln)
    if m:
        prev, cur = cur, m.group(1)
        blocks[cur] = {"ops": collections.Counter(), "succ": [], "fall": True}
        order.append(cur)
        if blocks[prev]["fall"]:
            blocks[prev]["succ"].append(cur)
        continue
    if not is_insn(ln):
        continue
    op = ln.split()[0]
    blocks[cur]["ops"][op] += 1
    if op.startswith("s_cbranch"):
        # the code behind a conditional branch is a block of its own
        blocks[cur]["succ"].append(ln.split()[1])
        prev, cur = cur, f"{cur.split('+')[0]}+{len(order)}"
        blocks[cur] = {"ops": collections.Counter(), "succ": [], "fall": True}
        order.append(cur)
        blocks[prev]["succ"].append(cur)
    elif op == "s_branch":
        blocks[cur]["succ"].append(ln.split()[1])
        blocks[cur]["fall"] = False
    elif op == "s_endpgm":
        blocks[cur]["fall"] = False
qs = {b: blocks[b]["ops"]["v_qsad_pk_u16_u8"] for b in order}
big = max(order, key=lambda b: qs[b])


# fewest packed SADs between a block and the walk (the walk itself not counted): an interior strip passes no clipped chunk
INF = 1 << 60
cost = {b: INF for b in order}
cost[big] = 0
for _ in order:
    for b in order:
        if b != big:
            c = min([cost[s] for s in blocks[b]["succ"] if s in blocks] or [INF])
            cost[b] = min(cost[b], qs[b] + c) if c < INF else cost[b]
pathb, b, passed = [], "entry", False
while True:
    pathb.append(b)
    passed = passed or b == big
    succ = [s for s in blocks[b]["succ"] if s in blocks and s not in pathb]
    if not succ:
        break
    if not passed:
        # towards the walk; among several such successors the one that passes no clipped chunk (fewest packed SADs on the way)
        nxt = min(succ, key=lambda s: (cost[s], order.index(s)))
    else:
        # after the walk: the side that carries the work (a skipped `if` body has none); ties go to the fall-through
        nxt = max(succ, key=lambda s: (sum(blocks[s]["ops"].values()) > 2, -order.index(s)))
    b = nxt


def row(o):
    v = tot(lambda k: k.startswith("v_"), o)
    return (o["v_qsad_pk_u16_u8"], o["v_sad_u8"], v - o["v_qsad_pk_u16_u8"] - o["v_sad_u8"],
            tot(lambda k: k.startswith("ds_"), o), tot(lambda k: k.startswith(("global_", "buffer_")), o), o["s_waitcnt"])


sums = [0] * 6
if show_blocks:
    print(f"  interior path ({len(pathb)} blocks; walk = {big}):  block  qsad  sad_u8  other-VALU  LDS  VMEM  s_waitcnt")
for b in pathb:
    r = row(blocks[b]["ops"])
    sums = [a + c for a, c in zip(sums, r)]
    if show_blocks and any(r):
        top = [f"{k}:{v}" for k, v in blocks[b]["ops"].most_common() if k.startswith("v_") and k not in SADS][:6]
        print(f"    {b:12s} {r[0]:5d} {r[1]:6d} {r[2]:6d} {r[3]:5d} {r[4]:4d} {r[5]:4d}   {' '.join(top)}")
print(f"  interior path: qsad {sums[0]}  sad_u8 {sums[1]}  non-SAD VALU {sums[2]}  LDS {sums[3]}  VMEM {sums[4]}  s_waitcnt {sums[5]}")
