#!/usr/bin/env python3
"""Where does a kernel's hot loop wait for its own memory operations?  Reads an assembly listing (.s) made with the flags of
snarkvm_amd/build.py plus `--cuda-device-only -S` and, for one kernel, walks the hot loop in program order keeping the vmcnt
queue (gfx950 counts vector loads AND stores in vmcnt, retired in issue order; `s_waitcnt vmcnt(N)` returns when at most N are
outstanding).  For every vector memory operation issued in the loop it prints how many VALU instructions, and how many of them
64-bit multiply-adds, stand between its issue and the first s_waitcnt that retires it: an operation retired after fewer
multiply-adds than one point addition holds (3 046) is waited for with the SIMD idle unless another wave covers it.

The hot loop is the loop around the block with the most multiply-adds (the addition): the blocks that reach a backward branch
without passing its target, for every backward branch whose loop holds that block.  The walk is linear: every block of the loop
in layout order, conditional ones (the flush) included, which is the order a wave with some lane in every branch executes
them.  Skipped, because they are off the hot path: loops inside the hot loop that do not hold the addition (the empty-bucket
search), every block with a call (s_swappc: the exceptional addition), and the blocks named with --ignore-block.  Skipped blocks neither issue nor retire anything and their instructions are not counted.  The loop is
walked three times - once to fill the queue as the previous iteration leaves it, once to issue, once more to retire what the
back edge carries - and only the middle iteration's operations are reported.

Only s_waitcnt, vector loads / stores, labels, branches and the v_* opcodes (counted, not interpreted) are read.

usage: isa_waits.py file.s <substring of the mangled kernel name> [--require-mads N] [--ignore-block .LBBx_y]...
exit status 1 with --require-mads N when an operation of the hot path is retired after fewer than N multiply-adds."""
import argparse
import re
import sys

MADS = ("v_mad_u64_u32", "v_mad_i64_i32")
VMEM = re.compile(r"^(global|flat|scratch|buffer)_(load|store|atomic)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
INSTR = re.compile(r"^\s+([a-z_0-9]+)(\s|$)")
BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")


def kernel_body(lines, key):
    start = end = None
    for i, l in enumerate(lines):
        if start is None and re.match(r"^_Z\S*:", l) and key in l:
            start = i
        elif start is not None and l.startswith(".Lfunc_end"):
            end = i
            break
    if start is None or end is None:
        sys.exit(f"isa_waits: no kernel whose name contains '{key}'")
    return start, end


def vmcnt_of(line):
    """Outstanding operations a `s_waitcnt` allows, None when it does not wait on vmcnt."""
    m = re.search(r"vmcnt\((\d+)\)", line)
    if m:
        return int(m.group(1))
    m = re.match(r"^\s+s_waitcnt\s+(0x[0-9a-f]+|\d+)\s*$", line)
    if m:  # unsymbolic form: vmcnt = bits 3:0 and 15:14 of the immediate
        imm = int(m.group(1), 0)
        v = (imm & 0xf) | (((imm >> 14) & 3) << 4)
        return None if v == 63 else v
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--require-mads", type=int, default=None)
    ap.add_argument("--ignore-block", action="append", default=[])
    args = ap.parse_args()
    lines = open(args.listing).read().split("\n")
    k0, k1 = kernel_body(lines, args.kernel)
    # blocks in layout order: (label, first line, last line + 1)
    blocks, cur, first = [], "entry", k0 + 1
    for i in range(k0 + 1, k1):
        m = LABEL.match(lines[i])
        if m:
            blocks.append((cur, first, i))
            cur, first = m.group(1), i + 1
    blocks.append((cur, first, k1))
    index = {b[0]: n for n, b in enumerate(blocks)}

    def opcodes(b):
        for i in range(b[1], b[2]):
            l = lines[i]
            m = INSTR.match(l)
            if m and not l.strip().startswith((".", ";")):
                yield i, m.group(1), l

    mads = [sum(op in MADS for _, op, _ in opcodes(b)) for b in blocks]
    hot = max(range(len(blocks)), key=lambda n: mads[n])
    # control flow between the labelled blocks: branch targets, and the next block unless the last instruction cannot fall through
    succs = [set() for _ in blocks]
    for n, b in enumerate(blocks):
        last = None
        for i, op, l in opcodes(b):
            last = op
            m = BRANCH.match(l)
            if m and m.group(1) in index:
                succs[n].add(index[m.group(1)])
        if last not in ("s_branch", "s_endpgm", "s_setpc_b64") and n + 1 < len(blocks):
            succs[n].add(n + 1)

    def reached_from(n, within):
        """blocks of `within` at the end of a path of one or more edges from n that stays inside `within`"""
        seen, todo = set(), [n]
        while todo:
            for s in succs[todo.pop()]:
                if s in within and s not in seen:
                    seen.add(s)
                    todo.append(s)
        return seen

    everything = set(range(len(blocks)))
    after = reached_from(hot, everything)
    body = {n for n in after if hot in reached_from(n, everything)}  # the blocks on a cycle through the addition
    if hot not in body:
        sys.exit("isa_waits: the block with the most multiply-adds is in no loop")
    # where the loop is entered from outside: an iteration that ends early (a base at infinity: `continue`) is a cycle without the
    # addition, but it passes the loop's entry; a loop INSIDE the iteration (the empty-bucket search) passes neither
    entries = {n for n in body if any(n in succs[p] for p in everything - body)}
    rest = body - entries - {hot}
    lo, hi = min(body), max(body)
    skipped = {n: "not in the loop" for n in range(lo, hi + 1) if n not in body}
    for n in rest:
        if n in reached_from(n, rest):
            skipped[n] = "inner loop"
    for n in body:
        if any(op == "s_swappc_b64" for _, op, _ in opcodes(blocks[n])):
            skipped[n] = "call"
        if blocks[n][0] in args.ignore_block:
            skipped[n] = "--ignore-block"
    for name in args.ignore_block:
        if name not in index or index[name] not in body:
            sys.exit(f"isa_waits: --ignore-block {name} is not a block of the hot loop")
    meta = {}
    for l in lines[k1:k1 + 80]:
        m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)", l)  # (scratch of a kernel with a call: the cold callee's frame included)
        if m:
            meta[m.group(1)] = int(m.group(2))
    print(f"kernel: {lines[k0].rstrip(':')}")
    print(f"meta: {meta}")
    print(f"hot loop: {blocks[lo][0]} .. {blocks[hi][0]} (lines {blocks[lo][1]} - {blocks[hi][2]}), addition in {blocks[hot][0]} ({mads[hot]} multiply-adds)")
    for n in sorted(skipped):
        print(f"skipped: {blocks[n][0]} ({skipped[n]}, {sum(1 for _ in opcodes(blocks[n]))} instructions)")

    queue, report = [], []  # queue entries: [line, opcode, block, valu at issue, mads at issue, reported?]
    valu = mad = 0
    for walk in range(3):
        for n in range(lo, hi + 1):
            if n in skipped:
                continue
            for i, op, l in opcodes(blocks[n]):
                if op.startswith("v_"):
                    valu += 1
                    mad += op in MADS
                elif VMEM.match(op):
                    queue.append([i + 1, op, blocks[n][0], valu, mad, walk == 1])
                elif op == "s_waitcnt":
                    allow = vmcnt_of(l)
                    if allow is None:
                        continue
                    while len(queue) > allow:
                        e = queue.pop(0)
                        if e[5]:
                            report.append((e[0], e[1], e[2], i + 1, blocks[n][0], l.split(None, 1)[1].strip(), valu - e[3], mad - e[4]))
    left = [e for e in queue if e[5]]
    print(f"\n{'line':>8s}  {'operation':24s} {'block':12s} {'retired at':>10s}  {'by':28s} {'VALU':>6s} {'mads':>6s}")
    bad = 0
    for line, op, blk, wline, wblk, wait, dv, dm in sorted(report):
        short = args.require_mads is not None and dm < args.require_mads
        bad += short
        print(f"{line:8d}  {op:24s} {blk:12s} {wline:10d}  {(wblk + ' ' + wait)[:28]:28s} {dv:6d} {dm:6d}{'  <-- waited for before the addition' if short else ''}")
    for e in left:
        print(f"{e[0]:8d}  {e[1]:24s} {e[2]:12s} {'never':>10s}  (no wait within one further iteration)")
    loads = sum(r[1].split('_')[1] == 'load' for r in report)
    print(f"\n{len(report)} operations per iteration ({loads} loads, {len(report) - loads} stores / atomics); "
          f"fewest multiply-adds before a retiring wait: {min((r[7] for r in report), default=0)}")
    if args.require_mads is not None:
        print(f"--require-mads {args.require_mads}: {'FAIL, ' + str(bad) + ' operations' if bad else 'ok'}")
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
