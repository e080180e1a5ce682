#!/usr/bin/env python3
"""How a kernel waits for its LDS reads, from hipcc -S output: every ds_read* with the number of LDS reads that are in
flight when the wave first waits for it (1 = the wave sits through that read's round trip alone), and the number of
other instructions between the read and that wait.  A read's wait is the first s_waitcnt after it whose lgkmcnt is
smaller than the number of LDS/scalar-memory operations issued since the read, itself included (they return in order as
far as LDS is concerned; scalar loads in between are counted as in flight too, which can only overstate the overlap).
usage: lds_waits.py file.s mangled-kernel-substring [first-line last-line]   (line numbers inside the kernel's body)"""
import re
import sys

txt = open(sys.argv[1]).read().splitlines()
key = sys.argv[2]
lo, hi = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (0, 1 << 30)
on = False
body = []
for l in txt:
    if re.match(r"^_Z\w*%s\w*:\s*(;.*)?$" % re.escape(key), l):
        on = True
        continue
    if on and l.startswith(".Lfunc_end"):
        break
    if on:
        body.append(l)

pending = []  # [body line, text, is_read, instructions since]
lone = total = 0
for n, l in enumerate(body, 1):
    m = re.match(r"^\s+([a-z_0-9]+)\s*(.*)$", l)
    if not m:
        continue
    op, args = m.group(1), m.group(2).split(";")[0].strip()
    if op == "s_waitcnt":
        w = re.search(r"lgkmcnt\((\d+)\)", args)
        if w:
            keep = int(w.group(1))
            done, pending = pending[: max(0, len(pending) - keep)], pending[max(0, len(pending) - keep):]
            flight = sum(1 for p in done + pending if p[2])
            for p in done:
                if p[2] and lo <= p[0] <= hi:
                    total += 1
                    lone += flight == 1
                    print(f"{p[0]:6d}  in flight {flight:2d}  {p[3]:3d} instructions to its wait  {p[1]}")
        for p in pending:
            p[3] += 1
        continue
    if op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
        for p in pending:
            p[3] += 1
        pending.append([n, f"{op} {args}", op.startswith("ds_read"), 0])
        continue
    for p in pending:  # (branches are not followed: the listing is read top to bottom)
        p[3] += 1
print(f"{total} LDS reads waited for in lines {lo}..{hi}, {lone} of them alone in flight")
