#!/usr/bin/env python3
"""Per-kernel comparison of two sets of `hipcc -S --cuda-device-only` outputs (no GPU needed): the parent commit's against this
one's, for jf_kernels.hip, jf_reverb.hip and jf_room.hip compiled with the Makefile's flags.

For every kernel: the opcode histogram, the float arithmetic singled out (v_(pk_)?(add|sub|mul|fma|fmac|mad)_f32*), and VGPRs,
SGPRs, LDS and scratch from the kernel's .amdhsa_ directives.  Prints the markdown of profiles/rv_spectrum/resources.md and
exits 1 if one of the criteria (a) - (c) there does not hold.

usage: compare_isa.py PARENT_DIR THIS_DIR     (each holding jf_kernels.s, jf_reverb.s, jf_room.s)

The .s files:  for f in jf_kernels jf_reverb jf_room; do
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -S --cuda-device-only -o DIR/$f.s $f.hip; done
"""
import collections
import re
import subprocess
import sys

UNITS = ("jf_kernels", "jf_reverb", "jf_room")
FLOAT = re.compile(r"^v_(pk_)?(add|sub|mul|fma|fmac|mad)_f32")
RES = {"vgpr": ".amdhsa_next_free_vgpr", "sgpr": ".amdhsa_next_free_sgpr", "lds": ".amdhsa_group_segment_fixed_size",
       "scratch": ".amdhsa_private_segment_fixed_size"}


def kernels(path):
    """mangled name -> (opcode Counter, resources dict) of every kernel in one .s file"""
    lines = open(path).read().splitlines()
    names = [m.group(1) for l in lines if (m := re.match(r"^\s+\.amdhsa_kernel\s+(\S+)", l))]
    out = {n: [collections.Counter(), {}] for n in names}
    cur = None
    for l in lines:
        if (m := re.match(r"^(\w+):", l)) and m.group(1) in out:
            cur = m.group(1)
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
        if cur and (m := re.match(r"^\s+([a-z][a-z_0-9]+)(\s|$)", l)):
            out[cur][0][m.group(1)] += 1
    desc = None
    for l in lines:
        if m := re.match(r"^\s+\.amdhsa_kernel\s+(\S+)", l):
            desc = m.group(1)
        elif desc:
            for key, word in RES.items():
                if (m := re.match(r"^\s+%s\s+(\d+)" % re.escape(word), l)):
                    out[desc][1][key] = int(m.group(1))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, r):
        d = re.sub(r"^void ", "", d).replace("jf::", "").replace("(anonymous namespace)::", "")
        d = re.sub(r"\(.*\)$", "", d)
        short[n] = d
    return short


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    bad = []
    for unit in UNITS:
        a, b = kernels(f"{a_dir}/{unit}.s"), kernels(f"{b_dir}/{unit}.s")
        short = demangle(sorted(set(a) | set(b)))
        print(f"\n## {unit}.hip: {len(b)} kernels\n")
        print("| kernel | VGPR | SGPR | LDS | scratch | instructions | float arithmetic | histogram |")
        print("|---|---|---|---|---|---|---|---|")
        notes = []
        for n in sorted(set(a) | set(b), key=lambda n: short[n]):
            if n not in a or n not in b:
                print(f"| `{short[n]}` | only in {'parent' if n in a else 'this'} |")
                bad.append(f"{short[n]}: not in both")
                continue
            (ha, ra), (hb, rb) = a[n], b[n]
            fa = {k: v for k, v in ha.items() if FLOAT.match(k)}
            fb = {k: v for k, v in hb.items() if FLOAT.match(k)}
            cell = lambda k: str(ra[k]) if ra[k] == rb[k] else f"**{ra[k]} -> {rb[k]}**"
            tot = lambda h: sum(h.values())
            diff = {k: hb.get(k, 0) - ha.get(k, 0) for k in set(ha) | set(hb) if ha.get(k, 0) != hb.get(k, 0)}
            hist = "identical" if not diff else "differs"
            print(f"| `{short[n]}` | {cell('vgpr')} | {cell('sgpr')} | {cell('lds')} | {cell('scratch')} | "
                  f"{tot(ha)}{'' if tot(ha) == tot(hb) else ' -> %d' % tot(hb)} | "
                  f"{tot(fa)}{' identical' if fa == fb else ' **-> %d, differs**' % tot(fb)} | {hist} |")
            if diff:
                notes.append(f"- `{short[n]}`: " + ", ".join(f"{k} {v:+d}" for k, v in sorted(diff.items())))
            head = "rv_head_wave" if unit == "jf_kernels" and re.search(r"rt_block_kernel<\d+, \d+, true", short[n]) else None
            if unit == "jf_kernels" and not head and (diff or ra != rb):
                bad.append(f"(a) {short[n]}")
            if any(ra[k] != rb[k] for k in ("vgpr", "lds", "scratch")) and (unit != "jf_kernels"):
                bad.append(f"(b) {short[n]}")
            if fa != fb and unit != "jf_kernels":
                bad.append(f"(c) {short[n]}")
        if notes:
            print("\nHistogram differences (this - parent):\n")
            print("\n".join(notes))
    print("\n## Criteria\n")
    print("all of (a), (b), (c) hold" if not bad else "NOT met:\n" + "\n".join(f"- {x}" for x in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
