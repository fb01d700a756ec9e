#!/usr/bin/env python3
"""Scan gfx950 assembly for multiplications whose 32-bit operand is an unmasked carry, and print ISA histograms of kernels and their loops.

  hipcc -O3 --offload-arch=gfx950 -std=c++17 --cuda-device-only -S bulletproofspp_amd/csrc/msm.hip -o msm.s
  python benchmarks/isa_carry_operands.py scan msm.s [kernel regex]     flagged v_mad_u64_u32 per kernel (0 is what every kernel must show)
  python benchmarks/isa_carry_operands.py hist msm.s [kernel regex]     histogram of each kernel and of its loops with over 300 products

Why: the field products mask a carry (c & 0xFFFFFF, c & 0x3FFFFF) into the top limb.  Where the compiler sees both top limbs of a product as
24-bit values it may take a8 * b8 for a 24-bit multiplication, drop the masks, and still select the full v_mad_u64_u32 (DESIGN.md 0.2, row
"exception-free mixed addition"; csrc/ec29.hip.h, fq29_opaque8).  In right code every multiplicand of a v_mad_u64_u32 with two vector operands
is the result of a 32-bit operation (mask, shift, add, select, load); in the faulty code it is the low half of a register pair that a 64-bit
operation wrote in the same basic block.  The scan is linear per kernel and forgets all writers at a label, so it reports only same-block evidence.
It is meant for the 26- and 29-bit limb code.  In 8 x 32-bit limb code (fe.hip.h) the low word of a product IS a limb, so such kernels are flagged
without being wrong (k_rp_scan_table_keys of rpscan_keys.hip: 150)."""
import collections
import re
import sys

def kernels(path):
    txt = open(path).read().splitlines()
    out, cur, name = {}, None, None
    for ln in txt:
        m = re.match(r'^(_ZN4bppp\w+):', ln)
        if m: name, cur = m.group(1), []; continue
        if name is not None:
            if ln.startswith('.Lfunc_end'): out[name] = cur; name = None; continue
            cur.append(ln)
    return out
def instrs(lines):
    res = []
    for ln in lines:
        s = ln.split(';')[0].strip()
        if not s or s.startswith('.') and not s.endswith(':') : continue
        if s.endswith(':'): res.append(('label', s[:-1])); continue
        if s.startswith('.'): continue
        res.append(('ins', s))
    return res
def hist(ins):
    c = collections.Counter(s.split()[0] for k, s in ins if k == 'ins')
    return c
def loops(ins):
    pos = {s: i for i, (k, s) in enumerate(ins) if k == 'label'}
    out = []
    for i, (k, s) in enumerate(ins):
        if k == 'ins' and (s.startswith('s_cbranch') or s.startswith('s_branch')):
            t = s.split()[-1]
            if t in pos and pos[t] < i: out.append((pos[t], i))
    return out
def show(title, c):
    print(f"== {title}: {sum(c.values())} instructions")
    for k, v in sorted(c.items(), key=lambda kv: (-kv[1], kv[0])): print(f"{v:7d} {k}")
    print()


W64 = ('v_mad_u64_u32', 'v_lshrrev_b64', 'v_lshl_add_u64', 'v_lshlrev_b64')
def regs(tok):
    m = re.match(r'v\[(\d+):(\d+)\]', tok)
    if m: return list(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r'v(\d+)$', tok)
    return [int(m.group(1))] if m else []
def scan(name, ins):
    last = {}
    bad = []
    for i, (k, s) in enumerate(ins):
        if k != 'ins':
            last = {}          # a label: forget the writers (only same-block evidence counts)
            continue
        op, _, rest = s.partition(' ')
        toks = [t.strip() for t in rest.split(',')]
        if op == 'v_mad_u64_u32' and all(regs(t) for t in toks[2:4]):
            for t in toks[2:4]:
                for r in regs(t):
                    w = last.get(r)
                    if w and w[0].startswith(W64) and w[2] == 0:      # low half of a 64-bit result
                        bad.append((i, s, w))
        if op.startswith(('v_', 'global_load', 'ds_read', 'buffer_load')) and toks and not op.startswith('v_cmp'):
            d = regs(toks[0])
            for j, r in enumerate(d):
                last[r] = (op, i, j if op.startswith(W64) and len(d) == 2 else -1)
    return bad


def main():
    mode, path, pat = sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "."
    total = 0
    for name, lines in kernels(path).items():
        if not re.search(pat, name):
            continue
        ins = instrs(lines)
        if mode == "scan":
            bad = scan(name, ins)
            total += len(bad)
            n = sum(1 for k, s in ins if k == "ins" and s.startswith("v_mad_u64_u32"))
            print(f"{name[:70]:70s} products {n:6d}  flagged {len(bad)}")
            for b in bad[:8]:
                print("    ", b[0], b[1], "<- low half of", b[2][0], "at", b[2][1])
        else:
            show("whole kernel " + name, hist(ins))
            for a, b in loops(ins):
                h = hist(ins[a:b + 1])
                if h["v_mad_u64_u32"] > 300:
                    show(f"loop of {name} (instructions {a}..{b})", h)
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
