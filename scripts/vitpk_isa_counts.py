"""Instruction counts of the packed Viterbi kernel from its generated ISA, per instantiation of vitpk_kernel<T, P>: one row
(the row-pair loop without the pass loops inside it, halved) and one pass of the D->D closure loop (mean of the innermost
loops inside the pair loop), by class: packed 16-bit, other VALU, LDS, s_waitcnt, s_nop, scalar.

  hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -I include -S --cuda-device-only \
        pyhmmer_amd/csrc/p7x_vitpk.hip -o vitpk.s
  python scripts/vitpk_isa_counts.py vitpk.s

prints table rows: instantiation | row: all, packed, other VALU, LDS, waitcnt, nop, scalar | pass: all, packed, other VALU,
LDS, scalar | pass loops found (two: one per row of the pair)."""
import re, sys, collections

def classify(op):
    if op.startswith("v_pk_"): return "pk"
    if op.startswith("ds_"): return "lds"
    if op == "s_waitcnt": return "wait"
    if op == "s_nop": return "nop"
    if op.startswith("v_"): return "valu"
    if op.startswith("s_"): return "salu"
    return "other"

def kernels(path):
    cur = None; out = {}
    for l in open(path):
        m = re.match(r"^_ZN3p7x12vitpk_kernelILi(\d+)ELi(\d+)EEEvNS_6ArgRefE:", l)
        if m: cur = (int(m.group(1)), int(m.group(2))); out[cur] = []; continue
        if l.startswith(".Lfunc_end"): cur = None
        if cur: out[cur].append(l.rstrip("\n"))
    return out

def analyse(lines):
    # blocks: label -> (header comment text, instrs)
    blocks = []; cur = None
    for l in lines:
        m = re.match(r"^\.L(BB\d+_\d+):(.*)$", l)
        if m: cur = {"label": m.group(1), "c": m.group(2), "ins": []}; blocks.append(cur); continue
        if cur is None: continue
        t = l.strip()
        if t.startswith(";") and not cur["ins"] and not t.startswith("; %bb"): cur["c"] += " " + t; continue
        if t.startswith("; %bb."):      # fallthrough block: same loop membership comment follows on the line
            cur = {"label": t.split()[1], "c": t, "ins": []}; blocks.append(cur); continue
        if not t or t.startswith(";") or t.startswith("."): continue
        cur["ins"].append(t.split()[0])
    # loop headers with depth
    hdr = {}
    for b in blocks:
        m = re.search(r"Loop Header: Depth=(\d+)", b["c"])
        if m: hdr[b["label"]] = int(m.group(1))
    def members(h):
        return [b for b in blocks if b["label"] == h or re.search(r"in Loop: Header=" + h + r"\b", b["c"])]
    def count(bs):
        c = collections.Counter()
        for b in bs:
            for op in b["ins"]: c[classify(op)] += 1
        return c
    deepest = max(hdr.values())
    inner = [h for h, d in hdr.items() if d == deepest]
    # the pair loop: the header of depth deepest-1 with the most instructions
    pair = max((h for h, d in hdr.items() if d == deepest - 1), key=lambda h: sum(len(b["ins"]) for b in members(h)))
    pc = count(members(pair))
    kids = [h for h in inner if re.search(r"Parent Loop " + pair.replace("BB", "BB") + r"\b", next(b for b in blocks if b["label"] == h)["c"])]
    kc = [count(members(h)) for h in kids]
    return pc, kc

for path in sys.argv[1:]:
    print(path)
    for k, lines in kernels(path).items():
        try:
            pc, kc = analyse(lines)
        except Exception as e:
            print(k, "?", e); continue
        row = {c: pc[c] / 2 for c in ("pk", "valu", "lds", "wait", "nop", "salu")}
        ps = {c: sum(x[c] for x in kc) / max(len(kc), 1) for c in ("pk", "valu", "lds", "wait", "nop", "salu")}
        tot = sum(row.values()); pt = sum(ps.values())
        print(f"| `<{k[0]}, {k[1]}>` | {tot:.0f} | {row['pk']:.0f} | {row['valu']:.0f} | {row['lds']:.0f} | {row['wait']:.0f} | {row['nop']:.0f} | {row['salu']:.0f} | {pt:.0f} | {ps['pk']:.0f} | {ps['valu']:.0f} | {ps['lds']:.0f} | {ps['salu']:.0f} | {len(kc)} |")
