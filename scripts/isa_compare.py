"""Compare the generated gfx950 code of two builds, kernel by kernel: the instruction streams with comments, labels and
debug lines stripped, and each kernel's registers and scratch.

  hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -I include -S --cuda-device-only \
        pyhmmer_amd/csrc/p7x_pipeline.hip -o before/p7x_pipeline.s        (the same at the other commit into after/)
  python scripts/isa_compare.py before after

prints one markdown table row per kernel: file | kernel | same / differs | VGPR | SGPR | scratch bytes (of the second build;
"a -> b" where the two differ), and for a kernel that differs the unified diff of its instructions."""
import difflib, pathlib, re, shutil, subprocess, sys


def kernels(path):
    """name -> (instructions, {NumVgprs, TotalNumSgprs, ScratchSize}) of every .amdhsa_kernel of an assembly file."""
    lines = path.read_text().splitlines()
    names = {m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    out, cur, tail = {}, None, None
    for l in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if m and m.group(1) in names:
            cur = tail = m.group(1); out[cur] = ([], {}); continue
        if l.startswith(".Lfunc_end"):
            cur = None; continue
        if cur:
            t = l.split(";")[0].strip()
            if t and not t.startswith(".") and not t.endswith(":"):
                out[cur][0].append(re.sub(r"\.LBB\d+_", ".LBB_", t))      # (the function's number is not part of its code)
        elif tail and (m := re.match(r";\s*(NumVgprs|TotalNumSgprs|ScratchSize):\s*(\d+)", l)):
            out[tail][1].setdefault(m.group(1), int(m.group(2)))
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        got = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, got))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


before, after = pathlib.Path(sys.argv[1]), pathlib.Path(sys.argv[2])
print("| file | kernel | code | VGPR | SGPR | scratch |\n|---|---|---|---|---|---|")
diffs = []
for fa in sorted(after.glob("*.s")):
    a, b = kernels(fa), kernels(before / fa.name)
    pretty = demangle(sorted(set(a) | set(b)))
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"| {fa.stem} | `{pretty[k]}` | only in {'the second' if k in a else 'the first'} | | | |"); continue
        same = a[k][0] == b[k][0]
        res = [str(a[k][1].get(r)) if a[k][1].get(r) == b[k][1].get(r) else f"{b[k][1].get(r)} -> {a[k][1].get(r)}" for r in ("NumVgprs", "TotalNumSgprs", "ScratchSize")]
        print(f"| {fa.stem} | `{pretty[k]}` | {'same' if same else 'differs'} | {res[0]} | {res[1]} | {res[2]} |")
        if not same:
            diffs.append((pretty[k], list(difflib.unified_diff(b[k][0], a[k][0], "first", "second", lineterm="", n=2))))
for name, d in diffs:
    print(f"\n{name}\n" + "\n".join(d))
