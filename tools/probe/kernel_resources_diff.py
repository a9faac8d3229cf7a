"""Kernel resources and instruction counts of two builds of the same .hip files, side by side.

Each directory holds, per source file NAME, what
  hipcc <flags of ops/build.py> -Rpass-analysis=kernel-resource-usage --save-temps -c NAME.hip 2> NAME.remarks
leaves behind: NAME.remarks and NAME-hip-amdgcn-amd-amdhsa-gfx950.s.  Prints one markdown row per kernel
of the second directory (resources; 'same' or what differs from the first), then per kernel the
counts of the instruction classes that carry the memory and matrix work, and whether the opcode sequence
(mnemonics in program order, operands dropped) is the parent's.  A kernel is compared with the parent's
kernel of the same mangled name, else of the same name without its arguments, else with the one a
NEW=OLD argument names (a kernel that was renamed or became a template instantiation).  ``--hunks``
prints where the opcode sequences differ, block labels included (a hunk between a loop's label and its
backward branch is inside the loop).

  python tools/probe/kernel_resources_diff.py PARENT_DIR NEW_DIR skinny_gemm skinny_w4
  python tools/probe/kernel_resources_diff.py PARENT_DIR NEW_DIR flash_ctx --hunks \
      'flash_ctx_kernel<false, false>=flash_ctx_kernel' 'flash_ctx_kernel<false, true>=flash_ctx_split_kernel'
"""
import collections
import difflib
import re
import shutil
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size"]
MUST_MATCH = ["SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size"]
CLASSES = ["v_mfma", "buffer_load", "buffer_store", "ds_", "global_", "s_barrier"]


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = []
    for d in out[: len(names)]:
        d = d.replace("(anonymous namespace)::", "")
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\((SkArgs|W4Args)\)$", "", d)
        short.append(re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", d) if d.endswith(")") else d)
    return dict(zip(names, short))


def resources(path):
    res, cur = collections.OrderedDict(), None
    for line in open(path):
        m = re.search(r"remark: .*?:\s+(Function Name|[A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = res.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[key] = int(val)
    return res


def opcodes(path):
    """-> {kernel: [mnemonic or block label, ...]} in program order"""
    ops, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = ops.setdefault(m.group(1), [])
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            cur.append(re.sub(r"^\.LBB\d+", ".LBB", m.group(1)) + ":")
        elif re.match(r"^\t[a-z]", line):
            cur.append(line.strip().split(" ")[0].split("\t")[0])
    return ops


def instr_counts(ops):
    return collections.Counter(c for op in ops for c in CLASSES if op.startswith(c))


def sequence_vs(pa, pb, hunks):
    a, b = [o for o in pa if not o.endswith(":")], [o for o in pb if not o.endswith(":")]
    if a == b:
        return f"identical ({len(b)})"
    sm = difflib.SequenceMatcher(None, pa, pb, autojunk=False)
    changed = [op for op in sm.get_opcodes() if op[0] != "equal"]
    for tag, i1, i2, j1, j2 in changed:
        hunks.append(f"  parent [{i1}:{i2}] {' '.join(pa[i1:i2]) or '-'}\n"
                     f"  new    [{j1}:{j2}] {' '.join(pb[j1:j2]) or '-'}")
    return f"{len(a)} -> {len(b)} opcodes, {len(changed)} hunks differ"


def main():
    args = [a for a in sys.argv[1:] if a != "--hunks"]
    show_hunks = "--hunks" in sys.argv[1:]
    a_dir, b_dir = args[0], args[1]
    names = [a for a in args[2:] if "=" not in a]
    renamed = dict(a.split("=", 1) for a in args[2:] if "=" in a)
    for name in names:
        ra, rb = resources(f"{a_dir}/{name}.remarks"), resources(f"{b_dir}/{name}.remarks")
        oa = opcodes(f"{a_dir}/{name}-hip-amdgcn-amd-amdhsa-gfx950.s")
        ob = opcodes(f"{b_dir}/{name}-hip-amdgcn-amd-amdhsa-gfx950.s")
        dm = demangle(sorted(set(ra) | set(rb)))
        by_short = {dm[k]: k for k in ra}
        parent_of = {k: k if k in ra else by_short.get(renamed.get(dm[k], dm[k])) for k in rb}
        print(f"\n## {name}.hip: {len(ra)} kernels in the parent, {len(rb)} in this tree")
        for k in ra:
            if k not in parent_of.values():
                print(f"removed: {dm[k]}")
        print("\n| kernel | parent's | " + " | ".join(FIELDS) + " | vs parent | " + " | ".join(CLASSES)
              + " | instructions vs parent | opcode sequence vs parent |")
        print("|---|" + "---|" * (len(FIELDS) + len(CLASSES) + 4))
        worse, all_hunks = [], []
        for k, r in rb.items():
            pk = parent_of[k]
            p = ra.get(pk)
            if p is None:
                vs = "new"
            else:
                d = [f"{f} {p[f]} -> {r[f]}" for f in FIELDS if p[f] != r[f]]
                vs = "; ".join(d) if d else "same"
                if any(p[f] != r[f] for f in MUST_MATCH):
                    worse.append(dm[k])
            cb, ca = instr_counts(ob.get(k, [])), instr_counts(oa.get(pk, []))
            di = [f"{c} {ca.get(c, 0)} -> {cb.get(c, 0)}" for c in CLASSES if ca.get(c, 0) != cb.get(c, 0)]
            hunks = []
            seq = sequence_vs(oa[pk], ob[k], hunks) if pk in oa and k in ob else "-"
            if hunks:
                all_hunks.append((dm[k], hunks))
            print(f"| {dm[k]} | {dm[pk] if pk else '-'} | " + " | ".join(str(r[f]) for f in FIELDS) + f" | {vs} | "
                  + " | ".join(str(cb.get(c, 0)) for c in CLASSES) + " | " + ("; ".join(di) if di else "same")
                  + f" | {seq} |")
        if worse:
            print("\nspills / scratch / occupancy / LDS differ: " + ", ".join(worse))
        if show_hunks:
            for kname, hunks in all_hunks:
                print(f"\n### {kname}: opcode hunks against the parent (positions count block labels)")
                print("\n".join(hunks))


if __name__ == "__main__":
    main()
