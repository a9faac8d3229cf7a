"""Kernel resources and instruction counts of two builds of the same .hip files, side by side.

Each directory holds, per source file NAME, what
  hipcc <flags of ops/build.py> -Rpass-analysis=kernel-resource-usage --save-temps -c NAME.hip 2> NAME.remarks
leaves behind: NAME.remarks and NAME-hip-amdgcn-amd-amdhsa-gfx950.s.  Prints one markdown row per kernel
of the second directory (resources; 'same' or what differs from the first), then per kernel the
counts of the instruction classes that carry the memory and matrix work.

  python tools/probe/kernel_resources_diff.py PARENT_DIR NEW_DIR skinny_gemm skinny_w4
"""
import collections
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


def instr_counts(path):
    counts, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = counts.setdefault(m.group(1), collections.Counter())
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        op = line.strip().split(" ")[0].split("\t")[0]
        for c in CLASSES:
            if op.startswith(c):
                cur[c] += 1
    return counts


def main():
    a_dir, b_dir, names = sys.argv[1], sys.argv[2], sys.argv[3:]
    for name in names:
        ra, rb = resources(f"{a_dir}/{name}.remarks"), resources(f"{b_dir}/{name}.remarks")
        ia = instr_counts(f"{a_dir}/{name}-hip-amdgcn-amd-amdhsa-gfx950.s")
        ib = instr_counts(f"{b_dir}/{name}-hip-amdgcn-amd-amdhsa-gfx950.s")
        dm = demangle(sorted(set(ra) | set(rb)))
        print(f"\n## {name}.hip: {len(ra)} kernels in the parent, {len(rb)} in this tree")
        for k in ra:
            if k not in rb:
                print(f"removed: {dm[k]}")
        print("\n| kernel | " + " | ".join(FIELDS) + " | vs parent | " + " | ".join(CLASSES) + " | instructions vs parent |")
        print("|---|" + "---|" * (len(FIELDS) + len(CLASSES) + 2))
        worse = []
        for k, r in rb.items():
            p = ra.get(k)
            if p is None:
                vs = "new"
            else:
                d = [f"{f} {p[f]} -> {r[f]}" for f in FIELDS if p[f] != r[f]]
                vs = "; ".join(d) if d else "same"
                if any(p[f] != r[f] for f in MUST_MATCH):
                    worse.append(dm[k])
            cb, ca = ib.get(k, {}), ia.get(k, {})
            di = [f"{c} {ca.get(c, 0)} -> {cb.get(c, 0)}" for c in CLASSES if ca.get(c, 0) != cb.get(c, 0)]
            print(f"| {dm[k]} | " + " | ".join(str(r[f]) for f in FIELDS) + f" | {vs} | "
                  + " | ".join(str(cb.get(c, 0)) for c in CLASSES) + " | " + ("; ".join(di) if di else "same") + " |")
        if worse:
            print("\nspills / scratch / occupancy / LDS differ: " + ", ".join(worse))


if __name__ == "__main__":
    main()
