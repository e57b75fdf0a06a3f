#!/usr/bin/env python3
"""Per-kernel resource figures of a device assembly file, or the comparison of two (the table the profiles/rNN/resource_usage.txt files hold).

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form --cuda-device-only -S -o this.s robust-nonlinear-mpc_amd/csrc/slsqp_api.hip
    python scripts/kernel_resources.py this.s                # every kernel
    python scripts/kernel_resources.py parent.s this.s       # same / differs / new / gone, matched by kernel name

Figures: each kernel's .amdgpu_metadata entry and its '; Occupancy:' line (what -Rpass-analysis=kernel-resource-usage prints).
Columns: SGPRs VGPRs AGPRs scratch[B/lane] dynamic-stack occupancy[waves/SIMD] SGPR-spill VGPR-spill LDS[B/block]."""
import re
import subprocess
import sys

KEYS = (".sgpr_count", ".vgpr_count", ".agpr_count", ".private_segment_fixed_size", ".uses_dynamic_stack", None, ".sgpr_spill_count", ".vgpr_spill_count",
        ".group_segment_fixed_size")


def read(path):
    occ, cur, meta, ent = {}, None, {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"^(\w+):\s+; @", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"^; Occupancy: (\d+)", line)
        if m and cur:
            occ[cur] = m.group(1)
            continue
        if line.startswith("  - .agpr_count:") or line.startswith("  - .args:"):
            ent = {}
        m = re.match(r"^(?:  - |    )(\.\w+):\s+(\S+)\s*$", line)
        if m and ent is not None:
            ent[m.group(1)] = m.group(2)
            if m.group(1) == ".wavefront_size" and ".name" in ent:
                meta[ent[".name"]] = ent
                ent = None
    out = {}
    for name, e in meta.items():
        out[name] = " ".join(occ.get(name, "?") if k is None else {"false": "False", "true": "True"}.get(e.get(k, "?"), e.get(k, "?")) for k in KEYS)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)).replace("slsqp::", "") for n, d in zip(names, r)}
    except Exception:
        return {n: n for n in names}


def main(argv):
    if len(argv) == 2:
        t = read(argv[1])
        nm = demangle(sorted(t))
        for n in sorted(t, key=lambda n: nm[n]):
            print(f"{nm[n]:70s} {t[n]}   {n}")
        return 0
    a, b = read(argv[1]), read(argv[2])
    nm = demangle(sorted(set(a) | set(b)))
    same = [n for n in a if n in b and a[n] == b[n]]
    diff = [n for n in a if n in b and a[n] != b[n]]
    new, gone = [n for n in b if n not in a], [n for n in a if n not in b]
    print(f"# {len(a)} kernels before, {len(b)} now: {len(same)} same, {len(diff)} differing, {len(new)} new, {len(gone)} gone")
    for n in sorted(set(a) | set(b), key=lambda n: nm[n]):
        if n in same:
            print(f"same     {nm[n]:66s} {a[n]}   {n}")
        elif n in diff:
            print(f"differs  {nm[n]:66s} {a[n]}  ->  {b[n]}   {n}")
        elif n in new:
            print(f"new      {nm[n]:66s} {b[n]}   {n}")
        else:
            print(f"gone     {nm[n]:66s} {a[n]}   {n}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
