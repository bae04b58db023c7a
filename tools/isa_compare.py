#!/usr/bin/env python3
"""Development tool (no GPU): compare the gfx950 device assembly of two builds of one source, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only OLD/suffix_attn.hip -o old.s   (likewise new.s)
    python tools/isa_compare.py old.s new.s [--rename 'REGEX=REPLACEMENT' ...]

A kernel = its label up to s_endpgm plus its .amdhsa_kernel descriptor and its metadata block; lines that carry the per-compile
`__hip_cuid_` symbol are dropped.  --rename maps an old mangled name onto the new one (a dropped template parameter) before
names are matched.  Prints one markdown row per kernel: identical, or old/new instruction count, VGPRs, SGPRs, global_load
count, `s_waitcnt vmcnt` count (whole kernel / inside the key loops, i.e. between a backward-branch target and its branch)."""
import argparse
import re
import sys


def kernels(path, renames):
    text = "".join(ln for ln in open(path) if "__hip_cuid_" not in ln)
    meta = {re.search(r"\.name:\s+(\S+)", blk).group(1): blk.split("\n...")[0] for blk in text.split("  - .agpr_count:")[1:]}
    out = {}
    for m in re.finditer(r"^(_ZN3hyd\w+):[^\n]*\n(.*?s_endpgm)\n.*?\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, flags=re.S | re.M):
        name, body, desc = m.groups()
        new = name
        for pat, rep in renames:
            new = re.sub(pat, rep, new)
        out[new] = (body.replace(name, new), desc + meta[name].replace(name, new))
    return out


def stats(body, desc):
    ins = [ln.split(";")[0].strip() for ln in body.splitlines()]
    ins = [i for i in ins if i and not i.startswith((".", ";")) and not i.endswith(":")]
    # key loops: from a label that a later s_cbranch jumps back to, up to that branch
    lines = body.splitlines()
    labels = {ln.split(":")[0].strip(): i for i, ln in enumerate(lines) if re.match(r"^\.LBB\w+:", ln)}
    inloop = set()
    for i, ln in enumerate(lines):
        m = re.search(r"s_cbranch_\w+ (\.LBB\w+)", ln)
        if m and labels.get(m.group(1), i) < i:
            inloop.update(range(labels[m.group(1)], i + 1))
    loop = [lines[i].split(";")[0] for i in sorted(inloop)]
    return dict(insts=len(ins), vgpr=int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)),
                sgpr=int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", desc).group(1)),
                scratch=int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)),
                gload=sum("global_load" in i for i in ins), vmcnt=sum("vmcnt" in i for i in ins),
                loop_gload=sum("global_load" in i for i in loop), loop_vmcnt=sum("vmcnt" in i for i in loop))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[])
    a = ap.parse_args()
    old = kernels(a.old, [r.split("=", 1) for r in a.rename])
    new = kernels(a.new, [])
    print(f"{len(old)} kernels old, {len(new)} new; only old: {sorted(set(old) - set(new))}; only new: {sorted(set(new) - set(old))}\n")
    print("| kernel | result | instructions | VGPRs | SGPRs | scratch | global_load (in loops) | s_waitcnt vmcnt (in loops) |")
    print("|---|---|---|---|---|---|---|---|")
    same = 0
    for k in sorted(set(old) & set(new)):
        if old[k] == new[k]:
            same += 1
            print(f"| `{k}` | identical | | | | | | |")
            continue
        o, n = stats(*old[k]), stats(*new[k])
        print(f"| `{k}` | differs | {o['insts']} / {n['insts']} | {o['vgpr']} / {n['vgpr']} | {o['sgpr']} / {n['sgpr']} | {o['scratch']} / {n['scratch']} | "
              f"{o['gload']} ({o['loop_gload']}) / {n['gload']} ({n['loop_gload']}) | {o['vmcnt']} ({o['loop_vmcnt']}) / {n['vmcnt']} ({n['loop_vmcnt']}) |")
    print(f"\n{same} of {len(set(old) & set(new))} identical")
    return 0 if same == len(old) == len(new) else 1


if __name__ == "__main__":
    sys.exit(main())
