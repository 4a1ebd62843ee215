#!/usr/bin/env python3
"""Per-kernel table over one file of tools/isa_compare.sh's output: name, instructions, VGPR, AGPR, SGPR, scratch bytes, SGPR / VGPR spills,
static LDS bytes, and -- with the same file of another commit -- that commit's instructions and VGPRs and whether the kernel's code is identical.

    tools/isa_kernel_table.py <outdir>/default/pdmp_kernels.s [<other outdir>/default/pdmp_kernels.s] [--filter REGEX] [--demangle]

Reads only the code-object metadata and counts the lines of each kernel's body; it does not look at what the instructions are.
"""
import argparse
import re
import subprocess


def kernels(path):
    """{name: dict(instr=, body=, vgpr=, ...)} of one assembly file"""
    out, body, name = {}, None, None
    meta = {}
    cur = None
    for line in open(path):
        s = line.rstrip("\n")
        if body is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", s)
            if m and not m.group(1).startswith(".L") and not m.group(1).endswith(".kd"):
                name, body = m.group(1), []
        else:
            if s.startswith(".Lfunc_end"):
                out[name] = {"body": body}
                body = None
            else:
                t = s.split(";")[0].strip()
                if t:
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
        m = re.match(r"^\s+- \.agpr_count:\s+(\d+)", s)
        if m:
            cur = {"agpr": int(m.group(1))}
            continue
        if cur is not None:
            m = re.match(r"^\s+\.(\w+):\s+(\S+)", s)
            if m:
                cur[m.group(1)] = m.group(2)
                if m.group(1) == "wavefront_size":  # (the last key of a kernel's entry)
                    meta[cur.get("name")] = cur
                    cur = None
    for n, k in out.items():
        md = meta.get(n, {})
        k["instr"] = sum(1 for t in k["body"] if not t.startswith(".") and not t.endswith(":"))
        for key, src in (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"),
                         ("sspill", "sgpr_spill_count"), ("vspill", "vgpr_spill_count")):
            k[key] = int(md.get(src, -1))
        k["agpr"] = int(md.get("agpr", -1))
    return {n: k for n, k in out.items() if n in meta}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("other", nargs="?")
    ap.add_argument("--filter", default="")
    ap.add_argument("--demangle", action="store_true")
    a = ap.parse_args()
    mine = kernels(a.asm)
    theirs = kernels(a.other) if a.other else None
    names = [n for n in mine if re.search(a.filter, n)]
    shown = names
    if a.demangle:
        shown = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")[:len(names)]
    print("kernel | instr | vgpr | agpr | sgpr | scratch | spills s/v | static lds" + (" | other instr | other vgpr | code" if theirs is not None else ""))
    for n, label in zip(names, shown):
        k = mine[n]
        row = f"{label} | {k['instr']} | {k['vgpr']} | {k['agpr']} | {k['sgpr']} | {k['scratch']} | {k['sspill']}/{k['vspill']} | {k['lds']}"
        if theirs is not None:
            o = theirs.get(n)
            row += " | - | - | absent" if o is None else f" | {o['instr']} | {o['vgpr']} | {'identical' if o['body'] == k['body'] else 'differs'}"
        print(row)
    if theirs is not None:
        for n in theirs:
            if n not in mine and re.search(a.filter, n):
                print(f"{n} | only in {a.other}")


if __name__ == "__main__":
    main()
