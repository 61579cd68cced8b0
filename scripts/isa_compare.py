#!/usr/bin/env python3
"""Compare two device assembly listings of renderer.hip kernel by kernel (text only).

usage: isa_compare.py OLD.s NEW.s        (each made with the Makefile's FLAGS plus --cuda-device-only -S)

Per kernel: whether the instruction streams are identical (comments, .loc / .file / .cfi lines
dropped, the per-function label numbers normalised), the instruction counts, and VGPRs,
accumulation offset, LDS bytes, scratch bytes and SGPR / VGPR spills of both listings."""
import re
import subprocess
import sys

META = (".vgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_spill_count")


def kernels(path):
    text = open(path).read()
    out = {}
    for blk in re.split(r"\n  - (?=\.agpr_count:)", text.split(".amdgpu_metadata")[1])[1:]:   # the YAML record per kernel
        f = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)$", blk, re.M))
        out[f[".name"]] = {"meta": [int(f[k]) for k in META]}
    for name, k in out.items():
        body = text[re.search(rf"^{re.escape(name)}:", text, re.M).start():]
        body = body[:re.search(r"\n\.Lfunc_end\d+:", body).start()]
        ins = []
        for line in body.split("\n")[1:]:
            line = re.sub(r"\.L(BB|JTI|tmp|func_end)\d+_?", r".L\1_", line.split(";")[0]).strip()
            if line and not re.match(r"\.(loc|file|cfi_)", line):
                ins.append(line)
        k["text"] = ins
        k["count"] = sum(1 for l in ins if not l.endswith(":") and not l.startswith("."))
        k["accum"] = int(re.search(rf"\.amdhsa_kernel {re.escape(name)}\n(?:.*\n)*?\s+\.amdhsa_accum_offset (\d+)", text).group(1))
    return out


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    names = sorted(set(old) | set(new))
    nice = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    print(f"{len(old)} kernels in {old_path}, {len(new)} in {new_path}; columns old -> new")
    print(f"{'kernel':<64} {'stream':<9} {'instr':>13} {'diff':>5}  vgpr accum lds scratch sgpr_spill vgpr_spill")
    worst = 0
    for name, label in zip(names, nice):
        label = re.sub(r"^void |\(.*$", "", label)
        if name not in old or name not in new:
            print(f"{label:<64} only in {'old' if name in old else 'new'}")
            continue
        a, b = old[name], new[name]
        same = a["text"] == b["text"]
        res = lambda k: "/".join(str(v) for v in k["meta"][:1] + [k["accum"]] + k["meta"][1:])
        worst = max(worst, abs(b["count"] - a["count"]))
        print(f"{label:<64} {'identical' if same else 'differs':<9} {a['count']:>6}->{b['count']:<6} {b['count'] - a['count']:>+5}  "
              f"{res(a)}" + ("  =" if res(a) == res(b) else f" -> {res(b)}"))
    print(f"largest instruction-count difference: {worst}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
