#!/usr/bin/env python
"""Compare the packed-form instantiations of duo_decode_scan_kernel in two assembly listings of duo_decode.hip.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S duo_decode.hip -o new.s     (same for the old tree)
    python tools/debug/decode_asm_diff.py old.s new.s

Per <GT, NT, FUSED>: the instruction streams (comments dropped, mangled names and label numbers normalised) must be
identical, as must .amdhsa_next_free_vgpr; every kernel of the new listing must have a private segment of 0 bytes."""
import re
import sys

KERNEL = re.compile(r"^(_Z\w*duo_decode\w*):")
ARGS = re.compile(r"duo_decode_scan_kernelILi(\d)ELb([01])ELb([01])E(?:Lb([01])E)?E")


def kernels(path):
    """mangled name -> (instruction lines, {amdhsa field: value})"""
    out, name, body = {}, None, None
    for line in open(path):
        m = KERNEL.match(line)
        if m:
            name, body = m.group(1), []
            out[name] = [body, {}]
        elif line.startswith(".Lfunc_end"):
            body = None
        elif body is not None:
            text = line.split(";")[0].strip()
            if text and not text.startswith(".p2align"):
                body.append(text)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size)\s+(\d+)", line)
        if m and name in out:
            out[name][1][m.group(1)] = int(m.group(2))
    return out


def normalised(name, body):
    labels = {}
    def lab(m):
        return ".L%d" % labels.setdefault(m.group(0), len(labels))
    return [re.sub(r"\.LBB\d+_\d+", lab, t.replace(name, "KERNEL")) for t in body]


def packed(ks):
    """(GT, NT, FUSED) -> name, for the scan kernel's packed form (the old listing has no WIDE parameter)"""
    res = {}
    for n in ks:
        m = ARGS.search(n)
        if m and m.group(4) in (None, "0"):
            res[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = n
    return res


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
po, pn = packed(old), packed(new)
bad = sorted(set(po) ^ set(pn))
for key in sorted(set(po) & set(pn)):
    a, b = old[po[key]], new[pn[key]]
    same = normalised(po[key], a[0]) == normalised(pn[key], b[0])
    regs = a[1]["next_free_vgpr"] == b[1]["next_free_vgpr"]
    print("GT=%d NT=%d FUSED=%d: %5d instructions %s, next_free_vgpr %d -> %d" % (
        *key, len(b[0]), "identical" if same else "DIFFER", a[1]["next_free_vgpr"], b[1]["next_free_vgpr"]))
    if not (same and regs):
        bad.append(key)
scratch = {n: k[1]["private_segment_fixed_size"] for n, k in new.items() if k[1].get("private_segment_fixed_size")}
print("%d kernels in the old listing, %d in the new; kernels with scratch in the new one: %s" % (len(old), len(new), scratch or "none"))
sys.exit(1 if bad or scratch or len(pn) != 12 else 0)
