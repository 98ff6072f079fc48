#!/usr/bin/env python3
"""Compare the device kernels of two builds of one HIP source, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S old/duo_int4.hip -o old.s      (and new.s)
    python tools/isa_compare.py old.s new.s [--map 'REGEX=REPLACEMENT' ...]

The method of profiles/int4_variant_prune.md: per kernel, the text between its label and `.Lfunc_end`, comments and
`.loc` / `.file` lines stripped, `.LBB<n>_` label prefixes normalised, the kernel's own mangled name replaced by a placeholder;
the `.amdhsa_*` descriptor block and the `.set <kernel>.<resource>` lines are compared separately.  `--map` renames kernels
of the NEW file before pairing (a kernel that gained a template parameter has another mangled name)."""
import re
import sys


def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path):
        line = line.rstrip("\n")
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                i0 = next(i for i, x in enumerate(cur) if ".amdhsa_kernel" in x)
                i1 = next(i for i, x in enumerate(cur) if ".end_amdhsa_kernel" in x)
                out[name] = [cur[:i0] + cur[i1 + 1:], cur[i0:i1 + 1]]
                cur = None
                continue
            line = re.sub(r";.*", "", line).rstrip()
            if not line.strip() or line.strip().startswith((".loc", ".file", ".cfi")):
                continue
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", line).replace(name, "KERNEL"))
            continue
        m = re.match(r"^\s*\.set (_Z\w+)\.(\w+), (.*)", line)
        if m and m.group(1) in out:
            out[m.group(1)][1].append(f"{m.group(2)} = {m.group(3).replace(m.group(1), 'KERNEL')}")
    return out


def main():
    maps = [a.split("=", 1) for i, a in enumerate(sys.argv) if sys.argv[i - 1] == "--map"]
    paths = [a for i, a in enumerate(sys.argv[1:], 1) if a != "--map" and sys.argv[i - 1] != "--map"]
    old, new = kernels(paths[0]), kernels(paths[1])

    def renamed(n):
        for pat, repl in maps:
            n = re.sub(pat, repl, n)
        return n

    new = {renamed(n): v for n, v in new.items()}
    same = True
    for n, (body, desc) in sorted(old.items()):
        if n not in new:
            print(f"{n}: MISSING in the new build")
            same = False
            continue
        b, d = new[n]
        ok_b, ok_d = body == b, desc == d
        same &= ok_b and ok_d
        print(f"{n}: {len(body)} / {len(b)} lines, body {'identical' if ok_b else 'DIFFERENT'}, "
              f"descriptor {'identical' if ok_d else 'DIFFERENT'}")
    for n in sorted(set(new) - set(old)):
        print(f"{n}: NEW, {len(new[n][0])} lines")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
