#!/usr/bin/env python3
"""Compare the kernels of two `make asm` listings (build/engine_dispatch.s) instruction by instruction.

    python tools/asm_identity.py OLD.s NEW.s [REGEX]

Every kernel of OLD whose mangled name matches REGEX (default: the blind-rotation kernels) must exist in NEW with the same
instruction stream (assembler directives are not compared).  Local labels (.LBB<f>_<b>) are renumbered per kernel and comments dropped, so a kernel that only moved
within the file compares equal.  Prints one line per kernel that differs or is missing and exits 1 if there is any."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        code = line.split(";")[0].rstrip()
        if code.strip() and not (code.strip().startswith(".") and not code.endswith(":")):      # (directives: the kernel descriptor's
            body.append(code)                                                                 #  kernarg size grows with the arguments)
    for name, body in out.items():
        labels = {}
        for l in body:
            for lab in re.findall(r"\.LBB\d+_\d+", l):
                labels.setdefault(lab, f".L{len(labels)}")
        out[name] = [re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], l) for l in body]
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else r"blind_rotate_kernel")
    bad = 0
    names = [k for k in old if pat.search(k)]
    for k in names:
        if k not in new:
            print(f"missing: {k}")
            bad += 1
        elif new[k] != old[k]:
            diff = sum(a != b for a, b in zip(old[k], new[k])) + abs(len(old[k]) - len(new[k]))
            print(f"differs: {k} ({len(old[k])} vs {len(new[k])} lines, {diff} differ)")
            bad += 1
    print(f"{len(names) - bad} of {len(names)} kernels identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
