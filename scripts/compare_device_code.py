#!/usr/bin/env python3
"""Device code of two builds of the library, symbol by symbol:
    python scripts/compare_device_code.py <parent libmigan_hip.so> <branch libmigan_hip.so>
Unbundles and disassembles both with mi-gan_amd/isa_lint.py's `unbundle`, strips addresses, encodings and trailing padding, and prints,
for every symbol whose body differs, both instruction counts, whether the opcode multisets agree, the position of the first s_barrier
and every differing line (unified diff, no context).  Exit status 0 when the two libraries hold the same symbols with identical bodies."""
import collections
import difflib
import importlib.util
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bodies(lib):
    spec = importlib.util.spec_from_file_location("migan_isa_lint", os.path.join(ROOT, "mi-gan_amd", "isa_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for _, text in lint.unbundle(lib, tmp, disassemble=True):
            cur = None
            for line in text.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                    continue
                if cur is None or not line.startswith("\t"):
                    continue
                ins = line.split("//")[0].strip()                    # drop "// address: encoding"
                ins = re.sub(r"<\S+\+0x[0-9a-f]+>", "<L>", ins)      # branch targets are printed as symbol + offset
                if ins:
                    cur.append(ins)
    for body in out.values():
        while body and body[-1] in ("s_nop 0", "s_code_end"):        # trailing padding
            body.pop()
    return out


def main(parent, branch):
    a, b = bodies(parent), bodies(branch)
    print(f"{len(a)} symbols in the parent, {len(b)} in the branch, same names: {set(a) == set(b)}; "
          f"{sum(len(v) for v in a.values())} / {sum(len(v) for v in b.values())} instructions")
    differ = 0
    for k in sorted(set(a) & set(b)):
        if a[k] == b[k]:
            continue
        differ += 1
        ops = collections.Counter(l.split()[0] for l in a[k]) == collections.Counter(l.split()[0] for l in b[k])
        bar = next((i for i, l in enumerate(a[k]) if l.startswith("s_barrier")), None)
        print(f"DIFFERS {k}: {len(a[k])} / {len(b[k])} instructions, same opcode multiset {ops}, first s_barrier at {bar}")
        for line in difflib.unified_diff(a[k], b[k], "parent", "branch", n=0, lineterm=""):
            print("    " + line)
    print(f"{differ} symbols differ")
    return 0 if set(a) == set(b) and differ == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
