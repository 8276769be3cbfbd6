#!/usr/bin/env python3
"""Compare the kernel bodies of two sets of device assembly listings (`make asm` output).

    isa_compare.py [--rename REGEX=REPL ...] OLD.s NEW.s [MORE_NEW.s ...]

The first file is one side; every further file is concatenated into the other side (a unit that was
split into several).  A kernel is a symbol with a `.amdhsa_kernel NAME` descriptor; its body runs
from its `NAME:` label to the next `.Lfunc_end` label.  Before comparing, basic-block labels
`BB<f>_<n>` (f numbers the function within its unit) become `BB_<n>`, trailing `;` comments go, and
blank lines go.  `--rename REGEX=REPL` (any number) rewrites the old side's symbol names with
re.sub, wherever they stand, before anything is matched (the argument is split at its first `=`, so
REGEX holds none): a kernel whose template argument list lost an entry then still compares body
against body.  Text only: the script knows nothing about what the lines mean.

Prints the kernel counts, the symbols on one side only and the symbols whose bodies differ;
exit status 1 on any of the latter two.
"""
import re
import sys

_BB = re.compile(r"BB\d+_(\d+)\b")


def kernels(paths, renames=()):
    lines = []
    for p in paths:
        with open(p, errors="replace") as f:
            lines += f.read().splitlines()
    for pat, repl in renames:
        lines = [pat.sub(repl, l) for l in lines]
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    out, cur, body = {}, None, None
    for l in lines:
        if cur is None:
            m = re.match(r"(\S+):", l)
            if m and m.group(1) in names and m.group(1) not in out:
                cur, body = m.group(1), []
            continue
        if l.startswith(".Lfunc_end"):
            out[cur], cur = body, None
            continue
        l = _BB.sub(r"BB_\1", l.split(";", 1)[0].rstrip())
        if l:
            body.append(l)
    missing = names - set(out)
    if missing:
        sys.exit(f"no body found for: {sorted(missing)}")
    return out


def main(argv):
    renames = []
    while len(argv) > 2 and argv[1] == "--rename":
        pat, sep, repl = argv[2].partition("=")
        if not sep:
            sys.exit("--rename takes REGEX=REPL")
        renames.append((re.compile(pat), repl))
        del argv[1:3]
    if len(argv) < 3:
        sys.exit(__doc__)
    old, new = kernels(argv[1:2], renames), kernels(argv[2:])
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    print(f"kernels: {len(old)} old, {len(new)} new")
    print(f"only in old: {len(only_old)}")
    for k in only_old:
        print(f"  {k}")
    print(f"only in new: {len(only_new)}")
    for k in only_new:
        print(f"  {k}")
    print(f"bodies that differ: {len(differ)}")
    for k in differ:
        print(f"  {k} ({len(old[k])} vs {len(new[k])} lines)")
    return 1 if (only_old or only_new or differ) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
