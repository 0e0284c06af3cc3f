#!/usr/bin/env python3
"""Compare the gfx950 code of two builds, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function --cuda-device-only -S \
        csrc/conv_igemm.hip -o new.s          (and the same at the other commit -> old.s)
    python tools/isa_diff.py old.s new.s
    python tools/isa_diff.py old.s -- conv_igemm.s conv_winograd.s conv_bf16.s conv_dgrad.s pool.s

Either side may be several files, the two sides separated by `--` (a unit that was split, or merged): a side is the union
of its files' kernel symbols, and a symbol that two files of one side define is an error.

For a refactor that must not change code generation.  Per kernel symbol it checks
  * the code-object metadata (VGPR / SGPR / AGPR counts, LDS and scratch bytes, spill counts),
  * the multiset of instruction mnemonics,
  * the instruction stream, line by line; differing lines are classified as an operand swap of one instruction
    (same mnemonic, same operands in another order), a register rename (same mnemonic, operands equal once
    register numbers are blanked), MOVED (the same text at another position: a reordering) or OTHER,
  * the text of every loop (from a label to the last backward branch to it) on its own.
Exit status 0: same symbols, metadata, mnemonics and loop text, and no MOVED or OTHER line (swaps and renames pass).
"""
import collections
import difflib
import re
import sys

META_KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".vgpr_spill_count", ".sgpr_spill_count")


def parse(path):
    """-> ({kernel: [instruction / label lines]}, {kernel: {key: value}})"""
    lines = open(path).read().split("\n")
    bodies, cur = {}, None
    for ln in lines:
        s = ln.split(";")[0].strip()
        m = re.match(r"^(\w+):", s)
        if m and not s.startswith(".L") and cur is None and m.group(1).startswith("_Z"):
            cur = m.group(1)
            bodies[cur] = []
            continue
        if cur is None:
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        elif s and (not s.startswith(".") or s.startswith(".LBB")):
            # (labels carry the function's position in the file: .LBB<function>_<block>)
            bodies[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)))
    meta = {}
    text = "\n".join(lines)
    start = text.find("amdhsa.kernels:")
    for chunk in re.split(r"\n  - ", text[start:])[1:]:
        name = re.search(r"^ {4}\.name:\s+(\S+)", chunk, re.M)
        if not name:
            continue
        vals = {}
        for k in META_KEYS:
            v = re.search(r"^ {2,4}" + re.escape(k) + r":\s+(\S+)", "    " + chunk, re.M)
            vals[k] = v.group(1) if v else None
        meta[name.group(1)] = vals
    return {k: v for k, v in bodies.items() if k in meta}, meta   # (data symbols have a label too)


def mnemonic(line):
    return line.split(" ", 1)[0]


def operands(line):
    parts = line.split(" ", 1)
    return [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []


def blank_regs(line):
    return re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", line)


def loop_lines(body):
    """indices of the lines inside loops: from a label to the last backward branch that targets it"""
    where = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    inside = set()
    for i, l in enumerate(body):
        if l.startswith(("s_cbranch", "s_branch")):
            tgt = l.split()[-1]
            if tgt in where and where[tgt] < i:
                inside.update(range(where[tgt], i + 1))
    return inside


def classify(a, b):
    if mnemonic(a) != mnemonic(b):
        return "other"
    if sorted(operands(a)) == sorted(operands(b)):
        return "operand swap"
    if blank_regs(a) == blank_regs(b):
        return "register rename"
    if sorted(operands(blank_regs(a))) == sorted(operands(blank_regs(b))):
        return "operand swap + register rename"
    return "other"


def parse_side(paths):
    """the union of the kernels of several files; a kernel that two of them define is an error"""
    bodies, meta = {}, {}
    for path in paths:
        b, m = parse(path)
        twice = sorted((set(b) & set(bodies)) | (set(m) & set(meta)))
        if twice:
            sys.exit("%s: defined in another file of the same side too: %s" % (path, twice))
        bodies.update(b)
        meta.update(m)
    return bodies, meta


def main():
    args = sys.argv[1:]
    if "--" in args:
        olds, news = args[:args.index("--")], args[args.index("--") + 1:]
    else:
        olds, news = args[:1], args[1:]
    if not olds or not news or (("--" not in args) and len(args) != 2):
        sys.exit(__doc__)
    old_b, old_m = parse_side(olds)
    new_b, new_m = parse_side(news)
    bad = False
    if set(old_b) != set(new_b) or set(old_m) != set(new_m):
        print("SYMBOLS DIFFER:", sorted(set(old_b) ^ set(new_b)), sorted(set(old_m) ^ set(new_m)))
        bad = True
    print("%d kernel symbols in each file" % len(old_b))
    total = collections.Counter()
    for k in sorted(set(old_b) & set(new_b)):
        a, b = old_b[k], new_b[k]
        notes = []
        if old_m.get(k) != new_m.get(k):
            notes.append("METADATA %s -> %s" % (old_m.get(k), new_m.get(k)))
            bad = True
        ca = collections.Counter(mnemonic(l) for l in a if not l.endswith(":"))
        cb = collections.Counter(mnemonic(l) for l in b if not l.endswith(":"))
        if ca != cb:
            notes.append("MNEMONICS -%s +%s" % (dict(ca - cb), dict(cb - ca)))
            bad = True
        la, lb = loop_lines(a), loop_lines(b)
        if [a[i] for i in sorted(la)] != [b[i] for i in sorted(lb)]:
            notes.append("LOOP TEXT DIFFERS")
            bad = True
        kinds = collections.Counter()
        if a != b:
            gone, come = collections.Counter(), collections.Counter()   # lines with no partner at their position
            for op, i0, i1, j0, j1 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
                if op == "equal":
                    continue
                if op == "replace" and i1 - i0 == j1 - j0:
                    for x, y in zip(a[i0:i1], b[j0:j1]):
                        kind = classify(x, y)
                        if kind == "other":
                            gone[x] += 1
                            come[y] += 1
                        else:
                            kinds[kind] += 1
                else:
                    gone.update(a[i0:i1])
                    come.update(b[j0:j1])
            moved = sum((gone & come).values())      # the same text, registers included, at another position
            other = max(sum(gone.values()), sum(come.values())) - moved
            if moved:
                kinds["moved"] = moved
            if other:
                kinds["other"] = other
            if moved or other:
                bad = True
        total.update(kinds)
        m = new_m.get(k) or {}
        print("%-90s %5d instr, %4d in loops, vgpr %s sgpr %s agpr %s lds %s : %s" % (
            k, sum(cb.values()), len(lb), m.get(".vgpr_count"), m.get(".sgpr_count"), m.get(".agpr_count"),
            m.get(".group_segment_fixed_size"),
            "; ".join(notes + ["%d x %s" % (n, kind) for kind, n in sorted(kinds.items())]) or "identical"))
    print("differing lines by kind:", dict(total) or "none")
    print("FAIL" if bad else "OK")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
