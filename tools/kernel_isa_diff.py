#!/usr/bin/env python3
"""Compare the device assembly of two builds of lh_kernels.hip, function by function (no GPU needed).

Make each file with the flags of tools/kernel_resources.sh plus `--cuda-device-only -S`:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S lh_kernels.hip -o tree.s

    tools/kernel_isa_diff.py parent.s tree.s [--map names.txt] [--lines N]

A file is cut into functions at its `_Z...:` labels, each up to its `.Lfunc_end`; comments go, and the function's number goes from
its local labels (.LBB12_3 -> .LBB_3: the compiler numbers functions in the order it emits them).  Functions are paired by their
short name -- `k_trace_persist_stage<1,0,3>`: the mangled name without the namespace and the argument list -- or through the name
map: lines of `REGEX REPLACEMENT`, the first whose regex matches the whole of an OLD short name gives the new one (re.sub syntax).

Per function one of
    identical       the same instructions, the same kernel descriptor;
    kernarg only    the same number of instructions, and every line that differs is a scalar load from the kernarg segment pointer
                    with another offset -- or the one s_add_u32 of a constant to that pointer's low half, the address of the
                    implicit arguments behind the explicit ones -- (and the descriptor's .amdhsa_kernarg_size): the argument list
                    moved, the code did not;
    DIFFERS         with the first differing lines.
Exit status 1 if any function differs or has no partner."""
import argparse
import re
import sys

LABEL = re.compile(r"^(_Z\w+):")
LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+_(\d+)")
SLOAD = re.compile(r"^s_load_dword(?:x\d+)?\s+(\S+),\s*(s\[\d+:\d+\]),\s*(\S+)$")
SADD = re.compile(r"^s_add_u32\s+(\S+),\s*(s\d+),\s*(0x[0-9a-f]+|\d+)$")          # the address of the implicit arguments, behind the explicit ones


def short_name(mangled):
    """_ZN12_GLOBAL__N_121k_trace_persist_stageILi1ELb0ELi3EEEv... -> k_trace_persist_stage<1,0,3>"""
    s = mangled[2:]
    if s.startswith("N"):
        s = s[1:]
    name = None
    while s and s[0].isdigit():          # the nested names: the last one is the function's
        m = re.match(r"\d+", s)
        n = int(m.group())
        name, s = s[m.end():m.end() + n], s[m.end() + n:]
    if name is None:
        return mangled
    if s.startswith("I"):                 # template arguments: literals only (Lb1E, Li3E, Lin1E)
        args, s = [], s[1:]
        while s and s[0] == "L":
            m = re.match(r"L[a-z](n?)(\d+)E", s)
            if not m:
                return mangled
            args.append(("-" if m.group(1) else "") + m.group(2))
            s = s[m.end():]
        name += "<" + ",".join(args) + ">"
    return name


def functions(path):
    """short name -> (code lines, descriptor lines, the kernarg pointer's SGPR pair or None)"""
    out, cur, name = {}, None, None
    for raw in open(path):
        line = raw.split(";", 1)[0].strip()
        m = LABEL.match(raw)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is None or not line:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            code, desc, in_desc, user = [], [], False, {}
            for ln in cur:
                if ln.startswith(".amdhsa_kernel"):
                    in_desc = True
                    continue
                if ln.startswith(".end_amdhsa_kernel"):
                    in_desc = False
                    continue
                if in_desc:
                    desc.append(ln)
                    k = ln.split()
                    if k[0].startswith(".amdhsa_user_sgpr_"):
                        user[k[0]] = int(k[1], 0)
                elif not ln.startswith((".section", ".p2align", ".text", ".type", ".size", ".globl", ".weak", ".protected", ".hidden")):
                    code.append(LOCAL.sub(r".L\1_\2", ln).replace(name, "<self>"))
            base = None
            if user.get(".amdhsa_user_sgpr_kernarg_segment_ptr"):
                b = 2 * user.get(".amdhsa_user_sgpr_dispatch_ptr", 0) + 2 * user.get(".amdhsa_user_sgpr_queue_ptr", 0)
                base = "s[%d:%d]" % (b, b + 1)
            out[short_name(name)] = (code, desc, base)
            cur = None
            continue
        cur.append(line)
    return out


def compare(a, b):
    (ca, da, ka), (cb, db, kb) = a, b
    dd = [(x, y) for x, y in zip(da, db) if x != y]
    if ca == cb and da == db:
        return "identical", []
    diff = [(x, y) for x, y in zip(ca, cb) if x != y]
    if len(ca) == len(cb) and len(da) == len(db) and ka == kb and ka is not None:
        ok = all(x.split()[0] == ".amdhsa_kernarg_size" == y.split()[0] for x, y in dd)
        lo = ka[2:].split(":")[0]          # s[0:1] -> 0
        for x, y in diff:
            mx, my = SLOAD.match(x) or SADD.match(x), SLOAD.match(y) or SADD.match(y)
            ok = ok and bool(mx and my) and x.split()[0] == y.split()[0] and mx.group(1) == my.group(1) and mx.group(2) == my.group(2) and mx.group(2) in (ka, "s" + lo)
        if ok:
            return "kernarg only (%d lines)" % len(diff), []
    if len(ca) != len(cb):
        diff.append(("%d lines" % len(ca), "%d lines" % len(cb)))
    return "DIFFERS", diff + dd


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", help="name map: lines of `REGEX REPLACEMENT` from old short names to new ones")
    ap.add_argument("--lines", type=int, default=6, help="differing lines shown per function")
    args = ap.parse_args()
    rules = []
    if args.map:
        for ln in open(args.map):
            ln = ln.split("#", 1)[0].split()
            if len(ln) == 2:
                rules.append((re.compile(ln[0]), ln[1]))
    old, new = functions(args.old), functions(args.new)
    bad, seen = 0, set()
    for name in sorted(old):
        to = name
        for rx, rep in rules:
            if rx.fullmatch(name):
                to = rx.sub(rep, name)
                break
        arrow = name if to == name else "%s -> %s" % (name, to)
        if to not in new:
            print("%-72s NO PARTNER" % arrow)
            bad += 1
            continue
        seen.add(to)
        verdict, diff = compare(old[name], new[to])
        print("%-72s %s" % (arrow, verdict))
        if verdict == "DIFFERS":
            bad += 1
            for x, y in diff[:args.lines]:
                print("    - %s\n    + %s" % (x, y))
    for name in sorted(set(new) - seen):
        print("%-72s NEW, NO PARTNER" % name)
        bad += 1
    print("%d functions in %s, %d in %s, %d not accounted for" % (len(old), args.old, len(new), args.new, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
