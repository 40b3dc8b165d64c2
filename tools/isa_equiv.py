#!/usr/bin/env python3
"""Compare two gfx950 assembly listings function by function.

Answers "did this refactor change the machine code of any kernel?" without
a GPU. Produce the listings from two trees with the same command, e.g.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S \\
    -fno-gpu-rdc -D__HIP_PLATFORM_AMD__=1 -DUSE_ROCM=1 \\
    -DTORCH_EXTENSION_NAME=_kakveda_hip <torch + python includes> \\
    kakveda_amd/ops/hip/kakveda_kernels.hip -o X.s

then:  python tools/isa_equiv.py OLD.s NEW.s

Each function body (kernels and __noinline__ device functions) is compared
after normalising what legitimately moves when other functions come or go:
basic-block and .Lfunc_* label numbers and assembler comments. Per symbol
the tool prints `identical`, or a unified diff; a kernel's descriptor
(.amdhsa_* directives) is compared apart from its instructions and changed
directives are listed, next to the old and new .vgpr_count /
.vgpr_spill_count / .private_segment_fixed_size / .group_segment_fixed_size
metadata. A symbol whose code differs also says whether the instructions per
mnemonic are the same (`DIFFERS (same instruction mix, N)`: only operands,
such as kernarg offsets and register numbers, or the order moved) or which
counts changed (`DIFFERS (v_cndmask_b32 40->24; ...)`). Exit status is 1
when a symbol present in both listings differs in code.

--alias 'REGEX=REPL' rewrites symbol names (in both listings, everywhere)
before matching, for a refactor that changes a mangled name on purpose, e.g.
a dropped defaulted template parameter:
  --alias 'cosine_topk_partial_tILi(\\d+)ELi2EE=cosine_topk_partial_tILi\\1EE'
or the routed scans, whose filtered twins became `template <bool FILTER>`
instantiations (old name, then new name, onto one readable name):
  --alias '_ZN7kakveda\\d+(ivf_scan_[a-z]+)_kernelE\\w+=\\1_kernel<false>'
  --alias '_ZN7kakveda\\d+(ivf_scan_[a-z]+)_filtered_kernelE\\w+=\\1_kernel<true>'
  --alias '_ZN7kakveda\\d+(ivf_scan_[a-z]+)_kernelILb0EEEv\\w+=\\1_kernel<false>'
  --alias '_ZN7kakveda\\d+(ivf_scan_[a-z]+)_kernelILb1EEEv\\w+=\\1_kernel<true>'
"""

import argparse
import collections
import difflib
import re
import sys

META_KEYS = (
    ".vgpr_count",
    ".vgpr_spill_count",
    ".private_segment_fixed_size",
    ".group_segment_fixed_size",
)

_TYPE_FN = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
_FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
_RODATA = re.compile(r"^\s*\.section\s+\.rodata")
_LABEL = re.compile(r"\.L(?:BB\d+_\d+|func_(?:begin|end)\d+|tmp\d+)")


def _normalise(lines):
    """Drop comments/blank lines; renumber local labels by first appearance."""
    names = {}
    out = []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        line = _LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line)
        out.append(re.sub(r"\s+", " ", line.strip()))
    return out


def parse(path, aliases):
    text = open(path, encoding="utf-8", errors="replace").read()
    for pat, repl in aliases:
        text = pat.sub(repl, text)
    lines = text.split("\n")
    funcs, order = {}, []
    sym, body = None, None
    for line in lines:
        m = _TYPE_FN.match(line)
        if m and body is None:
            sym = m.group(1)
            continue
        if sym is not None and body is None and line.startswith(sym + ":"):
            body = []
            continue
        if body is not None:
            if _FUNC_END.match(line):
                # a kernel's descriptor (.amdhsa_* directives) sits between
                # its last instruction and .Lfunc_end: compare it apart
                cut = next((i for i, l in enumerate(body) if _RODATA.match(l)), len(body))
                funcs[sym] = (_normalise(body[:cut]), _normalise(body[cut:]))
                order.append(sym)
                sym, body = None, None
            else:
                body.append(line)
    # kernel metadata (the YAML note at the end of the listing)
    meta = {}
    for entry in re.split(r"\n\s+- (?=\.)", text):
        s = re.search(r"\.symbol:\s+(\S+)\.kd", entry)
        if not s:
            continue
        vals = {}
        for key in META_KEYS:
            v = re.search(re.escape(key) + r":\s+(\d+)", entry)
            vals[key] = int(v.group(1)) if v else None
        meta[s.group(1)] = vals
    return funcs, order, meta


def mix(code):
    """Instructions per mnemonic of a normalised body (labels, directives out)."""
    return collections.Counter(
        l.split()[0] for l in code if not l.startswith(".") and not l.endswith(":"))


def short(sym, width=64):
    """Readable name: strip the mangling prefix/suffix where it is obvious."""
    m = re.match(r"_ZN\d+[a-z_]+?(\d+)", sym)
    if m:
        n = int(m.group(1))
        name, rest = sym[m.end() : m.end() + n], sym[m.end() + n :]
        t = re.match(r"IL([ib])(\d+)E", rest)
        if t:
            name += "<%s>" % (t.group(2) if t.group(1) == "i" else ("false", "true")[int(t.group(2)) != 0])
        return name
    return sym if len(sym) <= width else sym[: width - 3] + "..."


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--alias", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--max-diff-lines", type=int, default=60)
    args = ap.parse_args()
    aliases = []
    for a in args.alias:
        pat, _, repl = a.partition("=")
        aliases.append((re.compile(pat), repl))

    of, oorder, ometa = parse(args.old, aliases)
    nf, norder, nmeta = parse(args.new, aliases)
    rows, differs = [], 0
    for sym in oorder + [s for s in norder if s not in of]:
        om, nm = ometa.get(sym), nmeta.get(sym)
        fmt = lambda m: "/".join("-" if m is None or m[k] is None else str(m[k]) for k in META_KEYS)
        if sym not in nf:
            rows.append((short(sym), "removed", fmt(om), "-"))
            continue
        if sym not in of:
            rows.append((short(sym), "added", "-", fmt(nm)))
            continue
        (ocode, odesc), (ncode, ndesc) = of[sym], nf[sym]
        if ocode == ncode:
            verdict = "identical"
        else:
            differs += 1
            omix, nmix = mix(ocode), mix(ncode)
            moved = ["%s %d->%d" % (m, omix[m], nmix[m])
                     for m in sorted(set(omix) | set(nmix)) if omix[m] != nmix[m]]
            verdict = "DIFFERS (%s)" % ("; ".join(moved) if moved else
                                        "same instruction mix, %d" % sum(nmix.values()))
            diff = list(difflib.unified_diff(ocode, ncode, "old", "new", lineterm="", n=2))
            print("=== %s: code differs (%d -> %d lines)" % (short(sym), len(ocode), len(ncode)))
            for line in diff[: args.max_diff_lines]:
                print("    " + line)
            if len(diff) > args.max_diff_lines:
                print("    ... %d more diff lines" % (len(diff) - args.max_diff_lines))
        if odesc != ndesc:
            changed = [l[1:] for l in difflib.unified_diff(odesc, ndesc, lineterm="", n=0)
                       if l[:1] == "+" and l[:3] != "+++"]
            verdict += "; descriptor: " + ", ".join("`%s`" % c for c in changed)
        rows.append((short(sym), verdict, fmt(om), fmt(nm)))

    print("| symbol | code | old vgpr/spill/scratch/lds | new vgpr/spill/scratch/lds |")
    print("|---|---|---|---|")
    for r in rows:
        print("| `%s` | %s | %s | %s |" % r)
    kept = sum(1 for r in rows if r[1].startswith("identical"))
    print("\n%d identical, %d differ, %d removed, %d added"
          % (kept, differs, sum(r[1] == "removed" for r in rows), sum(r[1] == "added" for r in rows)))
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
