"""Compare the gfx950 kernels of two builds of libmobody_hip.so: which kernels exist, and whether the common ones are the
same machine code with the same resources.  Needs only the LLVM tools of the ROCm install (no GPU).

usage: python tools/isa_diff.py A.so B.so [--rename 'REGEX=REPL' ...] [--list]

Prints the kernels only in A, only in B, and every common kernel whose disassembly or kernel-descriptor resources (VGPR,
AGPR, SGPR, scratch, LDS) differ; exits 1 on any difference among the common kernels.  Kernels are matched by demangled name.
A refactor that drops template parameters renames its kernels: RENAMES below maps the names of A (the older build) onto the
new ones, but only for the instances whose dropped arguments had the value the new code fixes -- the others stay "only in
A".  --rename adds regular-expression rules applied to the names of A after the table; --list also prints every matched name."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")

# kernel template -> (number of template arguments in A, {index of a dropped argument: the value it must have had})
RENAMES = {
    "k_mlp3_fwd": (4, {1: "1", 2: "1"}),         # <ACT, MT, RG, NT>               -> <ACT, NT>
    "k_mlp3_fwd2": (3, {1: "1"}),                # <ACT, MT, NT>                   -> <ACT, NT>
    "k_mlp3_fwd_bf": (7, {2: "1", 5: "1"}),      # <ACT, PM, RG, NT, DS, MT, NT2>  -> <ACT, PM, NT, DS, NT2>
    "k_mlp3_bwd": (5, {1: "1"}),                 # <DX, MT, NT, MASK, PM>          -> <DX, NT, MASK, PM>
}
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def short(dem):
    """'void mobody::k<1, 2>(mobody::Args)' -> 'k<1, 2>'"""
    dem = re.sub(r"^void ", "", dem).replace("mobody::", "")
    depth = 0
    for i, c in enumerate(dem):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return dem[:i]
    return dem


def table_rename(name):
    m = re.fullmatch(r"(\w+)<(.*)>", name)
    if not m or m.group(1) not in RENAMES:
        return name
    argc, dropped = RENAMES[m.group(1)]
    args = [a.strip() for a in m.group(2).split(",")]
    if len(args) != argc or any(args[i] != v for i, v in dropped.items()):
        return name
    return "%s<%s>" % (m.group(1), ", ".join(a for i, a in enumerate(args) if i not in dropped))


def kernels(lib, tmp):
    """{short demangled name: (resources dict, [instruction text])} over every gfx950 code object of the library"""
    lib = os.path.abspath(lib)
    work = tempfile.mkdtemp(dir=tmp)
    link = os.path.join(work, "lib.so")
    os.symlink(lib, link)
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", link, cwd=work)
    out = {}
    for f in sorted(os.listdir(work)):
        if "gfx950" not in f:
            continue
        co = os.path.join(work, f)
        res = {}
        notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
        for entry in re.split(r"\n  - (?=\.)", notes.split("amdhsa.kernels:")[1].split("\namdhsa.")[0])[1:]:
            sym = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M).group(1)
            res[sym] = {k: int(re.search(r"^\s*%s:\s+(\d+)" % re.escape(k), entry, re.M).group(1)) for k in RESOURCES}
        text = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co)
        cur = None
        code = {}
        for line in text.splitlines():
            m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
            if m:
                cur = code.setdefault(m.group(1), [])
            elif cur is not None and line.strip() and line.strip() != "...":
                # ("..." is the disassembler's mark for the zero padding between two functions, not an instruction: a kernel
                #  that gets a neighbour behind it would otherwise count one line more)
                # drop the address comment and symbolic branch targets (they carry the mangled name)
                cur.append(re.sub(r"\s*<[^>]*>", "", line.split("//")[0]).strip())
        # demangled names: the symbol table printed twice, plain and with -C, lines in the same order
        plain = run(os.path.join(LLVM, "llvm-objdump"), "-t", co).splitlines()
        dem = run(os.path.join(LLVM, "llvm-objdump"), "-t", "-C", co).splitlines()
        for lp, ld in zip(plain, dem):
            f = lp.split()
            if f and f[-1] in res:
                out[short(ld[lp.index(f[-1]):])] = (res[f[-1]], code.get(f[-1], []))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--list", action="store_true")
    o = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ka, kb = kernels(o.a, tmp), kernels(o.b, tmp)
    renamed = {}
    for name, v in ka.items():
        new = table_rename(name)
        for rule in o.rename:
            pat, repl = rule.split("=", 1)
            new = re.sub(pat, repl, new)
        if new in renamed:
            sys.exit("rename rule maps two kernels of A onto %s" % new)
        renamed[new] = (name, v)
    only_a = sorted(n for n in renamed if n not in kb)
    only_b = sorted(n for n in kb if n not in renamed)
    common = sorted(n for n in renamed if n in kb)
    print("A: %d kernels, B: %d kernels, matched: %d" % (len(ka), len(kb), len(common)))
    print("only in A (%d):" % len(only_a))
    for n in only_a:
        print("  " + n)
    print("only in B (%d):" % len(only_b))
    for n in only_b:
        print("  " + n)
    bad = 0
    for n in common:
        (old, (ra, ca)), (rb, cb) = renamed[n], kb[n]
        diffs = ["%s %d -> %d" % (k[1:], ra[k], rb[k]) for k in RESOURCES if ra[k] != rb[k]]
        if ca != cb:
            diffs.append("ISA differs: %d -> %d instructions" % (len(ca), len(cb)))
        if diffs:
            bad += 1
            print("DIFF %s%s: %s" % (n, "" if old == n else " (A: %s)" % old, "; ".join(diffs)))
        elif o.list:
            print("same %s%s" % (n, "" if old == n else " (A: %s)" % old))
    print("%d of %d matched kernels differ" % (bad, len(common)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
