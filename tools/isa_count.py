"""Static instruction counts of gfx950 kernels, by class (hipcc -S --cuda-device-only: no GPU needed).

  python tools/isa_count.py strip1.hip 'strip1_kernelILi8ELi16ELb1ELi2ELi4ELb0ELb0ELb0ELi1ELb0E' [--blocks] [-D...]

compiles qllm_amd/csrc/<unit> (or a path) to assembly and, for every kernel whose mangled or demangled name matches the regular
expression, prints how many instructions it holds of each class -- from mnemonic prefixes alone:
  valu  v_* except MFMA          salu  s_* (smem: the s_load_* / s_buffer_load_* among them; wait: s_waitcnt / s_nop among them)
  vmem  global_ / buffer_ / flat_ / scratch_      lds  ds_*      mfma  v_mfma_* / v_smfmac_*
and the same counts for the instructions in front of the first non-temporal (`nt`) vector load: what a wave executes before its first
weight word is requested.  The counts are static: a kernel with uniform branches holds the instructions of every path; --blocks
prints them per basic block (label, counts, terminator), so that one path can be added up by hand."""
import argparse
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_asm  # noqa: E402

CLASSES = ("valu", "salu", "smem", "wait", "vmem", "lds", "mfma", "other")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")
LABEL = re.compile(r"^([.\w$]+):")
BB = re.compile(r"^; %bb\.(\d+):")


def classify(m):
    if m.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if m.startswith("v_"):
        return "valu"
    if m.startswith("s_"):
        return "salu"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if m.startswith("ds_"):
        return "lds"
    return "other"


def count(insns):
    c = dict.fromkeys(CLASSES, 0)
    for m, _ in insns:
        k = classify(m)
        c[k] += 1
        if k == "salu" and m.startswith(("s_load", "s_buffer_load")):
            c["smem"] += 1
        if k == "salu" and m.startswith(("s_waitcnt", "s_nop")):
            c["wait"] += 1
    return c


def kernels(text):
    """{mangled name: [(label, [(mnemonic, operands)])]}: the basic blocks of every .amdhsa_kernel of the assembly, in text order."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur, blocks = {}, None, None
    for line in text.splitlines():
        lab = LABEL.match(line)
        if lab:
            if lab.group(1) in names:
                cur, blocks = lab.group(1), [("entry", [])]
                out[cur] = blocks
            elif cur and lab.group(1).startswith(".Lfunc_end"):
                cur = None
            elif cur:
                blocks.append((lab.group(1), []))
            continue
        bb = BB.match(line)
        if cur and bb:                       # (a block that is only fallen into carries no label, just this comment)
            if blocks[-1][1]:
                blocks.append(("%bb." + bb.group(1), []))
            continue
        if cur is None or line.lstrip().startswith((".", ";")):
            continue
        m = INSN.match(line)
        if m:
            blocks[-1][1].append((m.group(1), m.group(2).split(";")[0]))
    return out


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not os.path.exists(filt):
        return {n: n for n in names}
    res = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, res))


def fmt(c):
    return " ".join("%s=%d" % (k, c[k]) for k in CLASSES if k != "other" or c[k])


def report(name, pretty, blocks, per_block):
    flat = [i for _, b in blocks for i in b]
    first_nt = next((n for n, (m, ops) in enumerate(flat) if classify(m) == "vmem" and "load" in m and re.search(r"\bnt\b", ops)), None)
    print(pretty)
    print("  total               ", fmt(count(flat)))
    if first_nt is None:
        print("  no nt load")
    else:
        print("  before first nt load", fmt(count(flat[:first_nt])))
    if per_block:
        for label, b in blocks:
            if b:
                print("  %-20s %s  -> %s" % (label, fmt(count(b)), b[-1][0] if b[-1][0].startswith(("s_cbranch", "s_branch", "s_endpgm")) else "falls through"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit", help="a .hip file of qllm_amd/csrc, or a path")
    ap.add_argument("pattern", help="regular expression on the kernel's mangled or demangled name")
    ap.add_argument("--blocks", action="store_true", help="counts per basic block too")
    ap.add_argument("--asm", action="store_true", help="read `unit` as an assembly file instead of compiling it")
    ap.add_argument("-D", dest="defs", action="append", default=[], help="preprocessor definitions for the compile")
    args = ap.parse_args()
    if args.asm:
        with open(args.unit) as f:
            text = f.read()
    else:
        src = args.unit if os.path.exists(args.unit) else os.path.join(kernel_asm.CSRC, args.unit)
        res = subprocess.run([kernel_asm.HIPCC, *kernel_asm.FLAGS, "-I", kernel_asm.CSRC, *["-D" + d for d in args.defs], src, "-o", "-"],
                             check=True, capture_output=True, text=True)
        text = res.stdout
    ks = kernels(text)
    pretty = demangle(sorted(ks))
    pat = re.compile(args.pattern)
    hits = [n for n in sorted(ks) if pat.search(n) or pat.search(pretty[n])]
    if not hits:
        sys.exit("no kernel matches %r (%d kernels in the unit)" % (args.pattern, len(ks)))
    for n in hits:
        report(n, pretty[n], ks[n], args.blocks)


if __name__ == "__main__":
    main()
