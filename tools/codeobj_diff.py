#!/usr/bin/env python3
"""Are the kernels of a .hip file the same before and after a change? No GPU needed.

    tools/codeobj_diff.py [--parent REV] [--jobs N] [--json OUT] decoder.hip xattn.hip ...

For each file (a name under janus_amd/csrc) the parent revision (default HEAD) and the
working tree are compiled device-only for gfx950, each with the flags its own Makefile
gives that file. The gfx950 code object is taken out of the offload bundle and compared
per kernel name: present on both sides, the resource figures of the code object's notes
(VGPRs, AGPRs, SGPRs, LDS, scratch, spill counts, ...), and whether the disassembly of the
symbol is the same text (comments, which carry addresses, removed). The order of the
kernels in the file and everything on the host side are free to change.

Exit status 0: every kernel present on both sides is identical and none appeared; kernels
that exist on one side only are listed for the reader to judge (an instantiation the
parent built and never launched may go). 1: a difference. 2: a tool failed.
"""
import argparse
import concurrent.futures
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("janus_amd", "csrc")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
           "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
           "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack")


def run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, **kw)
    if p.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), p.stderr[-4000:]))
    return p.stdout


def llvm_bin(compile_cmd):
    """The directory of the LLVM tools that belong to the Makefile's hipcc."""
    hipcc = os.path.realpath(compile_cmd[0])
    for d in (os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin"),
              os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin"),
              os.path.dirname(hipcc)):
        if os.path.exists(os.path.join(d, "llvm-readelf")):
            return d
    raise RuntimeError("no llvm-readelf beside " + hipcc)


def compile_command(csrc, name, objdir):
    """The Makefile's own command line for this object (make -n), as a list."""
    obj = os.path.join(objdir, os.path.splitext(name)[0] + ".o")
    out = run(["make", "-n", "-B", "-C", csrc, "OBJDIR=" + objdir, obj])
    lines = [l for l in out.splitlines() if " -c " in l and name in l]
    if len(lines) != 1:
        raise RuntimeError("no single compile line for %s in make -n:\n%s" % (name, out))
    return shlex.split(lines[0]), obj


def device_object(csrc, name, workdir):
    """Compile name device-only in csrc; returns (path of the gfx950 ELF, llvm tool directory)."""
    os.makedirs(workdir, exist_ok=True)
    cmd, obj = compile_command(csrc, name, workdir)
    run(cmd + ["--cuda-device-only"], cwd=csrc)
    tools = llvm_bin(cmd)
    with open(obj, "rb") as f:
        head = f.read(len(BUNDLE_MAGIC))
    if head != BUNDLE_MAGIC:
        return obj, tools    # a bare code object
    listed = run([os.path.join(tools, "clang-offload-bundler"), "--list", "--type=o", "--input=" + obj])
    if TARGET not in listed.split():
        raise RuntimeError("%s: no %s entry in the bundle (%s)" % (name, TARGET, listed.split()))
    elf = obj + ".gfx950.co"
    run([os.path.join(tools, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
         "--input=" + obj, "--output=" + elf])
    return elf, tools


def kernel_figures(elf, tools):
    """{kernel symbol: {figure: value}} from the code object's metadata note."""
    text = run([os.path.join(tools, "llvm-readelf"), "--notes", elf])
    kernels, cur, indent, inside = {}, None, None, False
    for line in text.splitlines():
        if re.match(r"\s*amdhsa\.kernels:", line):
            inside = True
            continue
        if not inside:
            continue
        m = re.match(r"(\s*)- (\.\w+):\s*(.*)$", line)
        if m and (indent is None or len(m.group(1)) == indent):
            indent = len(m.group(1))
            cur = {m.group(2)[1:]: m.group(3).strip()}
            kernels[id(cur)] = cur
            continue
        if indent is not None and re.match(r"\s{0,%d}\S" % indent, line) and not line.startswith(" " * (indent + 1)):
            inside = False   # the list ended (amdhsa.target / amdhsa.version follow)
            continue
        m = re.match(r"(\s*)(\.\w+):\s*(.*)$", line)
        if m and cur is not None and len(m.group(1)) == indent + 2:
            cur[m.group(2)[1:]] = m.group(3).strip()
    out = {}
    for k in kernels.values():
        name = k.get("name", "").strip("'\"")
        if name:
            out[name] = {f: k[f] for f in FIGURES if f in k}
    return out


def kernel_text(elf, tools, names):
    """{kernel symbol: its disassembly, comments removed}."""
    text = run([os.path.join(tools, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", elf])
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"[0-9a-fA-F]+ <(.+)>:\s*$", line)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            if cur is not None:
                out[cur] = []
            continue
        if cur is not None:
            out[cur].append(line.split("//")[0].rstrip())
    return {k: "\n".join(l for l in v if l) for k, v in out.items()}


def readable_names(elf, tools, names):
    """{kernel symbol: demangled name}: llvm-objdump (needed anyway) prints the symbol table
    with and without --demangle in the same order, so no separate demangler has to exist."""
    objdump = os.path.join(tools, "llvm-objdump")
    plain = run([objdump, "-t", elf]).splitlines()
    pretty = run([objdump, "-t", "--demangle", elf]).splitlines()
    out = {}
    if len(plain) == len(pretty):
        for a, b in zip(plain, pretty):
            sym = a.split()[-1] if a.split() else ""
            if sym in names and a[:a.rfind(sym)] == b[:a.rfind(sym)]:
                out[sym] = b[a.rfind(sym):].strip()
    missing = [n for n in names if n not in out]
    if missing:
        print("codeobj_diff: %d kernel names of %s stay mangled (llvm-objdump --demangle gave no match)"
              % (len(missing), os.path.basename(elf)), file=sys.stderr)
    return {n: out.get(n, n) for n in names}


def describe(csrc, name, workdir):
    elf, tools = device_object(csrc, name, workdir)
    figs = kernel_figures(elf, tools)
    if not figs:
        raise RuntimeError("%s: no kernels in the code object's notes" % name)
    return figs, kernel_text(elf, tools, set(figs)), readable_names(elf, tools, set(figs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="+", help=".hip files under janus_amd/csrc")
    ap.add_argument("--parent", default="HEAD", help="revision to compare the working tree with")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 2))
    ap.add_argument("--json", help="write the per-kernel record here")
    ap.add_argument("--keep", help="keep the build products in this directory")
    a = ap.parse_args()
    names = [os.path.basename(f) for f in a.files]
    tmp = a.keep or tempfile.mkdtemp(prefix="codeobj_diff_")
    os.makedirs(tmp, exist_ok=True)
    ptree = os.path.join(tmp, "parent_tree")
    os.makedirs(ptree, exist_ok=True)
    try:
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", a.parent, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", ptree], stdin=ar.stdout, check=True)
        if ar.wait() != 0:
            raise RuntimeError("git archive %s failed" % a.parent)
        sides = {"parent": os.path.join(ptree, CSRC), "branch": os.path.join(ROOT, CSRC)}
        with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, a.jobs)) as ex:
            jobs = {(n, side): ex.submit(describe, csrc, n, os.path.join(tmp, "obj_" + side))
                    for n in names for side, csrc in sides.items()}
            res = {k: f.result() for k, f in jobs.items()}
    except (RuntimeError, subprocess.CalledProcessError, OSError) as e:
        print("codeobj_diff: %s" % e, file=sys.stderr)
        return 2
    record, bad = {}, False
    for n in names:
        (pf, pt, pn), (bf, bt, bn) = res[(n, "parent")], res[(n, "branch")]
        both = sorted(set(pf) & set(bf))
        gone, new = sorted(set(pf) - set(bf)), sorted(set(bf) - set(pf))
        fig_diff = [k for k in both if pf[k] != bf[k]]
        txt_diff = [k for k in both if pt.get(k) != bt.get(k)]
        pretty = dict(pn, **bn)
        print("%-18s parent %3d kernels, branch %3d: %3d on both sides, %d figures differ, %d disassembly differs, "
              "%d only in parent, %d only in branch" % (n, len(pf), len(bf), len(both), len(fig_diff), len(txt_diff),
                                                       len(gone), len(new)))
        for k in fig_diff:
            print("  figures differ: %s\n    parent %s\n    branch %s" % (pretty[k], pf[k], bf[k]))
        for k in txt_diff:
            print("  disassembly differs: %s" % pretty[k])
        for k in gone:
            print("  only in parent: %s" % pretty[k])
        for k in new:
            print("  only in branch: %s" % pretty[k])
        bad = bad or bool(fig_diff or txt_diff or new)
        record[n] = {"parent_kernels": len(pf), "branch_kernels": len(bf), "identical": len(both) - len(set(fig_diff + txt_diff)),
                     "figures_differ": [pretty[k] for k in fig_diff], "disassembly_differs": [pretty[k] for k in txt_diff],
                     "only_in_parent": [pretty[k] for k in gone], "only_in_branch": [pretty[k] for k in new],
                     "figures": {k: bf[k] for k in both}}
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"parent": a.parent, "files": record}, f, indent=1, sort_keys=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
