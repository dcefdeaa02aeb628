#!/usr/bin/env python3
"""Which gfx950 kernels does libwsmgmap.so hold, and which of them did a traced run launch?

    tools/kernel_inventory.py                       # demangled names of every kernel of the built library, one per line
    tools/kernel_inventory.py --objects DIR         # the same from the per-file objects (csrc/build/*.o)
    tools/kernel_inventory.py --trace [LABEL=]T.csv [...]   # coverage table: name <TAB> launches <TAB> first LABEL that launched it

Builds nothing.  Recipe: the `.hip_fatbin` section of the library is a row of clang offload bundles (one per .hip file); each is cut
out at its `__CLANG_OFFLOAD_BUNDLE__` magic, `clang-offload-bundler --unbundle` extracts the hipv4 gfx950 code object, and
`llvm-objdump --syms [--demangle]` lists its `*.kd` kernel descriptors, mangled and demangled.  (`roc-obj-ls` is not needed.)

The trace is rocprofv3's `*_kernel_trace.csv` (`--kernel-trace`, with or without `--mangled-kernels`; several files = several
processes; a path may be a glob pattern); kernels of other libraries (torch, rocBLAS) in it are ignored.  The suite is traced one
test file per rocprofv3 run, each run's traces given as `tests/test_x.py=DIR/*/*kernel_trace.csv`: the third column is the first
label, in argument order, whose traces hold a launch of the kernel (blank without labels).
"""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "ws-mgmap_amd", "wsmgmap", "lib", "libwsmgmap.so")
LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
ARCH = "gfx950"


def _tool(name):
    p = os.path.join(LLVM_BIN, name)
    return p if os.path.exists(p) else name


def _bundle_targets(path):
    out = subprocess.run([_tool("clang-offload-bundler"), "--list", "--type=o", "--input=" + path],
                         check=True, capture_output=True, text=True).stdout
    return [t for t in out.split() if t.startswith("hip") and t.endswith(ARCH)]


def _kd_symbols(code_object):
    """{mangled: demangled} of the kernel descriptors (`*.kd` objects) of one code object.  llvm-objdump prints the symbol table twice,
    plain and with LLVM's demangler (which knows __bf16; the system c++filt does not); the two listings have the same order."""
    def names(*extra):
        out = subprocess.run([_tool("llvm-objdump"), "--syms", *extra, code_object], check=True, capture_output=True, text=True).stdout
        res = []
        for line in out.splitlines():
            if "\t" not in line or " O " not in line.split("\t", 1)[0]:
                continue
            res.append(line.split("\t", 1)[1].split(" ", 1)[1])          # after "<section>\t<size> "
        return res
    plain, pretty = names(), names("--demangle")
    assert len(plain) == len(pretty)
    out = {}
    for m, d in zip(plain, pretty):
        if m.endswith(".kd"):
            out[m[:-3]] = d[:-len(" (.kd)")] if d.endswith(" (.kd)") else (d[:-3] if d.endswith(".kd") else d)
    return out


def _bundles_of(path):
    """Byte strings of the offload bundles inside an ELF file (a shared library holds one per linked object)."""
    data = open(path, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    return [data[a:b] for a, b in zip(starts, starts[1:] + [len(data)])]


def inventory(lib=None, objects=None):
    """[(mangled, demangled)] of the gfx950 kernels of the library (or of the per-file objects), sorted by demangled name.  A name
    defined in two code objects is an error (a trace could not tell the two apart)."""
    if objects:
        paths = sorted(glob.glob(os.path.join(objects, "*.o")))
    else:
        paths = [lib or DEFAULT_LIB]
    for p in paths:
        if not os.path.exists(p):
            raise SystemExit("not built: " + p)
    found, dup = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        n = 0
        for path in paths:
            for blob in _bundles_of(path):
                n += 1
                b = os.path.join(tmp, "b%d.bundle" % n)
                with open(b, "wb") as f:
                    f.write(blob)
                for t in _bundle_targets(b):
                    co = os.path.join(tmp, "b%d.co" % n)
                    subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + t, "--input=" + b,
                                    "--output=" + co], check=True, capture_output=True)
                    for m, d in _kd_symbols(co).items():
                        if m in found:
                            dup.append(m)
                        found[m] = d
    if dup:
        raise SystemExit("kernel defined in more than one code object: " + ", ".join(sorted(dup)))
    return sorted(found.items(), key=lambda x: x[1])


def _squash(s):
    return re.sub(r"\s+", "", s)


def _col(header, *names):
    for n in names:
        if n in header:
            return header.index(n)
    raise SystemExit("trace has no column %s: %s" % ("/".join(names), header))


def _labelled(args):
    """[(label, path)] of the --trace arguments `[LABEL=]PATTERN`, patterns expanded, argument order kept."""
    out = []
    for arg in args:
        label, pat = ("", arg) if (os.path.exists(arg) or "=" not in arg) else arg.split("=", 1)
        files = sorted(glob.glob(pat))
        if not files:
            raise SystemExit("no trace file matches " + pat)
        out += [(label, f) for f in files]
    return out


def coverage(inv, traces):
    """[(demangled, launches, first label or '')] for every kernel of the inventory, in inventory order."""
    by_m = {m: d for m, d in inv}
    by_d = {_squash(d): d for _, d in inv}
    count = {d: 0 for _, d in inv}
    first = {}
    for label, fn in _labelled(traces):
        with open(fn, newline="") as f:
            r = csv.reader(f)
            h = next(r, None)
            if not h:
                continue
            kn = _col(h, "Kernel_Name")
            for row in r:
                name = row[kn]
                if name.endswith(".kd"):
                    name = name[:-3]
                d = by_m.get(name) or by_d.get(_squash(name))
                if d is None:
                    continue
                count[d] += 1
                first.setdefault(d, label)
    return [(d, count[d], first.get(d, "")) for _, d in inv]


def read_coverage(path):
    """[(name, launches, test)] of a committed coverage file ('#' lines are comments)."""
    rows = []
    with open(path) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            c = line.rstrip("\n").split("\t")
            rows.append((c[0], int(c[1]), c[2] if len(c) > 2 else ""))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=None, help="shared library (default: the built libwsmgmap.so)")
    ap.add_argument("--objects", default=None, help="directory of per-file objects instead of the library")
    ap.add_argument("--mangled", action="store_true", help="print mangled <TAB> demangled")
    ap.add_argument("--trace", nargs="+", default=None, help="[LABEL=]rocprofv3 *_kernel_trace.csv file(s) or pattern(s)")
    a = ap.parse_args()
    inv = inventory(a.lib, a.objects)
    if a.trace is None:
        for m, d in inv:
            print("%s\t%s" % (m, d) if a.mangled else d)
        return 0
    rows = coverage(inv, a.trace)
    never = sum(1 for r in rows if r[1] == 0)
    print("# kernel <TAB> launches <TAB> first test file that launched it; %d kernels, %d never launched" % (len(rows), never))
    for d, n, t in rows:
        print("%s\t%d\t%s" % (d, n, t))
    return 0


if __name__ == "__main__":
    sys.exit(main())
