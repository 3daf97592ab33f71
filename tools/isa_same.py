"""Do two source trees compile to the same gfx950 machine code?  For a refactor that is meant to leave the kernels as they are.

    python tools/isa_same.py PARENT_TREE [CHANGE_TREE] [--files a.hip b.hip ...] [--out FILE] [--keep DIR] [--alias REGEX=REPL ...]

Each named file of gecco_amd/csrc (default: the any-label lane-group files and the three contig-walk files) is compiled from both
trees with the flags gecco_amd/build.py of the CHANGE tree gives that file, plus `--cuda-device-only -S`.  The assembly is split by
kernel symbol (the .amdhsa_kernel directives name them); of a kernel's body the comments, the directives and the numbers of the
local labels are dropped, and what is left is compared as text, for equality only.  Printed: one line per kernel instance, "same" or
"differs" with the two instruction counts, then the summary, which `--out` keeps: per file the number of instances and how many are
the same, and every instance that differs by name.  Exit status 1 when an instance differs or exists in one tree only.  No device
is needed.

`--alias REGEX=REPL` is for a change that gives a kernel template a further parameter, which renames every instance: a kernel of
the CHANGE tree whose demangled name matches REGEX as a whole is compared under the name REPL gives (re.sub), the parent's name of
the instantiation that is meant to stay the same.  E.g. --alias 'gen_labelled<(\d+), (\w+), false>=gen_labelled<\1, \2>'."""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("crf_general.hip", "crf_general_windowed.hip", "crf_spans.hip", "crf_runs.hip", "crf_edges.hip", "crf_kbest.hip",
         "crf_minrun.hip", "crf_counts.hip")
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)?")


def build_module(tree):
    spec = importlib.util.spec_from_file_location("_isa_same_build", os.path.join(tree, "gecco_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(build, tree, name, out):
    cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", *build.EXTRA_FLAGS.get(name, []), "-x", "hip",
           "--cuda-device-only", "-S", os.path.join(tree, "gecco_amd", "csrc", name), "-o", out]
    subprocess.check_call(cmd)
    with open(out) as fh:
        return fh.read()


def kernels(text):
    """{kernel symbol: [instruction lines]} of one assembly file."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M))
    out, cur = {}, None
    for raw in text.splitlines():
        line = raw.split(";")[0].strip()
        if line.endswith(":") and line[:-1] in names:
            cur = out.setdefault(line[:-1], [])
            continue
        if cur is None or not line:
            continue
        if line.startswith((".Lfunc_end", ".section")):
            cur = None  # the end of the kernel's body
            continue
        if line.startswith(".") and not LOCAL_LABEL.match(line):
            continue  # a directive
        cur.append(LOCAL_LABEL.sub(".L", " ".join(line.split())))
    return out


def demangled(symbols):
    if not symbols:
        return {}
    try:
        res = subprocess.run(["c++filt", "-p", *symbols], capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(symbols, (r.replace("void ", "").replace("gecco::", "").replace("(anonymous namespace)::", "") for r in res)))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in symbols}


def aliased(change, parent, aliases):
    """`change` ({symbol: lines}) with every kernel whose demangled name an alias maps onto a parent kernel's under that symbol."""
    if not aliases:
        return change
    by_name = {name: sym for sym, name in demangled(sorted(parent)).items()}
    names, out = demangled(sorted(change)), {}
    for sym, body in change.items():
        for pattern, repl in aliases:
            if re.fullmatch(pattern, names[sym]):
                sym = by_name.get(re.sub(pattern, repl, names[sym]), sym)
                break
        out[sym] = body
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent", help="the parent commit, checked out")
    ap.add_argument("change", nargs="?", default=ROOT, help="the tree to compare with it (default: this one)")
    ap.add_argument("--files", nargs="+", default=list(FILES))
    ap.add_argument("--out", default=None, help="also write the summary to this file")
    ap.add_argument("--keep", default=None, help="keep the assembly files in this directory")
    ap.add_argument("--alias", nargs="+", default=[], metavar="REGEX=REPL",
                    help="compare a kernel of the change whose demangled name matches REGEX under the name REPL gives")
    args = ap.parse_args()
    build = build_module(args.change)
    keep = args.keep or tempfile.mkdtemp(prefix="isa_same_")
    os.makedirs(keep, exist_ok=True)
    jobs = [(side, tree, name) for name in args.files for side, tree in (("parent", args.parent), ("change", args.change))]
    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1, 16)) as pool:
        texts = list(pool.map(lambda j: assembly(build, j[1], j[2], os.path.join(keep, f"{j[0]}_{j[2]}.s")), jobs))
    asm = {(side, name): kernels(text) for (side, _, name), text in zip(jobs, texts)}
    flags = " ".join(["hipcc", f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "[the file's flags of build.py]", "--cuda-device-only", "-S"])
    lines = [f"# {flags}: every kernel instance of the parent tree against the change's; comments, directives and",
             "# the numbers of local labels dropped, the rest compared as text.",
             "file | flags of build.py | instances | same | differ"]
    exceptions, instances = [], []
    for name in args.files:
        p = asm[("parent", name)]
        c = aliased(asm[("change", name)], p, [tuple(a.split("=", 1)) for a in args.alias])
        names = demangled(sorted(set(p) | set(c)))
        same = 0
        for sym in sorted(set(p) | set(c)):
            count = lambda k: str(len(k[sym])) if sym in k else "absent"  # noqa: E731
            equal = sym in p and sym in c and p[sym] == c[sym]
            instances.append(f"{name}  {names[sym]} | {'same' if equal else 'differs'} | instructions parent {count(p)} change {count(c)}")
            if equal:
                same += 1
            else:
                exceptions.append(instances[-1])
        total = len(set(p) | set(c))
        lines.append(f"{name} | {' '.join(build.EXTRA_FLAGS.get(name, [])) or '-'} | {total} | {same} | {total - same}")
    lines.append(f"exceptions: {len(exceptions)}" + ("" if exceptions else " (identical code: no resource table and no timing to record)"))
    lines += exceptions
    print("\n".join(instances + lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(1 if exceptions else 0)


if __name__ == "__main__":
    main()
