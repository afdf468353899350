"""Compare the gfx950 machine code of two source trees, kernel by kernel.

    python tools/codeobj_diff.py OLD_TREE NEW_TREE [-j JOBS] [--per-file] [--only GLOB]

For every csrc/*.hip of either tree the device side alone is compiled with that tree's own
build.py FLAGS (plus --cuda-device-only --no-gpu-bundle-output -c).  By default every kernel of
a tree goes into one pool, so a kernel may move between source files: a symbol found in two
files of one tree is an error, and the two pools are compared by symbol for equality of
  (a) the set of kernel symbols,
  (b) each kernel's disassembled instruction stream (encodings and operands, not addresses),
  (c) each kernel's register counts, LDS / scratch sizes and workgroup-size limit.
One line per source file of the new tree with its kernel count, then the totals.  --per-file
compares file against file of the same name instead (a moved kernel then shows as only-old /
only-new); --only restricts both trees to the source files matching GLOB.
Exit status 1 on any difference.  Needs the compiler, no GPU.
"""
import argparse
import fnmatch
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

SUB = "mvml-mpi_amd"
FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".max_flat_workgroup_size")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_tree_build", os.path.join(tree, SUB, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hip_sources(tree, only="*"):
    csrc = os.path.join(tree, SUB, "csrc")
    return sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and fnmatch.fnmatch(f, only))


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s failed:\n%s\n%s" % (" ".join(cmd), r.stdout, r.stderr))
    return r.stdout


def kernel_meta(notes):
    """{kernel name: {field: value}} from `llvm-readelf --notes` (the amdhsa.kernels list)."""
    out = {}
    for entry in re.split(r"^  - ", notes, flags=re.M)[1:]:
        top = dict(re.findall(r"^    (\.\w+): +(\S+)$", entry, flags=re.M))
        top.update(re.findall(r"^(\.\w+): +(\S+)$", entry.split("\n", 1)[0], flags=re.M))
        if ".name" in top:
            out[top[".name"]] = {f: top.get(f) for f in FIELDS}
    return out


def kernel_code(disasm):
    """{symbol: [instruction lines without their addresses]} from `llvm-objdump -d`."""
    out, cur = {}, None
    for line in disasm.splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and "//" in line:  # an instruction with its encoding (not elided padding)
            cur.append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line).strip())
    return out


def code_object(tree, src, outdir):
    b = load_build(tree)
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(b.HIPCC))), "llvm", "bin")
    obj = os.path.join(outdir, src + ".co")
    run([b.HIPCC, *b.FLAGS, "--cuda-device-only", "--no-gpu-bundle-output", "-c",
         os.path.join(tree, SUB, "csrc", src), "-o", obj])
    meta = kernel_meta(run([os.path.join(llvm, "llvm-readelf"), "--notes", obj]))
    code = kernel_code(run([os.path.join(llvm, "llvm-objdump"), "-d", obj]))
    return {k: (meta[k], code.get(k)) for k in meta}


def compare(old, new):
    """(differing, only-old, only-new) kernel symbols of two {symbol: (meta, code)} maps."""
    both = sorted(set(old) & set(new))
    return ([k for k in both if old[k] != new[k] or old[k][1] is None],
            sorted(set(old) - set(new)), sorted(set(new) - set(old)))


def report(differ, gone, added):
    for tag, ks in (("differs", differ), ("only in old", gone), ("only in new", added)):
        for k in ks:
            print("    %s: %s" % (tag, k))
    return len(differ) + len(gone) + len(added)


def per_file(jobs, names):
    bad = 0
    for src in names:
        if (0, src) not in jobs or (1, src) not in jobs:
            print("%-18s only in the %s tree" % (src, "old" if (0, src) in jobs else "new"))
            bad += 1
            continue
        old, new = jobs[0, src].result(), jobs[1, src].result()
        differ, gone, added = compare(old, new)
        print("%-18s kernels old %d new %d, compared %d, differing %d, only-old %d, only-new %d"
              % (src, len(old), len(new), len(set(old) & set(new)), len(differ), len(gone), len(added)))
        bad += report(differ, gone, added)
    return bad


def pooled(jobs, names):
    bad, pools = 0, ({}, {})
    home = ({}, {})  # symbol -> the source file that defines it
    for (i, src), job in sorted(jobs.items()):
        for k, v in job.result().items():
            if k in home[i]:
                print("%s tree: %s is defined in both %s and %s" % (("old", "new")[i], k, home[i][k], src))
                bad += 1
            home[i][k] = src
            pools[i][k] = v
    for src in names:
        if (1, src) in jobs:
            print("%-18s %d kernels" % (src, len(jobs[1, src].result())))
    differ, gone, added = compare(*pools)
    print("pooled: kernels old %d new %d, compared %d, differing %d, only-old %d, only-new %d"
          % (len(pools[0]), len(pools[1]), len(set(pools[0]) & set(pools[1])), len(differ), len(gone),
             len(added)))
    return bad + report(differ, gone, added)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-j", type=int, default=4)
    ap.add_argument("--per-file", action="store_true", help="compare file against file, not pooled")
    ap.add_argument("--only", default="*", help="source files to compile (a glob, default all)")
    a = ap.parse_args()
    trees = [os.path.abspath(a.old), os.path.abspath(a.new)]
    names = sorted(set(hip_sources(trees[0], a.only)) | set(hip_sources(trees[1], a.only)))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=a.j) as ex:
        jobs = {}
        for i, tree in enumerate(trees):
            os.makedirs(os.path.join(tmp, str(i)))
            for src in hip_sources(tree, a.only):
                jobs[i, src] = ex.submit(code_object, tree, src, os.path.join(tmp, str(i)))
        bad = (per_file if a.per_file else pooled)(jobs, names)
    print("TOTAL differing, unmatched or doubly defined kernels: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
