#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 kernels?   tools/isa_same.py <parent tree> <branch tree>

Every csrc/*.hip of both trees is compiled to device assembly with the flags of that tree's build.py (per-file flags
included), the assembly is cut into kernels (the function's text and its .amdhsa_kernel descriptor), each kernel is
normalised -- comments stripped, its own mangled symbol replaced by a placeholder, the function index dropped from the
function-numbered local labels -- and the trees are compared file by file as multisets of kernels.  Everything else,
symbolic references included, has to match to the letter.  Text comparison only: nothing is loaded and no GPU is used.
Exit status 1 if any kernel exists only in the branch (a surviving kernel changed, or a new one appeared).
"""
import collections
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

BEGIN = re.compile(r";\s*-- Begin function (\S+)")
LOCAL = re.compile(r"\.L(BB|func_end|JTI)\d+")


def load_build(tree):
    """the tree's build.py as a module (it sits next to csrc/ in the package directory)"""
    (path,) = [p for p in glob.glob(os.path.join(tree, "*", "build.py")) if os.path.isdir(os.path.join(os.path.dirname(p), "csrc"))]
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernels(asm):
    """[(symbol, normalised text)] of every function of the assembly that carries a kernel descriptor"""
    out, sym, body = [], None, []
    for line in asm.splitlines():
        m = BEGIN.search(line)
        if m:
            sym, body = m.group(1), []
        if sym is None:
            continue
        code = line.split(";", 1)[0].rstrip()
        if code:
            body.append(LOCAL.sub(r".L\1", code.replace(sym, "<kernel>")))
        if "-- End function" in line:
            if any(b.lstrip().startswith(".amdhsa_kernel") for b in body):
                out.append((sym, "\n".join(body)))
            sym = None
    return out


def compile_tree(tree, tmp):
    b = load_build(tree)

    def cc(src):
        name = os.path.basename(src)
        out = os.path.join(tmp, name + ".s")
        cmd = ["hipcc"] + b.FLAGS + b.PER_FILE_FLAGS.get(name, []) + ["-S", "--cuda-device-only", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
        with open(out) as f:
            return name, kernels(f.read())

    with ThreadPoolExecutor(max_workers=6) as ex:
        return dict(ex.map(cc, sorted(glob.glob(os.path.join(b.CSRC, "*.hip")))))


def demangle(syms):
    """(binutils' c++filt does not know the bf16 mangling DF16b: it borrows the half type's, which this project never uses)"""
    llvm, gnu = shutil.which("llvm-cxxfilt"), shutil.which("c++filt")
    if not syms or not (llvm or gnu):
        return syms
    args = syms if llvm else [s.replace("DF16b", "Dh") for s in syms]
    out = subprocess.run([llvm or gnu] + args, capture_output=True, text=True, check=True).stdout.split("\n")[:len(syms)]
    return out if llvm else [re.sub(r"\bhalf\b", "__bf16", n) for n in out]


def only(a, b):
    """symbols of the kernels of a that have no partner left in b (multiset difference on the normalised text)"""
    left = collections.Counter(text for _, text in b)
    syms = []
    for sym, text in a:
        if left[text] > 0:
            left[text] -= 1
        else:
            syms.append(sym)
    return demangle(syms)


def main(parent, branch):
    with tempfile.TemporaryDirectory() as tp, tempfile.TemporaryDirectory() as tb:
        kp, kb = compile_tree(parent, tp), compile_tree(branch, tb)
    n_parent = n_branch = 0
    for name in sorted(set(kp) | set(kb)):
        a, b = kp.get(name, []), kb.get(name, [])
        gone, new = only(a, b), only(b, a)
        print("%-24s parent %3d  branch %3d  identical %3d  parent only %2d  branch only %2d"
              % (name, len(a), len(b), len(a) - len(gone), len(gone), len(new)))
        for tag, names in (("parent only", gone), ("branch only", new)):
            for n in names:
                print("    %s: %s" % (tag, n))
        n_parent, n_branch = n_parent + len(gone), n_branch + len(new)
    print("total: %d kernels only in the parent, %d only in the branch" % (n_parent, n_branch))
    return 1 if n_branch else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
