#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 device code?  (the bar for a refactor of the kernels; needs no GPU)

    python tools/isa_diff.py OLD NEW                                            every locator_amd/csrc/*.hip
    python tools/isa_diff.py OLD NEW --old-flags=-DA --new-flags=-DB --files x.hip   some, with extra flags per tree
    python tools/isa_diff.py OLD NEW --patch tools/probes/stack_fused_probes.patch --files stack_fused.hip --flags=-DSF_STAMPS=0
                                                                                each tree's file with each tree's patch applied

Compiles with each tree's own Makefile flags plus -S --cuda-device-only and drops the lines that hold __hip_cuid_ (a hash of
the source text).  Exit status 1 if any file differs; the first differing kernel (last label above the line) is named.
"""
import argparse, concurrent.futures, glob, os, re, shlex, subprocess, sys, tempfile


def asm(tree, name, extra, patch, tmp, side):
    csrc = os.path.join(tree, "locator_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950")
    src = os.path.join(csrc, name)
    if patch:
        src = os.path.join(tmp, side + "_" + name)
        open(src, "w").write(open(os.path.join(csrc, name)).read())
        subprocess.run(["patch", "-s", "--no-backup-if-mismatch", src, os.path.join(tree, patch)], check=True)
    out = os.path.join(tmp, side + "_" + name + ".s")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *shlex.split(flags), "-I", csrc, *extra, "-S", "--cuda-device-only", src, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return [l for l in open(out) if "__hip_cuid_" not in l]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old"), ap.add_argument("new")
    ap.add_argument("--files", nargs="*"), ap.add_argument("--patch")
    ap.add_argument("--flags", default=""), ap.add_argument("--old-flags", default=""), ap.add_argument("--new-flags", default="")
    a = ap.parse_args()
    names = a.files or sorted(os.path.basename(p) for p in glob.glob(os.path.join(a.new, "locator_amd", "csrc", "*.hip")))
    fl = {"old": shlex.split(a.flags + " " + a.old_flags), "new": shlex.split(a.flags + " " + a.new_flags)}
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        jobs = {(n, s): ex.submit(asm, getattr(a, s), n, fl[s], a.patch, tmp, s) for n in names for s in ("old", "new")}
        for n in names:
            o, w = jobs[n, "old"].result(), jobs[n, "new"].result()
            i = next((i for i, (x, y) in enumerate(zip(o, w)) if x != y), None if len(o) == len(w) else min(len(o), len(w)))
            where = ""
            if i is not None:
                bad += 1
                labels = [l.split(":")[0] for l in w[:i] if re.match(r"^[A-Za-z_][\w.$]*:", l) and not l.startswith(".L")]
                where = "  first difference at line %d, in %s" % (i + 1, labels[-1] if labels else "?")
            print("%-22s %6d lines  %s%s" % (n, len(w), "DIFFERENT" if where else "identical", where))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
