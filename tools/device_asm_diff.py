#!/usr/bin/env python3
"""Do the kernels of the working tree compile to the same gfx950 instructions as those of a revision?

    python tools/device_asm_diff.py REV [files...]

Each csrc/*.hip (default: all; a file is named by its basename or any path to it) is compiled to device
assembly with build.py's flags, once from `git show REV:...` and once from the working tree, each next
to its own csrc/*.h.  Lines carrying the `__hip_cuid_<hash>` symbol (a hash of the source text) are
dropped; the listing has no line information, so a clean-up that changes no instruction compares equal.
Prints one `identical` / `DIFFERENT` line per file; exits 1 on any difference.  Needs no GPU.
"""
import concurrent.futures as cf
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ai_agent_kubectl_amd.build import ARCH, CSRC, HIPCC, file_flags  # noqa: E402

REL = os.path.relpath(CSRC, ROOT)


def listing(src):
    out = src + ".s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", f"--offload-arch={ARCH}", "-munsafe-fp-atomics", *file_flags(src),
                        "--cuda-device-only", "-S", src, "-o", out], stderr=subprocess.PIPE, text=True)
    if r.returncode:
        raise RuntimeError(f"{src} does not compile:\n{r.stderr}")
    with open(out) as f:
        return [l for l in f if "__hip_cuid_" not in l]


def main(argv):
    if not argv:
        sys.exit(__doc__)
    rev = argv[0]
    names = sorted(os.path.basename(p) for p in (argv[1:] or glob.glob(os.path.join(CSRC, "*.hip"))))
    with tempfile.TemporaryDirectory() as tmp:
        old, new = os.path.join(tmp, "old"), os.path.join(tmp, "new")
        os.mkdir(old), os.mkdir(new)
        headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))
        for name in names + headers:
            r = subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{REL}/{name}"], stdout=subprocess.PIPE,
                               stderr=subprocess.DEVNULL)
            if r.returncode == 0:
                with open(os.path.join(old, name), "wb") as f:
                    f.write(r.stdout)
            elif not name.endswith(".h"):   # a header may be newer than REV; a kernel file must exist there
                raise RuntimeError(f"{name} does not exist at {rev}")
            with open(os.path.join(CSRC, name), "rb") as g, open(os.path.join(new, name), "wb") as f:
                f.write(g.read())
        with cf.ThreadPoolExecutor(16) as ex:   # at most 16 compiles at a time
            res = list(ex.map(listing, [os.path.join(d, n) for d in (old, new) for n in names]))
    differ = 0
    for name, x, y in zip(names, res[:len(names)], res[len(names):]):
        if x == y:
            print(f"{name}: identical")
            continue
        differ += 1
        first = next((i for i, (p, q) in enumerate(zip(x, y), 1) if p != q), min(len(x), len(y)) + 1)
        print(f"{name}: DIFFERENT (first differing line {first})")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
