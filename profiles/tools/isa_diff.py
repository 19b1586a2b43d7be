"""Prove that a device refactor moved code without changing it: compare the compiler's ISA text kernel by kernel.

    python profiles/tools/isa_diff.py dump <checkout of the commit before> /tmp/isa_before   # hipcc -S of every .hip in build.SOURCES
    python profiles/tools/isa_diff.py dump . /tmp/isa_after
    python profiles/tools/isa_diff.py compare /tmp/isa_before /tmp/isa_after > profiles/isa_identity_<parent hash>.txt

`dump` compiles with exactly build.py's CFLAGS (+ JAMUN_EXTRA_CFLAGS) plus `-S --cuda-device-only`.  `compare` splits every .s at the
kernel symbols (`.amdhsa_kernel` names), keeps instructions and block labels (comments and directives dropped, `.LBB<n>_<m>` -> `.LBB_<m>`:
<n> is the function's position in its file), and matches the kernels BY MANGLED NAME ACROSS THE UNION OF FILES.  The kernel descriptor
(`.amdhsa_*`: registers, static LDS, scratch) is compared as well.  Exit status 1 unless both sides have the same kernels and every one is identical.
"""
import glob
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor


def dump(root, out):
    csrc = os.path.join(root, "jamun_amd", "csrc")
    spec = importlib.util.spec_from_file_location("_build", os.path.join(csrc, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    os.makedirs(out, exist_ok=True)
    hips = [s for s in b.SOURCES if s.endswith(".hip")]
    cmd = lambda s: [b.HIPCC] + b.CFLAGS + b.EXTRA + ["-S", "--cuda-device-only", os.path.join(csrc, s), "-o", os.path.join(out, s[:-4] + ".s")]
    with ThreadPoolExecutor(max_workers=min(len(hips), os.cpu_count() or 4)) as ex:
        list(ex.map(lambda s: subprocess.check_call(cmd(s)), hips))


def kernels(d):
    """{mangled kernel name: (file, [instructions and labels], [descriptor lines])} over every .s of directory d"""
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        lines = open(path).read().split("\n")
        names = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")}
        cur = None
        for l in lines:
            s = l.split(";")[0].strip()
            m = re.match(r"^(\w+):$", s)
            if m and m.group(1) in names:
                assert m.group(1) not in out, f"{m.group(1)} defined twice"
                cur = out[m.group(1)] = (os.path.basename(path), [], [])
            elif s.startswith(".amdhsa_kernel "):
                cur = out[s.split()[1]]
            elif s.startswith((".Lfunc_end", ".end_amdhsa_kernel")):
                cur = None
            elif cur and s.startswith(".amdhsa_"):
                cur[2].append(s)
            elif cur and s and (not s.startswith(".") or s.startswith(".LBB")):
                cur[1].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def compare(before, after):
    a, b = kernels(before), kernels(after)
    bad = 0
    print(f"{'instructions':>12}  {'verdict':<9} {'file before -> file after':<44} kernel")
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            verdict = "ONLY BEFORE" if k in a else "ONLY AFTER"
        else:
            verdict = "same" if a[k][1] == b[k][1] and a[k][2] == b[k][2] else ("DIFFERS" if a[k][1] != b[k][1] else "DESCRIPTOR")
        bad += verdict != "same"
        n = sum(1 for x in (a.get(k) or b[k])[1] if not x.startswith(".LBB"))
        fa, fb = a[k][0] if k in a else "-", b[k][0] if k in b else "-"
        print(f"{n:>12}  {verdict:<9} {fa + (' -> ' + fb if fb != fa else ''):<44} {k}")
    print(f"summary: {len(a)} kernels before, {len(b)} after, {len(set(a) | set(b)) - bad} identical, {bad} not")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
