"""Device assembly of every csrc/*.hip, to show that a host-only change left the kernels alone.

  python tools/device_asm.py dump OUTDIR [--csrc DIR]   compile each source device-only (-S) with the build's own flags
  python tools/device_asm.py compare DIR_A DIR_B         compare two dumps file by file; exit status 1 on a difference

Dump once in a checkout of the parent commit and once in the branch (`--csrc` points this script at another checkout's
pykaldi2_amd/csrc).  Lines that contain `__hip_cuid_` are dropped before comparing: that symbol is a hash of the
translation unit's text and is the one thing an edit of host code changes in the device assembly.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import build as B  # noqa: E402


def dump(out, csrc):
    os.makedirs(out, exist_ok=True)
    flags = [f for f in B.FLAGS if not f.startswith("-I")] + ["-I" + os.path.join(os.path.dirname(os.path.dirname(csrc)), "include"), "-I" + csrc]

    def cc(s):
        cmd = [B._hipcc()] + flags + B.FILE_FLAGS.get(s, []) + ["--cuda-device-only", "-S", os.path.join(csrc, s), "-o", os.path.join(out, s[:-4] + ".s")]
        return s, subprocess.run(cmd, capture_output=True, text=True)

    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=8) as ex:
        for s, r in ex.map(cc, srcs):
            if r.returncode:
                sys.exit("hipcc failed on %s\n%s" % (s, r.stderr))
    print("%d files -> %s" % (len(srcs), out))


def lines(path):
    with open(path) as f:
        return [l for l in f if "__hip_cuid_" not in l]


def compare(a, b):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print("%-32s only in one dump" % n); bad += 1
            continue
        la, lb = lines(pa), lines(pb)
        same = la == lb
        print("%-32s %7d lines  %s" % (n, len(la), "identical" if same else "DIFFERENT"))
        bad += not same
    print("%d of %d files identical" % (len(names) - bad, len(names)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        csrc = os.path.abspath(sys.argv[sys.argv.index("--csrc") + 1]) if "--csrc" in sys.argv else B.CSRC
        dump(sys.argv[2], csrc)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
