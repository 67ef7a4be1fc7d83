"""Are the kernels of two builds the same machine code? Compares hipcc -S listings function by function:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only heat_amd/csrc/kernels.hip -o NEW.s   (each source so)
    python tools/listing_diff.py OLD.s NEW.s [NEW2.s ...]
Per mangled name, the text between the function's label and its .Lfunc_end — instructions and, for a kernel, every
.amdhsa_* descriptor line — must be equal once what depends on a function's place in its file is normalised: the function
index in block labels (BB<n>_, .Lfunc_end<n>), the numbers of .Ltmp<n> labels (renumbered by first use), the __hip_cuid_*
symbol and the padding in front of comments. The NEW listings are united: a function may have moved file. Prints the
functions missing, added or different with the first differing lines; exit status 1 on any difference.
(Compare listings, not code objects: linked kernels differ in pc-relative constants and the descriptor's entry offset.)"""
import re, sys


def functions(path):
    """{mangled name: (normalised lines, is a kernel)} of one listing"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if name is None and m:
            name, body = m.group(1), []
        elif name is not None and re.match(r"\.Lfunc_end\d+:", line):
            tmp = {}
            text = re.sub(r"\.Ltmp\d+", lambda t: tmp.setdefault(t.group(0), ".Ltmp#%d" % len(tmp)), "\n".join(body))
            out[name] = (text.split("\n"), any(l.startswith(".amdhsa_kernel ") for l in body))
            name = None
        elif name is not None:
            line = re.sub(r"BB\d+_", "BB#_", re.sub(r"__hip_cuid_\w+", "__hip_cuid_#", line))
            body.append(" ".join(line.split()))
    return out


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    old, new = functions(argv[1]), {}
    for path in argv[2:]:
        new.update(functions(path))
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%s: %s" % ("ADDED  " if name in new else "MISSING", name))
        elif old[name][0] != new[name][0]:
            a, b = old[name][0], new[name][0]
            i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("DIFFERS: %s\n  line %d of %d / %d\n  - %s\n  + %s" % (name, i + 1, len(a), len(b), "\n  - ".join(a[i:i + 3]),
                                                                       "\n  + ".join(b[i:i + 3])))
        else:
            continue
        bad += 1
    same = [n for n in old if n in new and old[n][0] == new[n][0]]
    print("%d functions identical (%d of them kernels), %d missing, added or different" % (
        len(same), sum(old[n][1] for n in same), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
