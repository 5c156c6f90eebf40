"""Side-by-side register / scratch / occupancy table of two builds of the same sources, from the compiler's own remarks:

    hipcc <flags of csrc/Makefile> -Rpass-analysis=kernel-resource-usage -c X.hip -o X.o 2> X_parent.txt     (the parent's source)
    hipcc ...                                                            -c X.hip -o X.o 2> X_new.txt        (this tree's)
    python tools/kernel_resources.py X_parent.txt X_new.txt [more pairs...] [--only substring,substring]

One line per kernel: VGPRs, AGPRs, scratch bytes per lane, occupancy in waves per SIMD, parent -> new; a trailing `!` marks a kernel whose
scratch grew from 0 or whose occupancy dropped."""
import re
import subprocess
import sys


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None and val.isdigit():
            cur[key] = int(val)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines())) if r.returncode == 0 else {n: n for n in names}


def main(argv):
    only = None
    if "--only" in argv:
        i = argv.index("--only")
        only = argv[i + 1].split(",")
        argv = argv[:i] + argv[i + 2:]
    print(f"{'kernel':<78s} {'VGPRs':>10s} {'AGPRs':>8s} {'scratch B/lane':>15s} {'occupancy':>10s}")
    bad = 0
    for a, b in zip(argv[0::2], argv[1::2]):
        pa, pb = parse(a), parse(b)
        names = demangle(list(pa))
        for k, ra in pa.items():
            rb = pb.get(k)
            short = re.sub(r"^void ", "", names[k]).split("(")[0]
            if rb is None or (only and not any(s in short for s in only)):
                continue
            col = lambda key: f"{ra.get(key, '-')} -> {rb.get(key, '-')}"
            worse = (ra.get("ScratchSize [bytes/lane]", 0) == 0 and rb.get("ScratchSize [bytes/lane]", 0) > 0) or \
                rb.get("Occupancy [waves/SIMD]", 0) < ra.get("Occupancy [waves/SIMD]", 0)
            bad += worse
            print(f"{short[:78]:<78s} {col('VGPRs'):>10s} {col('AGPRs'):>8s} {col('ScratchSize [bytes/lane]'):>15s} {col('Occupancy [waves/SIMD]'):>10s}"
                  + (" !" if worse else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
