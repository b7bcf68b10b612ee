"""Per-kernel resource table from the text hipcc -Rpass-analysis=kernel-resource-usage prints (as ssme_amd/build.py runs it), and the
comparison of two such reports: the form of profiles/user_cov_stock_kernels.txt and profiles/series_history_stock_kernels.txt.

    python tools/kernel_resources.py PARENT_REPORT CHANGE_REPORT > profiles/NAME.txt

Kernel names are demangled with c++filt when it is on the path."""
import re
import shutil
import subprocess
import sys

KEYS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("LDS Size [bytes/block]", "lds"), ("ScratchSize [bytes/lane]", "scratch"),
        ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"), ("Occupancy [waves/SIMD]", "occ"))


def parse(path):
    stats, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            stats.setdefault(name, {})
            continue
        for key, short in KEYS:
            m = re.search(r"remark: .*\s" + re.escape(key) + r": (\d+)", line)
            if m and name:
                stats[name].setdefault(short, int(m.group(1)))
    return stats


def demangle(names):
    if not shutil.which("c++filt"):
        return {n: n for n in names}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def table(stats):
    pretty = demangle(sorted(stats))
    rows = [" vgpr  sgpr    lds scratch sspill vspill  occ  kernel"]
    for n in sorted(stats, key=lambda k: pretty[k]):
        s = stats[n]
        rows.append("%5d %5d %6d %7d %6d %6d %4d  %s" % tuple([s.get(k, 0) for _, k in KEYS] + [pretty[n]]))
    return rows


def main(parent, change):
    a, b = parse(parent), parse(change)
    common = sorted(set(a) & set(b))
    differ = [n for n in common if a[n] != b[n]]
    new = sorted(set(b) - set(a))
    gone = sorted(set(a) - set(b))
    pretty = demangle(sorted(set(a) | set(b)))
    print("kernels: parent %d, change %d; in both: %d; kernels in both whose figures differ: %d; new: %d; gone: %d"
          % (len(a), len(b), len(common), len(differ), len(new), len(gone)))
    for n in differ:
        print("  differs: %s\n    parent %s\n    change %s" % (pretty[n], a[n], b[n]))
    for n in gone:
        print("  gone: " + pretty[n])
    print("\n== NEW KERNELS ==")
    print("\n".join(table({n: b[n] for n in new})))
    print("\n== PARENT ==")
    print("\n".join(table(a)))
    print("\n== CHANGE ==")
    print("\n".join(table(b)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
