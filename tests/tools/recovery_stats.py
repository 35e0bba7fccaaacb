"""k_mcl_main and k_pf_recovery_fold per case and mode from the kernel traces of tests/tools/recovery_probe.py under
`rocprofv3 --kernel-trace --stats -f csv` (profiles/recovery_<mode>_kernel_trace.csv): launches, median, mean, min and max in us over
the steady updates (the first five moved updates of each case -- the interpolating first one and the warm-up -- left out).  Prints
the CSV that profiles/recovery_kernel_stats.csv holds."""
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rows(path):
    with open(path) as f:
        out = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    return sorted(out, key=lambda r: r[1])


def line(mode, case, kernel, d):
    return f"{mode},{case},{kernel},{len(d)},{statistics.median(d):.2f},{statistics.mean(d):.2f},{min(d):.2f},{max(d):.2f}"


def main():
    d = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    print("mode,case,kernel,launches,median_us,mean_us,min_us,max_us")
    for mode in ("parent", "off", "p0", "p25"):
        rs = rows(os.path.join(d, f"recovery_{mode}_kernel_trace.csv"))
        mcl = [(e - s) / 1000.0 for n, s, e in rs if n.startswith("void k_mcl_main")]
        half = len(mcl) // 2                 # the probe runs 200^2 / 100k first, then 2000^2 / 1M, the same number of updates each
        for case, sub in (("200^2/100k", mcl[:half]), ("2000^2/1M", mcl[half:])):
            print(line(mode, case, "k_mcl_main", sub[5:]))
        fold = [(e - s) / 1000.0 for n, s, e in rs if "k_pf_recovery_fold" in n]
        if fold:
            print(line(mode, "both", "k_pf_recovery_fold", fold))


if __name__ == "__main__":
    main()
