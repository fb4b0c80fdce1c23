"""Median duration of each kernel of a rocprofv3 --kernel-trace CSV, per kernel name and grid size (two shapes of one kernel in one run stay apart).
    python tools/kernel_trace_medians.py <..._kernel_trace.csv> [name filter]"""
import csv, statistics, sys


def main():
    path, want = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""
    runs = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if want in r["Kernel_Name"]:
                runs.setdefault((r["Kernel_Name"], int(r["Grid_Size_X"])), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    print("%-34s %10s %6s %10s %10s %10s" % ("kernel", "grid_x", "calls", "median_us", "min_us", "max_us"))
    for (name, grid), v in sorted(runs.items()):
        print("%-34s %10d %6d %10.2f %10.2f %10.2f" % (name, grid, len(v), statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3))


if __name__ == "__main__":
    main()
