"""Per-kernel medians of a rocprofv3 --kernel-trace CSV of
    python tools/rtcp_rate.py --variants stats,stats_report,stats_sm,stats_report_sm --out ""
told apart by the list the call ran on.  A stats call starts with its fill kernel; the tool's two checking calls come first (frame-major, stream-major), then
every round runs two calls on the frame-major list and two on the stream-major one.
    python tools/rtcp_trace_split.py <..._kernel_trace.csv>"""
import csv, statistics, sys


def main():
    rows = []
    with open(sys.argv[1], newline="") as f:
        for r in csv.DictReader(f):
            if "lc3_rtcp" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    call, runs = -1, {}
    for _, name, grid, ns in rows:
        if name == "lc3_rtcp_fill_kernel":
            call += 1
        order = ("frame_major", "stream_major")[call] if call < 2 else ("frame_major", "stream_major")[(call - 2) % 4 // 2]
        runs.setdefault((order, name, grid), []).append(ns)
    for order in ("frame_major", "stream_major"):
        print("# the %s list" % order.replace("_", "-"))
        print("%-26s %8s %6s %10s %10s %10s" % ("kernel", "grid_x", "calls", "median_us", "min_us", "max_us"))
        total = 0.0
        for (o, name, grid), v in sorted(runs.items()):
            if o == order:
                total += statistics.median(v) / 1e3
                print("%-26s %8d %6d %10.2f %10.2f %10.2f" % (name, grid, len(v), statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3))
        print("%-26s %8s %6s %10.2f" % ("sum of the medians", "", "", total))


if __name__ == "__main__":
    main()
