"""Read the kernel-trace CSVs of tools/probes/adamw_segments_times.py (one per sample) and print, per sample and buffer size, the mean time
of the 12 launches after warm-up of adamw_guarded_kernel and of adamw_segments_kernel with 1 and with 26 segments.
Usage: python tools/probes/adamw_segments_parse.py TRACE.csv [TRACE.csv ...]"""
import csv
import sys

REPS, WARM = 15, 3
for path in sys.argv[1:]:
    rows = list(csv.DictReader(open(path)))
    runs = {}   # (kernel, grid) -> [duration in us, in launch order]
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"]
        for k in ("adamw_guarded_kernel", "adamw_segments_kernel"):
            if k in name:
                runs.setdefault((k, int(r["Grid_Size_X"])), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (k, grid), d in sorted(runs.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        chunks = [d[i:i + REPS] for i in range(0, len(d), REPS)]
        for c, label in zip(chunks, ("",) if k == "adamw_guarded_kernel" else (" 1 segment", " 26 segments")):
            t = c[WARM:]
            print("%s: grid %9d threads  %-22s%-12s mean %8.2f us  min %8.2f  max %8.2f  (%d launches)" % (
                path.split("/")[-3] if path.count("/") >= 3 else path, grid, k, label, sum(t) / len(t), min(t), max(t), len(t)))
