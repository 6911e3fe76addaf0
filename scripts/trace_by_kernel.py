"""Device times per kernel name from a `rocprofv3 --kernel-trace --output-format csv` run:
trace_by_kernel.py <kernel_trace.csv> [name-substring ...] [--skip-first N]
Per kernel name (template arguments included) that contains one of the substrings: the number of dispatches, the median, the
quartiles and the maximum of their durations in microseconds; --skip-first leaves out the first N dispatches of each name."""
import csv, sys
import numpy as np

args = sys.argv[1:]
skip = 0
if "--skip-first" in args:
    i = args.index("--skip-first")
    skip = int(args[i + 1])
    del args[i:i + 2]
rows = list(csv.DictReader(open(args[0])))
name_col = next(c for c in rows[0] if c.lower() in ("kernel_name", "name"))
start_col = next(c for c in rows[0] if c.lower().startswith("start"))
end_col = next(c for c in rows[0] if c.lower().startswith("end"))
by = {}
for x in sorted(rows, key=lambda x: int(x[start_col])):
    if not args[1:] or any(p in x[name_col] for p in args[1:]):
        by.setdefault(x[name_col].split("(")[0], []).append((int(x[end_col]) - int(x[start_col])) / 1e3)
for name in sorted(by):
    d = np.array(by[name][skip:])
    if len(d):
        print("%-70s n %4d  median %8.1f us  quartiles %8.1f / %8.1f  max %8.1f" % (
            name, len(d), np.median(d), np.percentile(d, 25), np.percentile(d, 75), d.max()))
