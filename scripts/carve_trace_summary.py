"""Per-configuration device times of the dense map's kernels from a `rocprofv3 --kernel-trace --output-format csv` run of
scripts/bench_densemap_carve.py: carve_trace_summary.py <kernel_trace.csv> <adds per configuration> <configs, e.g. off,1,4,16>.
The dispatches of k_dm_insert and of k_dm_carve are taken in time order and cut into one chunk per configuration; of each chunk the
first fifth (where the table still grows) is left out, and the median and the quartiles of the rest are printed in microseconds,
with the sum over the whole chunk (cells visited over that sum is the lookup rate)."""
import csv, sys
import numpy as np

path, per_cfg, cfgs = sys.argv[1], int(sys.argv[2]), sys.argv[3].split(",")
rows = list(csv.DictReader(open(path)))
name_col = next(c for c in rows[0] if c.lower() in ("kernel_name", "name"))
start_col = next(c for c in rows[0] if c.lower().startswith("start"))
end_col = next(c for c in rows[0] if c.lower().startswith("end"))


def durations(prefix):
    r = sorted((int(x[start_col]), int(x[end_col])) for x in rows if prefix in x[name_col])
    return np.array([(e - s) / 1e3 for s, e in r])


def show(label, d):
    total = d.sum()
    d = d[len(d) // 5:]
    print("  %-12s n %3d  median %8.1f us  quartiles %8.1f / %8.1f  max %8.1f  (all dispatches of the chunk: %.1f us)" % (
        label, len(d), np.median(d), np.percentile(d, 25), np.percentile(d, 75), d.max(), total))


ins, carve = durations("k_dm_insert"), durations("k_dm_carve")
n_carve_cfgs = sum(c != "off" for c in cfgs)
assert len(ins) == per_cfg * len(cfgs), (len(ins), per_cfg, cfgs)
assert len(carve) == per_cfg * n_carve_cfgs, (len(carve), per_cfg, cfgs)
k = 0
for i, c in enumerate(cfgs):
    print("config %s" % c)
    show("k_dm_insert", ins[i * per_cfg:(i + 1) * per_cfg])
    if c != "off":
        show("k_dm_carve", carve[k * per_cfg:(k + 1) * per_cfg])
        k += 1
