"""Per-step durations of the DCT-I launches in a rocprofv3 kernel trace of bench.py
(`rocprofv3 --kernel-trace --stats -f csv -- python bench.py --gpus 1 --steps 12`; kernel names
not truncated, so that the SOLVE template argument shows): around every column solve, the
two row passes before it (the early rows beside the chain, the marked rows after it) and the
one after it (inverse rows).  Means over the last 12 steps, microseconds.
    python tools/dct_launches.py <..._kernel_trace.csv>"""
import csv
import sys

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        nm = r["Kernel_Name"]
        if "k_dct1" in nm:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), nm))
rows.sort()
steps = []
for i, (s, e, nm) in enumerate(rows):
    if ("k_dct1<true" in nm or "k_dct1s<true" in nm) and i >= 2 and i + 1 < len(rows):
        d = lambda j: (rows[j][1] - rows[j][0]) / 1e3
        steps.append((d(i - 2), d(i - 1), d(i), d(i + 1)))
print("kernels:", sorted({nm[:60] for _, _, nm in rows}))
print("solves seen:", len(steps))
last = steps[-12:]
for k, n in enumerate(("early_rows", "marked_rows", "column_solve", "inverse_rows")):
    v = [s[k] for s in last]
    print(f"{n:13s} mean {sum(v) / len(v):8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}")
post = [s[1] + s[2] + s[3] for s in last]
print(f"post-chain sum (marked + solve + inverse) mean {sum(post) / len(post):8.1f} us; "
      f"with early rows {sum(sum(s) for s in last) / len(last):8.1f} us")
