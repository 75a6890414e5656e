"""What the bench tools share: one JSON line per measurement, and device-event timing."""
import json
import os

import numpy as np
import torch

OUT = os.environ.get("RMT_BENCH_OUT")


def emit(**kw):
    """One JSON line on stdout, appended to the file named by RMT_BENCH_OUT when set."""
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def median(ms):
    return float(np.median(ms))


def timed(fn, reps, other=None, warm=3, stat=median):
    """stat (the median) of the device-event ms of fn over reps, after `warm` warm-ups; with
    other: [of fn, of other], the two alternating."""
    fns = [fn] + ([other] if other else [])
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for k, f in enumerate(fns):
            ev[k][r][0].record(); f(); ev[k][r][1].record()
    torch.cuda.synchronize()
    res = [stat([a.elapsed_time(b) for a, b in e]) for e in ev]
    return res if other else res[0]
