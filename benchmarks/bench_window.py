#!/usr/bin/env python
"""Segmented-scan window route against the whole-tensor torch route.

Times window._ordered_local_device whole (the sort is common to both
routes) on one seeded frame per function, with the scan route on and off
alternated in one process after a warm-up of each, device events around
calls that end in a synchronise.  Then times the scan calls alone on
pre-sorted inputs, with the bytes each launch must move.  One JSON line per
function and per scan variant.  rolling_max(1000) has no "off" device time:
past width 128 the torch route hands the node to host pandas, so it is
reported alone.

`scan_wins` is the rule that sets the default route of the min/max family:
the scan route's slowest timing is no slower than the torch route's fastest.
Widths 3 and 4 stand on either side of
gpu.SEG_SCAN_ROLLING_MINMAX_MIN_WIDTH; "on" here means the kernels at every
width.

Needs a GPU: there is nothing to measure without one.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

# (name, value column, function, argument)
FUNCS = [
    ("cumsum_i64", "vi", "cumsum", None),
    ("cumsum_f64", "vf", "cumsum", None),
    ("cummax", "vf", "cummax", None),
    ("cummean", "vf", "cummean", None),
    ("rolling_sum_16", "vf", "rolling_sum", 16),
    ("rolling_max_2", "vf", "rolling_max", 2),
    ("rolling_max_3", "vf", "rolling_max", 3),
    ("rolling_max_4", "vf", "rolling_max", 4),
    ("rolling_max_16", "vf", "rolling_max", 16),
    ("rolling_max_128", "vf", "rolling_max", 128),
    ("rolling_max_1000", "vf", "rolling_max", 1000),
]
# (name, op, value dtype, reverse, want_count)
SCANS = [
    ("sum_i64", "sum_i64", torch.int64, False, False),
    ("sum_f64", "sum_f64", torch.float64, False, False),
    ("sum_f64_count", "sum_f64", torch.float64, False, True),
    ("max_f64_count", "max_f64", torch.float64, False, True),
    ("max_f64_count_reverse", "max_f64", torch.float64, True, True),
]


def scan_bytes(n, value_bytes, want_count):
    """Bytes per launch: reduce reads at most every value and head flag
    (it stops at the last head of each block's range, one tile per block
    when partitions are short), the spine is a few KiB, apply reads them
    all again and writes 8 B per output."""
    read = n * (value_bytes + 1)
    return {"reduce_max": read, "apply": read + n * 8 * (1 + want_count)}


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1 << 27)
    p.add_argument("--partitions", type=int, default=1 << 17)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--only", default="")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_window.py needs a GPU")
    assert args.reps >= 5, "at least five timings per side"

    from bodo_amd.core import types as bt
    from bodo_amd.core.column import Column
    from bodo_amd.core.table import Table
    from bodo_amd.engine import window
    from bodo_amd.ops import gpu

    n = args.rows
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    rnd = lambda lo, hi: torch.randint(  # noqa: E731
        lo, hi, (n,), generator=gen, device="cuda")
    # integer-valued floats: both routes' sums are exact, so they can be
    # compared bit for bit
    tbl = Table(["k", "o", "vi", "vf"], [
        Column(bt.int64, rnd(0, args.partitions), length=n),
        Column(bt.int64, rnd(0, 1 << 40), length=n),
        Column(bt.int64, rnd(-1000, 1000), length=n),
        Column(bt.float64, rnd(-1000, 1000).double(), length=n)], n)
    only = args.only.split(",") if args.only else None
    # "on" means the kernels at every width, also below the default threshold
    gpu.SEG_SCAN_ROLLING_MINMAX_MIN_WIDTH = 1

    for name, col, func, arg in FUNCS:
        if only and name not in only:
            continue
        spec = [("r", col, func, arg)]

        def fn():
            out = window._ordered_local_device(tbl, ["k"], ["o"], [True], spec)
            return None if out is None else out.column("r").data

        outs = {}
        for on in (True, False):  # warm-up of this function, both routes
            gpu.SEG_SCAN = on
            outs[on] = _time(fn)[1]
        has_off = outs[False] is not None
        same = has_off and bool(torch.equal(outs[True], outs[False]))
        del outs
        ms = {True: [], False: []}
        for _ in range(args.reps):
            for on in (True, False) if has_off else (True,):
                gpu.SEG_SCAN = on
                ms[on].append(round(_time(fn)[0], 3))
        print(json.dumps({
            "function": name, "rows": n, "partitions": args.partitions,
            "scan_ms": ms[True],
            "torch_ms": ms[False] if has_off else "no device route",
            "scan_wins": max(ms[True]) <= min(ms[False]) if has_off else None,
            "same_result": same if has_off else None}), flush=True)
        torch.cuda.empty_cache()
    gpu.SEG_SCAN = True

    heads = torch.zeros(n, dtype=torch.bool, device="cuda")
    heads[torch.randint(0, n, (args.partitions,), generator=gen,
                        device="cuda")] = True
    for name, op, dtype, reverse, want_count in SCANS:
        if only and name not in only:
            continue
        vals = rnd(-1000, 1000).to(dtype)
        fn = lambda: gpu.segmented_scan(  # noqa: E731
            vals, heads, op, reverse=reverse, want_count=want_count)
        _time(fn)
        ms = [round(_time(fn)[0], 3) for _ in range(args.reps)]
        nbytes = scan_bytes(n, vals.element_size(), want_count)
        print(json.dumps({
            "scan": name, "rows": n, "ms": ms, "bytes": nbytes,
            "apply_bytes_tbs": round(nbytes["apply"] / min(ms) / 1e9, 3)}),
            flush=True)
        del vals


if __name__ == "__main__":
    main()
