#!/usr/bin/env python
"""Grouped median by segmented radix select (csrc/segselect.hip) against the
two full sorts it replaces, and a GROUP BY with a percentile against the host
route such a query took before.

Kernel level: gpu._median_by_group with gpu.SEG_SELECT on and off, on uniform
group ids and on a skewed shape (one group holds half the rows), float64 and
int32 values; the select route's two parts (laying the column out by group,
the kernel) are also timed on their own.  Whole query: PERCENTILE_CONT plus two sums through SQL, against
the same aggregates with the percentile as a python callable, which is the
plan that sent the whole shard to host pandas.  The routes alternate in one
process after a warm-up of each shape, with device events around calls that
end in a synchronise.  One JSON line per cell with every timing;
"select_wins" is the rule for routing the median: the select route's slowest
timing beats the sort route's fastest.

Needs a GPU: there is nothing to measure without one.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def _alternate(routes, reps):
    """routes: name -> thunk.  One warm-up each, then reps rounds."""
    outs = {name: _time(fn)[1] for name, fn in routes.items()}
    ms = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            ms[name].append(round(_time(fn)[0], 3))
    return ms, outs


def _group_ids(gen, n, ngroups, skewed):
    gid = torch.randint(0, ngroups, (n,), generator=gen, device="cuda",
                        dtype=torch.int32)
    if skewed:  # group 0 takes every second row
        gid[::2] = 0
    return gid


def kernel_level(args):
    from bodo_amd.core import types as bt
    from bodo_amd.core.column import Column
    from bodo_amd.ops import gpu

    # what is measured here decides this, so it does not gate it
    gpu.SEG_SELECT_MEDIAN_MIN_GROUP_ROWS = 0
    for logn in args.log_rows:
        n = 1 << logn
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1234)
        cols = {
            "float64": Column(bt.float64, torch.randn(
                n, generator=gen, device="cuda", dtype=torch.float64)),
            "int32": Column(bt.int32, torch.randint(
                -2**31, 2**31 - 1, (n,), generator=gen, device="cuda",
                dtype=torch.int32)),
        }
        shapes = [(g, False) for g in args.groups] + [(args.groups[-2:][0], True)]
        for ngroups, skewed in shapes:
            gid = _group_ids(gen, n, ngroups, skewed)
            for name, col in cols.items():
                def route(on):
                    def run():
                        gpu.SEG_SELECT = on
                        try:
                            return gpu._median_by_group(col, gid, ngroups).data
                        finally:
                            gpu.SEG_SELECT = True
                    return run

                ms, outs = _alternate({"select": route(True),
                                       "sort": route(False)}, args.reps)
                # the select route's two parts, each on its own
                vals, seg_start, cnt, _ = gpu.group_segments(col, gid, ngroups)
                rank = (cnt - 1) // 2
                parts, _ = _alternate({
                    "segments": lambda: gpu.group_segments(col, gid, ngroups),
                    "seg_select": lambda: gpu.seg_select(vals, seg_start, rank),
                }, args.reps)
                print(json.dumps({
                    "level": "kernel", "values": name, "rows": n,
                    "groups": ngroups, "skewed": skewed,
                    **{f"{r}_ms": v for r, v in ms.items()},
                    **{f"{r}_ms": v for r, v in parts.items()},
                    "same_result": bool(torch.equal(
                        outs["select"].nan_to_num(), outs["sort"].nan_to_num())),
                    "select_wins": max(ms["select"]) < min(ms["sort"]),
                }), flush=True)
            del gid
        del cols
        torch.cuda.empty_cache()


def whole_query(args):
    import pandas as pd

    import bodo_amd.config as cfg
    import bodo_amd.pandas as bpd
    from bodo_amd.sql import BodoSQLContext

    cfg.DEVICE = "cuda"
    for logn in args.log_rows_whole:
        n = 1 << logn
        rng = np.random.default_rng(99)
        df = pd.DataFrame({"g": rng.integers(0, 10_000, n),
                           "x": rng.random(n), "a": rng.random(n),
                           "b": rng.integers(0, 100, n)})
        bdf = bpd.from_pandas(df)
        ctx = BodoSQLContext({"t": bdf})
        routes = {
            "kernel": lambda: ctx.sql(
                "select g, percentile_cont(0.9) within group (order by x) "
                "as p, sum(a) as sa, sum(b) as sb from t group by g"
            ).to_pandas(),
            "host": lambda: bdf.groupby("g", as_index=False).agg(
                p=bpd.NamedAgg("x", lambda s: s.quantile(0.9)),
                sa=bpd.NamedAgg("a", "sum"), sb=bpd.NamedAgg("b", "sum")
            ).to_pandas(),
        }
        ms, outs = _alternate(routes, args.reps)
        k, h = (outs[r].sort_values("g").reset_index(drop=True)
                for r in ("kernel", "host"))
        print(json.dumps({
            "level": "whole", "rows": n, "groups": 10_000,
            **{f"{r}_ms": v for r, v in ms.items()},
            "max_abs_diff": float((k[["p", "sa", "sb"]]
                                   - h[["p", "sa", "sb"]]).abs().max().max()),
            "kernel_wins": max(ms["kernel"]) < min(ms["host"]),
        }), flush=True)
        del bdf, ctx, df
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--log-rows", type=int, nargs="*", default=[24, 27])
    p.add_argument("--log-rows-whole", type=int, nargs="*", default=[24])
    p.add_argument("--groups", type=int, nargs="*",
                   default=[1, 100, 10_000, 1_000_000])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--level", choices=["kernel", "whole", "both"],
                   default="both")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_quantile.py needs a GPU")
    if args.level in ("kernel", "both"):
        kernel_level(args)
    if args.level in ("whole", "both"):
        whole_query(args)


if __name__ == "__main__":
    main()
