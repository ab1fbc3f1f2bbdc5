#!/usr/bin/env python
"""Radix select (csrc/select.hip) against a full sort, kernel level and whole
call.

Kernel level: gpu.radix_select plus the sort of its k rows, against
torch.argsort(stable=True)[:k] and, on plain keys, torch.topk.  Whole call:
df.nlargest and a two-key ORDER BY ... LIMIT on an 8-column table with the
route on, with it off (full sort_indices, k rows gathered), and on the plan
the executor ran before it had a one-GPU top-k path (full sort, full-width
gather, slice).  The routes alternate in one process after a warm-up of each
shape, with device events around calls that end in a synchronise.  One JSON
line per cell with every timing; "select_wins" is the rule that sets
gpu.TOPK_SELECT_MIN_ROWS and TOPK_SELECT_MAX_FRACTION: the select route's
slowest timing beats the other route's fastest.

Needs a GPU: there is nothing to measure without one.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def key_shapes():
    """name -> (builder(gen, n), (begin_bit, end_bit), ties, plain)"""
    def ri(lo, hi, dtype):
        return lambda g, n: torch.randint(lo, hi, (n,), generator=g,
                                          device="cuda", dtype=dtype)
    return {
        "int32": (ri(-2**31, 2**31 - 1, torch.int32), (0, 32), "first", True),
        "int64": (ri(-2**63, 2**63 - 1, torch.int64), (0, 64), "first", True),
        "float64": (lambda g, n: torch.randn(
            n, generator=g, device="cuda", dtype=torch.float64),
            (0, 64), "first", True),
        "packed40": (ri(0, 2**40, torch.int64), (0, 40), "first", False),
        "three_first": (ri(0, 3, torch.int64), (0, 64), "first", True),
        "three_all": (ri(0, 3, torch.int64), (0, 64), "all", False),
    }


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


def _spread(v):
    return round(max(v) - min(v), 3)


def kernel_level(args):
    from bodo_amd.ops import gpu

    for name, (build, (b0, b1), ties, plain) in key_shapes().items():
        if args.only and name not in args.only.split(","):
            continue
        for logn in args.log_rows:
            n = 1 << logn
            gen = torch.Generator(device="cuda")
            gen.manual_seed(1234)
            keys = build(gen, n)
            for k in (10, 1000, 100_000, n // 16):
                def select():
                    cand = gpu.radix_select(keys, k, b0, b1, ties=ties,
                                            max_out=4 * k)
                    if cand is None:
                        return None
                    sub = keys[cand]
                    return cand[torch.argsort(sub, stable=True)][:k]

                routes = {"select": select, "argsort": lambda: torch.argsort(
                    keys, stable=True)[:k]}
                if plain:
                    routes["topk"] = lambda: torch.topk(
                        keys, k, largest=False, sorted=True).indices
                ms, outs = _alternate(routes, args.reps)
                passes = -(-(b1 - b0) // 8)
                print(json.dumps({
                    "level": "kernel", "keys": name, "rows": n, "k": k,
                    "ties": ties, **{f"{r}_ms": v for r, v in ms.items()},
                    "argsort_spread_ms": _spread(ms["argsort"]),
                    "returned_none": outs["select"] is None,
                    "same_result": outs["select"] is None or bool(
                        torch.equal(outs["select"], outs["argsort"])),
                    # first pass, emission count and scatter read the column;
                    # the other passes read it only without a survivor buffer
                    "min_key_bytes": 3 * n * keys.element_size(),
                    "max_key_bytes": (passes + 2) * n * keys.element_size(),
                    "select_wins": max(ms["select"]) < min(ms["argsort"]),
                }), flush=True)
            del keys
            torch.cuda.empty_cache()


def whole_call(args):
    import pandas as pd

    import bodo_amd.config as cfg
    import bodo_amd.pandas as bpd
    from bodo_amd.engine import executor
    from bodo_amd.ops import gpu
    from bodo_amd.sql import BodoSQLContext

    cfg.DEVICE = "cuda"
    topk_max = executor._TOPK_MAX
    # what is measured here decides these two, so they do not gate it
    gpu.TOPK_SELECT_MIN_ROWS, gpu.TOPK_SELECT_MAX_FRACTION = 0, 1.0
    for logn in args.log_rows_whole:
        n = 1 << logn
        rng = np.random.default_rng(99)
        df = pd.DataFrame({
            "a": rng.integers(0, 1 << 20, n) / 8.0,
            "b": rng.integers(-2**40, 2**40, n),
            **{f"c{i}": rng.random(n) for i in range(6)}})
        bdf = bpd.from_pandas(df)
        ctx = BodoSQLContext({"t": bdf})
        for k in (10, 1000, 100_000):
            calls = {
                "nlargest": lambda: bdf.nlargest(k, "b").to_pandas(),
                "order_by_2": lambda: ctx.sql(
                    "select * from t order by a desc, b limit %d" % k
                ).to_pandas(),
            }
            for cname, call in calls.items():
                def route(on, parent=False):
                    def run():
                        gpu.TOPK_SELECT = on
                        executor._TOPK_MAX = -1 if parent else topk_max
                        try:
                            return call()
                        finally:
                            gpu.TOPK_SELECT = True
                            executor._TOPK_MAX = topk_max
                    return run

                ms, outs = _alternate({
                    "select": route(True), "sort_prefix": route(False),
                    "full_sort_plan": route(False, parent=True)}, args.reps)
                other = ms["sort_prefix"] + ms["full_sort_plan"]
                print(json.dumps({
                    "level": "whole", "call": cname, "rows": n, "k": k,
                    **{f"{r}_ms": v for r, v in ms.items()},
                    "sort_prefix_spread_ms": _spread(ms["sort_prefix"]),
                    "same_result": bool(
                        outs["select"].reset_index(drop=True).equals(
                            outs["full_sort_plan"].reset_index(drop=True))),
                    "select_wins": max(ms["select"]) < min(other),
                }), flush=True)
        del bdf, ctx, df
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--log-rows", type=int, nargs="*", default=[20, 24, 27])
    p.add_argument("--log-rows-whole", type=int, nargs="*", default=[20, 24])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--only", default="", help="comma-separated key shapes")
    p.add_argument("--level", choices=["kernel", "whole", "both"],
                   default="both")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_topk.py needs a GPU")
    if args.level in ("kernel", "both"):
        kernel_level(args)
    if args.level in ("whole", "both"):
        whole_call(args)


if __name__ == "__main__":
    main()
