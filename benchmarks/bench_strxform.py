#!/usr/bin/env python
"""Transforms of a plain string column: the csrc/strxform.hip route against
the host route (copy to host, arrow compute or a pandas object series, copy
back).

Two seeded column shapes: `short`, rows of 8 to 24 random letters, and `mix`,
the same with every 4096th row of 64 KiB, whose tiles take the kernels'
wave-per-row paths.  Half the rows begin and half end with a blank.  Each op
is timed as the whole str_op call (concat as the whole eval_expr call) with
config.STRING_TRANSFORM on and off, alternated in one process after a warm-up
of each, device events around calls that end in a synchronise.  The two
routes' outputs are compared at the timed size.  One JSON line per shape, row
count and op, every repeat listed so the spread shows; bytes/s counts the
column's bytes and offsets once (twice the bytes for the ops that write
strings).

Needs a GPU: there is nothing to measure without one.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

LONG_ROW = 64 << 10
OPS = {"len": (), "lower": (), "upper": (), "strip": (), "lstrip": (),
       "rstrip": (), "slice": (1, 4, 1), "concat_literal": None,
       "concat_column": None}


def make_column(n, long_every, gen):
    from bodo_amd.core import types as bt
    from bodo_amd.core.column import Column

    dev = "cuda"
    lens = torch.randint(8, 25, (n,), generator=gen, device=dev)
    if long_every:
        lens[::long_every] = LONG_ROW
    offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=offs[1:])
    data = torch.randint(65, 123, (int(offs[-1]),), generator=gen, device=dev,
                         dtype=torch.uint8)
    data[(data > 90) & (data < 97)] = 101  # letters only
    for at in (offs[:-1], offs[1:] - 1):
        data[at[torch.rand(n, generator=gen, device=dev) < 0.5]] = 32
    return Column(bt.string, data, None, offsets=offs, length=n)


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def _same(x, y):
    return torch.equal(x.data, y.data) and \
        (x.offsets is None or torch.equal(x.offsets, y.offsets))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, nargs="+",
                   default=[1 << 20, 1 << 22, 1 << 24])
    p.add_argument("--shapes", nargs="+", default=["short", "mix"])
    p.add_argument("--ops", nargs="+", default=list(OPS))
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_strxform.py needs a GPU")

    from bodo_amd import config
    from bodo_amd.core.table import Table
    from bodo_amd.ops.evaluate import eval_expr, str_op
    from bodo_amd.plan.expr import BinOp, ColRef, Const

    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    for shape in args.shapes:
        for n in args.rows:
            col = make_column(n, 4096 if shape == "mix" else 0, gen)
            tbl = Table(["c"], [col])
            nbytes = col.data.numel() + col.offsets.numel() * 8
            for op in args.ops:
                if op == "concat_literal":
                    e = BinOp("concat", ColRef("c"), Const("-x"))
                    fn = lambda: eval_expr(e, tbl)  # noqa: E731
                elif op == "concat_column":
                    e = BinOp("concat", ColRef("c"), ColRef("c"))
                    fn = lambda: eval_expr(e, tbl)  # noqa: E731
                else:
                    fn = lambda: str_op(col, op, OPS[op])  # noqa: E731
                outs = {}
                for on in (True, False):  # warm-up of both routes
                    config.STRING_TRANSFORM = on
                    outs[on] = _time(fn)[1]
                assert _same(outs[True], outs[False]), (shape, n, op)
                del outs
                ms = {True: [], False: []}
                for _ in range(args.reps):
                    for on in (True, False):
                        config.STRING_TRANSFORM = on
                        ms[on].append(round(_time(fn)[0], 3))
                moved = nbytes if op == "len" else nbytes + col.data.numel()
                print(json.dumps({
                    "shape": shape, "rows": n, "bytes": nbytes, "op": op,
                    "same_result": True,
                    "kernel_route_ms": ms[True], "host_route_ms": ms[False],
                    "kernel_route_gbs": round(moved / min(ms[True]) / 1e6, 1),
                    "host_route_gbs": round(moved / min(ms[False]) / 1e6, 3),
                    "kernel_wins": max(ms[True]) <= min(ms[False])}),
                    flush=True)
            config.STRING_TRANSFORM = True
            del col, tbl
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
