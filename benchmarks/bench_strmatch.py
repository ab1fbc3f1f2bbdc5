#!/usr/bin/env python
"""LIKE on a plain string column: the csrc/strmatch.hip route against the
host route (copy to host, arrow compute, copy back).

Two seeded columns: `comment`, o_comment-like rows of 19 to 78 bytes with the
pattern words planted in a few percent of them, and `long`, the same with
1 % of its rows of 64 KiB, whose tiles take the kernel's wave-per-row path.
Each TPC-H pattern is lowered as the SQL planner lowers it and timed through
str_op with config.STRING_MATCH on and off, alternated in one process after a
warm-up of each, device events around calls that end in a synchronise.  The
two routes' outputs are compared at the timed size.  One JSON line per
column and pattern; bytes/s counts the column's bytes and offsets and the
output once.

Needs a GPU: there is nothing to measure without one.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PATTERNS = ["%special%requests%", "%green%", "PROMO%", "%BRASS"]
LONG_ROW = 64 << 10


def make_column(n, long_every, gen):
    """Plain string column of n rows of 19..78 random lower-case bytes, every
    `long_every`-th row LONG_ROW bytes instead (0 = none), with the pattern
    words planted: 'special' and 'requests' each in 4 % of the rows, 'green'
    in 5 %, 'PROMO' at the start and 'BRASS' at the end of 10 %."""
    from bodo_amd.core import types as bt
    from bodo_amd.core.column import Column

    dev = "cuda"
    lens = torch.randint(19, 79, (n,), generator=gen, device=dev)
    if long_every:
        lens[::long_every] = LONG_ROW
    offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=offs[1:])
    nbytes = int(offs[-1])
    data = torch.randint(97, 123, (nbytes,), generator=gen, device=dev,
                         dtype=torch.uint8)

    def plant(word, share, where):
        k = int(n * share)
        rows = torch.randint(0, n, (k,), generator=gen, device=dev)
        w = torch.tensor(list(word.encode()), dtype=torch.uint8, device=dev)
        room = lens[rows] - len(w)
        at = {"start": torch.zeros_like(room), "end": room}.get(where)
        if at is None:
            at = (torch.rand(k, generator=gen, device=dev) * (room + 1)).long()
            at = torch.minimum(at, room)
        pos = offs[rows] + at
        data[pos[:, None] + torch.arange(len(w), device=dev)] = w

    plant("special", 0.04, "any")
    plant("requests", 0.04, "any")
    plant("green", 0.05, "any")
    plant("PROMO", 0.10, "start")
    plant("BRASS", 0.10, "end")
    return Column(bt.string, data, None, offsets=offs, length=n)


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=15_000_000)
    p.add_argument("--long-rows", type=int, default=1_000_000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--only", default="", help="comment or long")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_strmatch.py needs a GPU")

    from bodo_amd import config
    from bodo_amd.ops.evaluate import str_op
    from bodo_amd.plan.expr import ColRef
    from bodo_amd.sql.planner import _like_expr

    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    for name, n, long_every in (("comment", args.rows, 0),
                                ("long", args.long_rows, 100)):
        if args.only and name != args.only:
            continue
        col = make_column(n, long_every, gen)
        nbytes = col.data.numel() + col.offsets.numel() * 8 + n
        for pattern in PATTERNS:
            e = _like_expr(ColRef("c"), pattern)
            fn = lambda: str_op(col, e.op, e.args).data  # noqa: E731
            outs = {}
            for on in (True, False):  # warm-up of both routes
                config.STRING_MATCH = on
                outs[on] = _time(fn)[1]
            assert torch.equal(outs[True], outs[False]), (name, pattern)
            hits = int(outs[True].sum())
            del outs
            ms = {True: [], False: []}
            for _ in range(args.reps):
                for on in (True, False):
                    config.STRING_MATCH = on
                    ms[on].append(round(_time(fn)[0], 3))
            print(json.dumps({
                "column": name, "rows": n, "bytes": nbytes, "pattern": pattern,
                "op": e.op, "hits": hits, "same_result": True,
                "kernel_route_ms": ms[True], "host_route_ms": ms[False],
                "kernel_route_gbs": round(nbytes / min(ms[True]) / 1e6, 1),
                "host_route_gbs": round(nbytes / min(ms[False]) / 1e6, 3),
                "kernel_wins": max(ms[True]) <= min(ms[False])}), flush=True)
        config.STRING_MATCH = True
        del col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
