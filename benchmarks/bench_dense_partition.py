"""Both routes of groupby_dense_fused (atomic kernel, partitioned) over a
grid of table sizes and row counts, for the thresholds of the automatic
choice (csrc/kernels.hip DP_MIN_TABLE_BYTES / DP_MIN_ROWS).

    python benchmarks/bench_dense_partition.py [--reps 3]

Keys are uniform over the table, the aggregates are the flagship's (size and
a float64 sum with an invalid count).  Prints one JSON line per shape with
the fastest and slowest call of each route in ms (device events around the
whole call, which ends in the route's one host sync).
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INT8, INT16, INT32, FLOAT64 = 0, 1, 2, 5
AGG_SUM_F64, AGG_SIZE = 0, 7
ENV = "BODO_AMD_DENSE_PARTITION"


def time_route(K, args, mode, reps):
    os.environ[ENV] = mode
    times = []
    for r in range(reps + 1):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        out = K.groupby_dense_fused(*args)
        end.record()
        torch.cuda.synchronize()
        assert out, "key out of range"
        if r:  # the first call warms the allocator
            times.append(start.elapsed_time(end))
        del out
    return min(times), max(times)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--slots", type=int, nargs="*", default=[
        1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24, 16854000])
    p.add_argument("--rows", type=int, nargs="*", default=[
        1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28])
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from bodo_amd.ops import gpu

    K = gpu.kernels()
    gen = torch.Generator(device="cuda").manual_seed(7)
    for n in a.rows:
        value = torch.rand(n, device="cuda", dtype=torch.float64,
                           generator=gen)
        size_col = torch.zeros(1, dtype=torch.int8, device="cuda")
        for nslots in a.slots:
            key = torch.randint(0, nslots, (n,), device="cuda",
                                dtype=torch.int32, generator=gen)
            args = ([key], [INT32], [0], [nslots], [size_col, value],
                    [None, None], [INT8, FLOAT64], [AGG_SIZE, AGG_SUM_F64],
                    [0.0, 0.0], [0, 0], n)
            row = {"rows": n, "slots": nslots, "table_mb": nslots * 24 / 2**20}
            for mode, name in (("0", "atomic"), ("force", "partitioned")):
                lo, hi = time_route(K, args, mode, a.reps)
                row[name + "_ms"] = [round(lo, 3), round(hi, 3)]
            row["partitioned_wins"] = \
                row["partitioned_ms"][1] < row["atomic_ms"][0]
            print(json.dumps(row), flush=True)
            del key
    os.environ.pop(ENV, None)


if __name__ == "__main__":
    main()
