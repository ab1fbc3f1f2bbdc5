#!/usr/bin/env python
"""Flagship benchmark: NYC-Taxi Q1 ("Monthly Trips with Precipitation",
BASELINE.md config 2/3) on synthetic FHVHV-shaped data, N MI355X GPUs.

Reference: benchmarks/nyc_taxi/bodo/nyc_taxi_precipitation.py (query shape),
run on 1,036,465,968 rows x the columns the query touches
(benchmarks/nyc_taxi/README.md).  Data is synthetic and resident in HBM
(there is no network for the S3 dataset); generation is untimed; the timed
region is the full query: datetime extraction, inner merge with weather,
UDF time-bucketing, 6-key hash groupby (count + mean), and sort.

Driver contract:
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W
Rank 0 prints one JSON line with the aggregate rows/sec.

A plain run sets up, warms up, times the steps and prints the result line.
--dump-outputs DIR also writes the last timed step's result as .npy arrays;
--full is reserved for anything measured beyond the headline figure.
"""

import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

TOTAL_ROWS = 1_036_465_968  # FHVHV row count, benchmarks/nyc_taxi/README.md
N_LOCATIONS = 265
YEAR_NS = 365 * 86400 * 10**9
BASE_TS = 1_672_531_200_000_000_000  # 2023-01-01


def make_trips_shard(n, rank, device):
    """Synthetic trips shard generated directly in HBM."""
    import pyarrow as pa

    from bodo_amd.core import types as bt
    from bodo_amd.core.column import Column
    from bodo_amd.core.table import Table

    g = torch.Generator(device=device)
    g.manual_seed(12345 + rank)
    dev = torch.device(device)
    pickup = BASE_TS + torch.randint(0, YEAR_NS, (n,), generator=g,
                                     dtype=torch.int64, device=dev)
    pu = torch.randint(1, N_LOCATIONS + 1, (n,), generator=g,
                       dtype=torch.int64, device=dev)
    do = torch.randint(1, N_LOCATIONS + 1, (n,), generator=g,
                       dtype=torch.int64, device=dev)
    miles = torch.rand(n, generator=g, dtype=torch.float64, device=dev) * 20.0
    lic = torch.randint(0, 4, (n,), generator=g, dtype=torch.int32, device=dev)
    lic_dict = pa.array(["HV0002", "HV0003", "HV0004", "HV0005"],
                        type=pa.large_string())
    pu_col = Column(bt.int64, pu)
    pu_col.val_range = (1, N_LOCATIONS)
    do_col = Column(bt.int64, do)
    do_col.val_range = (1, N_LOCATIONS)
    cols = {
        "hvfhs_license_num": Column(bt.dictionary, lic, dictionary=lic_dict),
        "pickup_datetime": Column(bt.timestamp_ns, pickup),
        "PULocationID": pu_col,
        "DOLocationID": do_col,
        "trip_miles": Column(bt.float64, miles),
    }
    return Table(list(cols), list(cols.values()), n)


def make_weather():
    import pandas as pd

    rng = np.random.default_rng(7)
    dates = pd.date_range("2023-01-01", "2023-12-31")
    return pd.DataFrame({"DATE": dates,
                         "PRCP": rng.exponential(0.05, len(dates)).round(2)})


def get_time_bucket(t):
    if t in (8, 9, 10):
        return "morning"
    if t in (11, 12, 13, 14, 15):
        return "midday"
    if t in (16, 17, 18):
        return "afternoon"
    if t in (19, 20, 21):
        return "evening"
    return "other"


def run_query(bpd, trips_table, weather_df):
    """The exact NYC-Taxi Q1 query shape through the lazy frontend."""
    from bodo_amd.engine import executor as ex
    from bodo_amd.pandas.frame import BodoDataFrame
    from bodo_amd.plan import nodes as pn

    key = ex.register_object(trips_table)
    t = BodoDataFrame(pn.PandasScan(key, tuple(trips_table.names),
                                    distributed=True),
                      list(trips_table.names))
    w = bpd.from_pandas(weather_df)
    w = w.rename(columns={"DATE": "date", "PRCP": "precipitation"})
    w["date"] = w["date"].dt.date
    t["date"] = t["pickup_datetime"].dt.date
    t["month"] = t["pickup_datetime"].dt.month
    t["hour"] = t["pickup_datetime"].dt.hour
    t["weekday"] = t["pickup_datetime"].dt.dayofweek.isin([0, 1, 2, 3, 4])
    m = t.merge(w, on="date", how="inner")
    m["date_with_precipitation"] = m["precipitation"] > 0.1
    m["time_bucket"] = m.hour.map(get_time_bucket)
    g = m.groupby(
        ["PULocationID", "DOLocationID", "month", "weekday",
         "date_with_precipitation", "time_bucket"],
        as_index=False).agg(
        trips=bpd.NamedAgg("hvfhs_license_num", "count"),
        avg_distance=bpd.NamedAgg("trip_miles", "mean"))
    g = g.sort_values(
        by=["PULocationID", "DOLocationID", "month", "weekday",
            "date_with_precipitation", "time_bucket"])
    shard = g.execute()  # materialized device shard
    ex.delete_object(key)
    return shard


def trips_parquet_dir(n_local, rank, world, device):
    """Where this rank's trips shard lives as parquet.  The shard is a pure
    function of this file (seeds, schema, writer settings), the torch
    version and the shard's place in the run, so the name is a hash of
    those and a later run with the same arguments finds the files of an
    earlier one instead of encoding 22 GB again.  Entries of the scratch
    directory that nobody wrote or reused for six hours are removed."""
    with open(os.path.abspath(__file__), "rb") as f:
        h = hashlib.sha1(f.read())
    h.update(f"|{torch.__version__}|{device}|{n_local}|{rank}|{world}"
             .encode())
    base = os.path.join(tempfile.gettempdir(), f"bodo_bench_pq_{os.getuid()}")
    os.makedirs(base, exist_ok=True)
    for name in os.listdir(base):
        old = os.path.join(base, name)
        try:
            if time.time() - os.path.getmtime(old) > 6 * 3600:
                shutil.rmtree(old, ignore_errors=True)
        except OSError:
            pass
    return os.path.join(base, f"trips_{h.hexdigest()[:16]}")


def write_trips_parquet(trips, pq_dir, n_threads=12):
    """Write the shard as a directory of snappy parquet files, one per
    2**24-row chunk (two 2**23-row row groups each), encoded by a thread
    pool.  The row groups, and their order under the reader's sorted file
    listing, are the ones a single sequential writer produces; only the
    encoding runs in parallel.  Host staging stays bounded at one chunk
    (~0.6 GB) per thread.  The files appear under pq_dir's final name only
    once all are complete, so a reader never meets a partial shard."""
    import pyarrow.parquet as pq

    from bodo_amd import ops as _ops

    final_dir, pq_dir = pq_dir, f"{pq_dir}.tmp{os.getpid()}"
    shutil.rmtree(pq_dir, ignore_errors=True)
    os.makedirs(pq_dir)
    CHUNK = 1 << 24

    def write_chunk(i):
        s = i * CHUNK
        at = _ops.slice_table(trips, s, min(s + CHUNK, len(trips))) \
            .to_device("cpu").to_arrow()
        path = os.path.join(pq_dir, f"part-{i:05d}.parquet")
        with pq.ParquetWriter(path, at.schema, compression="SNAPPY",
                              use_dictionary=["hvfhs_license_num"]) as writer:
            writer.write_table(at, row_group_size=1 << 23)
        return os.path.getsize(path)

    n_chunks = max(1, -(-len(trips) // CHUNK))
    with ThreadPoolExecutor(max_workers=n_threads) as pool:
        n_bytes = sum(pool.map(write_chunk, range(n_chunks)))
    try:
        os.rename(pq_dir, final_dir)
    except OSError:  # another run finished the same shard first: use theirs
        shutil.rmtree(pq_dir, ignore_errors=True)
    return n_bytes


def dump_outputs(shard, out_dir, rank, world, max_rows=1 << 19):
    """Write the last timed step's result shard as <column>.npy (float64).
    A result larger than max_rows is cut to a fixed seeded sample of its
    rows (ascending, so the sort order is kept); string columns are stored
    as the rank of each value among the sample's sorted distinct values.
    num_rows.npy holds the full shard length."""
    import pandas as pd

    from bodo_amd import ops as _ops

    os.makedirs(out_dir, exist_ok=True)
    n = len(shard)
    if n > max_rows:
        idx = np.sort(np.random.default_rng(2023).choice(
            n, max_rows, replace=False))
        shard = _ops.take_table(
            shard, torch.from_numpy(idx).to(shard.device))
    df = shard.to_device("cpu").to_pandas()
    suffix = "" if world == 1 else f"_rank{rank}"
    arrays = {"num_rows": np.array([n], dtype=np.float64)}
    for name in df.columns:
        col = df[name]
        if not (pd.api.types.is_numeric_dtype(col.dtype)
                or pd.api.types.is_bool_dtype(col.dtype)):
            col = col.astype(str)
            col = pd.Categorical(col, categories=sorted(col.unique())).codes
        arrays[name] = np.asarray(col, dtype=np.float64)
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), arr)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--rows", type=int, default=TOTAL_ROWS,
                   help="total rows (dev override; judged runs use default)")
    p.add_argument("--parquet", action="store_true", default=True,
                   help="read the trips table from snappy parquet each step "
                        "with on-GPU decode (BASELINE config 2; the default)")
    p.add_argument("--no-parquet", dest="parquet", action="store_false",
                   help="skip parquet IO: query in-HBM synthetic shards")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last step's result "
                        "as DIR/<column>.npy (float64; a fixed seeded row "
                        "sample when the result is large)")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements beyond the headline "
                        "figure (none at present: a plain run already does "
                        "only setup, warmup, the timed steps and the result)")
    args = p.parse_args()

    import bodo_amd  # noqa: F401  (inits process group under torchrun)
    import bodo_amd.config as cfg
    from bodo_amd.parallel import comm

    on_gpu = torch.cuda.is_available()
    device = "cuda" if on_gpu else "cpu"
    cfg.DEVICE = device
    if on_gpu:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
    rank, world = comm.get_rank(), comm.get_world_size()
    if on_gpu:
        import bodo_amd_kernels  # noqa: F401 - fail loudly if ext missing
    import bodo_amd.pandas as bpd

    n_total = args.rows
    base, rem = divmod(n_total, world)
    n_local = base + (1 if rank < rem else 0)
    weather = make_weather()

    def log(msg):
        if rank == 0:
            print(f"[bench +{time.perf_counter() - T0:.1f}s] {msg}",
                  file=sys.stderr, flush=True)

    T0 = time.perf_counter()
    trips = None
    pq_path = None
    if args.parquet:
        # this rank's shard as snappy parquet (untimed; the realistic
        # on-disk layout); each step re-reads it with the on-GPU decoder
        # before the query
        pq_path = trips_parquet_dir(n_local, rank, world, device)
    if pq_path is not None and os.path.isdir(pq_path):
        os.utime(pq_path)  # in use: keep it from the age sweep
        log(f"parquet reused: {pq_path}")
    else:
        trips = make_trips_shard(n_local, rank, device)
        log(f"generated {n_local} rows on {device}")
    if pq_path is not None and trips is not None:
        pq_bytes = write_trips_parquet(trips, pq_path)
        # the generated device table is only the write source; freeing it
        # returns ~37 GB of HBM to the query working set at 1B rows
        del trips
        trips = None
        if on_gpu:
            torch.cuda.empty_cache()
        log(f"parquet written: {pq_bytes} bytes")

    def read_trips():
        if pq_path is None:
            return trips
        from bodo_amd.engine.executor import ExecutionContext
        from bodo_amd.io import parquet_gpu

        ctx1 = ExecutionContext(device)
        ctx1.world, ctx1.rank = 1, 0  # rank-private file
        if on_gpu:
            t = parquet_gpu.read_shard_gpu(pq_path, None, ctx1)
            assert t is not None, "GPU parquet decode fell back"
            return t
        from bodo_amd.io import parquet as pio

        return pio.read_shard(pq_path, None, (), ctx1)

    def one_step():
        shard = run_query(bpd, read_trips(), weather)
        return sum(comm.allgather_obj(len(shard))), shard

    for _ in range(args.warmup):
        one_step()
        log("warmup step done")
    comm.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out_rows = 0
    last_shard = None
    for i in range(args.steps):
        out_rows, shard = one_step()
        if i == args.steps - 1:
            last_shard = shard
        del shard
        log("timed step done")
    if on_gpu:
        torch.cuda.synchronize()
    comm.barrier()
    elapsed = time.perf_counter() - t0
    elapsed = max(comm.allgather_obj(elapsed))
    ms_per_step = elapsed / args.steps * 1000.0
    rows_per_sec = n_total / (elapsed / args.steps)
    if args.dump_outputs and last_shard is not None:
        dump_outputs(last_shard, args.dump_outputs, rank, world)
        log(f"outputs written to {args.dump_outputs}")
    if rank == 0:
        print(json.dumps({
            "metric": "nyc_taxi_q1_rows_per_sec",
            "value": rows_per_sec,
            "unit": "rows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "fp64",
            "data": ("synthetic snappy parquet (on-GPU decode in timed "
                     "region)" if args.parquet else
                     "synthetic (in-HBM, generation untimed; no parquet IO)"),
            "config": {
                "model": "nyc_taxi_q1_monthly_trips_precipitation",
                "rows": n_total,
                "out_groups": out_rows,
                "query": "dt-extract + inner-merge(weather) + udf-bucket + "
                         "6-key groupby(count,mean) + sort",
                "parallelism": f"dp{world}-hash-shuffle-rccl",
            },
        }), flush=True)


if __name__ == "__main__":
    main()
