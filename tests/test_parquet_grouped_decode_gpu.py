"""Pipelined shard read with one decompress launch per group of row
groups: two snappy files of three small row groups each, so a group of two
crosses a file boundary and leaves a remainder."""

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

pytestmark = pytest.mark.gpu

ROWS_PER_FILE = 15_000
N_FILES = 2
N_COLS = 5


@pytest.fixture(scope="module")
def shard(tmp_path_factory):
    d = tmp_path_factory.mktemp("grouped")
    rng = np.random.default_rng(77)
    for i in range(N_FILES):
        n = ROWS_PER_FILE
        nul = rng.integers(-10**12, 10**12, n).astype("float64")
        nul[rng.random(n) < 0.10] = np.nan
        df = pd.DataFrame({
            "loc": rng.integers(1, 266, n).astype("int64"),
            "f": rng.random(n),
            "nul": pd.array(nul).astype("Int64"),
            "s_dict": rng.choice(["alpha", "beta", "gamma", "delta"], n),
            "s_plain": np.array(["s" + str(v) for v in
                                 rng.integers(0, 10**9, n)], dtype=object),
        })
        pq.write_table(pa.Table.from_pandas(df, preserve_index=False),
                       str(d / f"part-{i:05d}.parquet"), compression="SNAPPY",
                       use_dictionary=["s_dict"], row_group_size=5000,
                       data_page_size=4096)
    ref = pa.concat_tables(
        [pq.read_table(str(d / f"part-{i:05d}.parquet"))
         for i in range(N_FILES)]).to_pandas()
    return str(d), ref


@pytest.mark.parametrize("group", [None, 1, 2, 4],
                         ids=["default", "g1", "g2", "g4"])
def test_grouped_decode_matches_pyarrow(shard, group, monkeypatch):
    from bodo_amd.engine.executor import ExecutionContext
    from bodo_amd.io import parquet_gpu as g

    path, ref = shard
    if group is not None:
        monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", group)
    ctx = ExecutionContext("cuda")
    ctx.world, ctx.rank = 1, 0
    slow, batched = g.STATS["slow"], g.STATS["batched"]
    t = g.read_shard_gpu(path, None, ctx)
    assert t is not None, "GPU decode fell back"
    assert g.STATS["slow"] == slow
    assert g.STATS["batched"] == batched + N_FILES * 3 * N_COLS
    out = t.to_pandas()
    for c in out.columns:
        if out[c].dtype.name == "category":
            out[c] = out[c].astype(object)
    assert list(out.columns) == list(ref.columns)
    assert len(out) == len(ref)
    for c in ref.columns:
        a, b = out[c], ref[c]
        assert (a.isna().to_numpy() == b.isna().to_numpy()).all(), c
        ok = ~b.isna().to_numpy()
        assert (a.to_numpy()[ok] == b.to_numpy()[ok]).all(), c
