"""Quantile aggregates away from the GPU: the rank and interpolation
arithmetic against numpy, groupby().quantile and the SQL percentiles on the
CPU backend against pandas, and the single-phase shuffle on two gloo ranks.

bodo_amd is imported inside the tests: a gloo rank unpickles its query from
this module before it has its rank in the environment, and the package
joins the process group when it is first imported."""

import numpy as np
import pandas as pd
import pytest
import torch

INTERPOLATIONS = ["linear", "lower", "higher", "midpoint", "nearest"]


@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
@pytest.mark.parametrize("q", [0, 0.25, 0.5, 0.9, 1])
def test_ranks_and_finish_equal_numpy(q, interpolation):
    from bodo_amd.ops import gpu

    rng = np.random.default_rng(0)
    counts = [0, 1, 2, 3, 10]
    segs = [np.sort(rng.integers(-50, 50, c) / 8.0) for c in counts]
    cnt = torch.tensor(counts)
    rank = gpu.quantile_ranks(cnt, q, interpolation)
    pick = lambda s, r: s[min(r, len(s) - 1)] if len(s) else 0.0
    lo = torch.tensor([pick(s, int(r)) for s, r in zip(segs, rank)])
    hi = torch.tensor([pick(s, int(r) + 1) for s, r in zip(segs, rank)])
    got = gpu.quantile_finish(lo, hi, cnt, q, interpolation).numpy()
    exp = [np.quantile(s, q, method=interpolation) if len(s) else np.nan
           for s in segs]
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, exp)


def test_quantile_agg_is_a_plain_value():
    from bodo_amd.ops import gpu
    from bodo_amd.plan.nodes import QuantileAgg

    assert QuantileAgg(0.5) == QuantileAgg(0.5, "linear")
    assert len({QuantileAgg(0.5), QuantileAgg(0.5), QuantileAgg(0.5, "lower")}) == 2
    assert not callable(QuantileAgg(0.5))
    with pytest.raises(ValueError):
        gpu.quantile_ranks(torch.tensor([3]), 1.5)
    with pytest.raises(ValueError):
        gpu.quantile_ranks(torch.tensor([3]), 0.5, "cubic")


def _frame():
    rng = np.random.default_rng(1)
    x = rng.integers(-100, 100, 500) / 4.0
    x[rng.random(500) < 0.1] = np.nan
    return pd.DataFrame({"g": rng.integers(0, 12, 500), "x": x,
                         "i": rng.integers(-99, 99, 500)})


@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
def test_groupby_quantile_cpu(interpolation):
    import bodo_amd.pandas as bpd

    df = _frame()
    got = bpd.from_pandas(df).groupby("g", as_index=False).quantile(
        0.3, interpolation=interpolation).to_pandas().sort_values("g")
    # Series.quantile per group: numpy's half-to-even `nearest`, which pandas'
    # own groupby.quantile does not share on exact ties
    exp = df.groupby("g").agg(
        lambda s: s.quantile(0.3, interpolation=interpolation))
    for c in ("x", "i"):
        np.testing.assert_array_equal(got[c].to_numpy(), exp[c].to_numpy())


def test_sql_percentiles_cpu():
    """What the python-lambda plan of these aggregates gave."""
    from bodo_amd.sql import BodoSQLContext

    df = _frame()
    got = BodoSQLContext({"t": df}).sql(
        "select g, percentile_cont(0.3) within group (order by x) as pc, "
        "percentile_disc(0.7) within group (order by i) as pd, "
        "sum(i) as s from t group by g").to_pandas().sort_values("g")
    gb = df.groupby("g")
    np.testing.assert_array_equal(
        got["pc"].to_numpy(), gb["x"].agg(lambda s: s.quantile(0.3)))
    np.testing.assert_array_equal(
        got["pd"].to_numpy(),
        gb["i"].agg(lambda s: s.quantile(0.7, interpolation="nearest")))
    one = BodoSQLContext({"t": df}).sql(
        "select percentile_cont(0.3) within group (order by x) as pc from t"
    ).to_pandas()
    assert one["pc"].iloc[0] == df["x"].quantile(0.3)


def _q_quantile(bpd, rank, payload):
    from bodo_amd.parallel import comm
    from bodo_amd.plan.nodes import QuantileAgg

    assert comm.get_world_size() == 2
    return bpd.from_pandas(payload["df"]).groupby("g", as_index=False).agg(
        p=bpd.NamedAgg("x", QuantileAgg(0.3, "midpoint")),
        s=bpd.NamedAgg("i", "sum")).sort_values("g")


@pytest.mark.multi_rank
def test_quantile_agg_two_ranks():
    from test_distributed import run_dist

    df = _frame()
    got = run_dist(_q_quantile, {"df": df})
    exp = df.groupby("g").agg(
        p=("x", lambda s: s.quantile(0.3, interpolation="midpoint")),
        s=("i", "sum"))
    np.testing.assert_array_equal(got["p"].to_numpy(), exp["p"].to_numpy())
    np.testing.assert_array_equal(got["s"].to_numpy(), exp["s"].to_numpy())
