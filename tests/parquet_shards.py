"""The shard of the in-place parquet decode tests, GPU and CPU: two files of
three row groups (4999, 5000, 5001 rows), so the second row group's 4-byte
columns start at an address that is 4- but not 8-byte aligned and a group of
row groups crosses a file boundary, and 4 KiB pages whose values start at
odd offsets behind the definition-level prefix."""

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

RG_ROWS = (4999, 5000, 5001)
N_FILES = 2
WORDS = ["alpha", "beta", "gamma", "delta"]
# columns decoded in place / columns that keep the per-chunk finish
DIRECT_COLS = ["loc", "f", "i32", "f32", "ts", "req", "s_dict", "cat"]
OTHER_COLS = ["nul", "s_plain", "nostat"]
SCHEMA = pa.schema([
    pa.field("loc", pa.int64()),
    pa.field("f", pa.float64()),
    pa.field("i32", pa.int32()),
    pa.field("f32", pa.float32()),
    pa.field("ts", pa.timestamp("us")),
    pa.field("req", pa.int64(), nullable=False),
    pa.field("s_dict", pa.string()),
    pa.field("nul", pa.int64()),
    pa.field("s_plain", pa.string()),
    pa.field("nostat", pa.int64()),
    # a dictionary array, as a table written from dictionary columns has it
    pa.field("cat", pa.dictionary(pa.int32(), pa.large_string())),
])


def _row_group(rng, n, k):
    # every row group meets the words in another first order; the fourth
    # one never sees "delta"
    words = WORDS[k % 4:] + WORDS[:k % 4]
    if k == 3:
        words = [w for w in words if w != "delta"]
    s_dict = np.concatenate([words, rng.choice(words, n - len(words))])
    return pa.table({
        "loc": rng.integers(1, 266, n).astype("int64"),
        "f": rng.random(n),
        "i32": rng.integers(-10**6, 10**6, n).astype("int32"),
        "f32": rng.random(n).astype("float32"),
        "ts": pa.array(rng.integers(0, 2 * 10**15, n),
                       type=pa.timestamp("us")),
        "req": rng.integers(-10**12, 10**12, n).astype("int64"),
        "s_dict": pa.array(s_dict.tolist(), type=pa.string()),
        "nul": pa.array(rng.integers(-10**12, 10**12, n), type=pa.int64(),
                        mask=rng.random(n) < 0.10),
        "s_plain": pa.array(["s" + str(v)
                             for v in rng.integers(0, 10**9, n)]),
        "nostat": rng.integers(0, 1000, n).astype("int64"),
        "cat": pa.DictionaryArray.from_arrays(
            pa.array(rng.integers(0, 3, n).astype(np.int32)),
            pa.array(["HV3", "HV4", "HV5"], type=pa.large_string())),
    }, schema=SCHEMA)


def write_shard(d, compressions=("SNAPPY",) * N_FILES):
    """Write the shard's files into directory d, one per entry of
    compressions; returns (directory path, the shard as pyarrow reads it)."""
    rng = np.random.default_rng(99)
    k = 0
    paths = []
    for i, compression in enumerate(compressions):
        path = str(d / f"part-{i:05d}.parquet")
        paths.append(path)
        with pq.ParquetWriter(
                path, SCHEMA, compression=compression,
                use_dictionary=["s_dict", "cat"], data_page_size=4096,
                write_statistics=[c for c in SCHEMA.names
                                  if c != "nostat"]) as w:
            for n in RG_ROWS:
                w.write_table(_row_group(rng, n, k), row_group_size=n)
                k += 1
        md = pq.ParquetFile(path).metadata
        assert [md.row_group(r).num_rows
                for r in range(md.num_row_groups)] == list(RG_ROWS)
    ref = pa.concat_tables([pq.read_table(p) for p in paths])
    return str(d), ref
