"""The argument checks that radix_argsort, radix_select and seg_select share
(csrc/radix.h), through the extension's entry points directly.

Every case is rejected before anything is launched, so no kernel runs; the
message is matched with the entry point's name in front.
"""

import pytest
import torch

from bodo_amd.ops import gpu

pytestmark = pytest.mark.gpu
_DEV = "cuda"
MAX_BLOCKS = 2048  # RS_MAX_BLOCKS of csrc/radix.h
N = 8


def _call(who, keys, max_blocks=MAX_BLOCKS, begin=0, end=-1):
    """The entry point `who` on `keys`, every other argument valid."""
    K = gpu.kernels()
    if who == "radix_argsort":
        return K.radix_argsort(keys, begin, end, None, max_blocks)
    if who == "radix_select":
        return K.radix_select(keys, 3, begin, end, False, -1, max_blocks)
    seg_start = torch.tensor([0, N], device=_DEV)
    rank = torch.tensor([3], device=_DEV)
    return K.seg_select(keys, seg_start, rank, max_blocks)


def _keys(dtype=torch.int32, n=N):
    return torch.arange(n, device=_DEV).to(dtype)


WHO = ["radix_argsort", "radix_select", "seg_select"]


@pytest.mark.parametrize("who", WHO)
def test_key_dtype(who):
    with pytest.raises(RuntimeError, match=f"{who}: unsupported key dtype"):
        _call(who, _keys(torch.float16))


@pytest.mark.parametrize("shape", ["2d", "strided"])
@pytest.mark.parametrize("who", WHO)
def test_key_layout(who, shape):
    keys = _keys().reshape(2, 4) if shape == "2d" else _keys(n=2 * N)[::2]
    with pytest.raises(RuntimeError, match=f"{who}: keys must be a contiguous "
                                           "1-d device tensor"):
        _call(who, keys)


@pytest.mark.parametrize("max_blocks", [0, MAX_BLOCKS + 1])
@pytest.mark.parametrize("who", WHO)
def test_max_blocks(who, max_blocks):
    with pytest.raises(RuntimeError, match=rf"{who}: max_blocks must be in "
                                           rf"\[1, {MAX_BLOCKS}\]"):
        _call(who, _keys(), max_blocks=max_blocks)


@pytest.mark.parametrize("bits", [(8, 8), (9, 8), (-1, 8), (0, 65)])
@pytest.mark.parametrize("who", ["radix_argsort", "radix_select"])
def test_bit_range(who, bits):
    with pytest.raises(RuntimeError, match=rf"{who}: bad bit range \[{bits[0]}, "
                                           rf"{bits[1]}\)"):
        _call(who, _keys(torch.int64), begin=bits[0], end=bits[1])


def test_perm_dtype():
    perm = torch.arange(N, device=_DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="radix_argsort: perm must be a "
                                           "contiguous int64 tensor"):
        gpu.kernels().radix_argsort(_keys(), 0, -1, perm, MAX_BLOCKS)


@pytest.mark.parametrize("nstart", [1, 3])
def test_seg_start_length(nstart):
    seg_start = torch.zeros(nstart, device=_DEV, dtype=torch.int64)
    rank = torch.zeros(1, device=_DEV, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="seg_select: seg_start must have "
                                           "one entry more than rank"):
        gpu.kernels().seg_select(_keys(), seg_start, rank, MAX_BLOCKS)


@pytest.mark.parametrize("k", [0, N])
def test_select_k(k):
    with pytest.raises(RuntimeError, match=r"radix_select: k must be in "
                                           r"\[1, n\)"):
        gpu.kernels().radix_select(_keys(), k, 0, -1, False, -1, MAX_BLOCKS)
