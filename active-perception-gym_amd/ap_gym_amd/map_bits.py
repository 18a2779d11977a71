"""Packed-bit floor maps: the layout `map_obs="bits"` hands out, and their expansion to dense maps on the device.

A packed map is its occupancy rows, 64-bit words [H, wpr] with wpr = ceil(W / 64): bit `x & 63` of word `x >> 6` of
row `y` is cell `(y, x)`, 1 = wall -- `np.unpackbits(rows.view(np.uint8), bitorder="little")` per row.  The padding bits
at `x >= W` are unspecified: consumers ignore them.  A batch is an int64 tensor [n, H, wpr] (uint64 in numpy), 32x
smaller than the float32 [n, H, W, 1] map observation.

`unpack_map_bits` (the HIP kernel k_unpack_maps, csrc/apg_unpack.hip) expands a chosen subset of a batch to dense
maps of the network's dtype: the replay-buffer pattern stores the bits and unpacks only the minibatch.
"""

from __future__ import annotations

import numpy as np

from . import _native as N

WALL_F32 = float(np.float32(1) / np.float32(255))  # the dense observation's wall value (lidar_localization2d.py:299)
MAX_MAP_SIDE = 511


def words_per_row(width: int) -> int:
    return (int(width) + 63) // 64


def host_words_np(t) -> np.ndarray:
    """A host int64 tensor of packed maps as a numpy uint64 array over the same memory.  The reinterpretation is done
    on the tensor, not with ndarray.view: numpy collapses chains of views, so slices of `t.numpy().view(np.uint64)`
    would have the hidden int64 array as their base and hold no reference to the array handed out."""
    import torch

    return t.view(torch.uint64).numpy()


def unpack_dtypes() -> dict:
    import torch

    return {torch.float32: N.APG_UNPACK_F32, torch.float16: N.APG_UNPACK_F16, torch.bfloat16: N.APG_UNPACK_BF16,
            torch.uint8: N.APG_UNPACK_U8}


def default_wall(dtype) -> float:
    """`wall` of unpack_map_bits when none is given: 1/255 in float32 (with dtype float32 the result is exactly the
    dense map observation), 1 for uint8."""
    import torch

    return 1.0 if dtype == torch.uint8 else WALL_F32


def unpack_map_bits(bits, width: int, env_ids=None, *, dtype=None, wall: float | None = None, out=None, err=None):
    """Dense maps [M, H, W, 1] of `dtype` from packed maps `bits` (a contiguous int64 [n_src, H, ceil(W / 64)] tensor on
    a GPU device, e.g. bit rows taken out of a replay buffer): output map m is map `env_ids[m]` of `bits` (a 1-d int64
    tensor on the same device, any order, duplicates allowed; None: every map in order), its cells `wall` where the
    bit is set and 0 elsewhere.

    dtype   torch.float32 (default), float16, bfloat16 or uint8 (`out`'s dtype when `out` is given)
    wall    converted once to `dtype`, round-to-nearest-even; default 1/255 (float32's, so float32 output equals the
            dense map observation) and 1 for uint8, where it must be an integer in 0..255
    out     a contiguous [M, H, W, 1] (or [M, H, W]) tensor of `dtype` on the same device to write into, at any
            element offset of its storage
    err     an int32 [1] device tensor: an id outside [0, n_src) yields an all-zero map (it is never read) and sets
            APG_ERR_INDEX in it (the env method raises that as IndexError at check_errors())

    Runs on the current stream without synchronising the host."""
    import torch

    dtypes = unpack_dtypes()
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int64 or bits.dim() != 3:
        raise TypeError("bits must be an int64 tensor [n_src, H, ceil(width / 64)]")
    width = int(width)
    if not 1 <= width <= MAX_MAP_SIDE or not 1 <= bits.shape[1] <= MAX_MAP_SIDE:
        raise ValueError(f"map height and width must be in 1..{MAX_MAP_SIDE}")
    if bits.shape[2] != words_per_row(width):
        raise ValueError(f"bits has {bits.shape[2]} words per row, width {width} needs {words_per_row(width)}")
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch tensor")
        if dtype is not None and out.dtype != dtype:
            raise TypeError(f"out is {out.dtype}, dtype {dtype} was asked for")
        dtype = out.dtype
    elif dtype is None:
        dtype = torch.float32
    if dtype not in dtypes:
        raise TypeError(f"dtype must be one of {', '.join(str(d) for d in dtypes)}, got {dtype}")
    if wall is None:
        wall = default_wall(dtype)
    wall = float(wall)
    if dtype == torch.uint8 and not (0 <= wall <= 255 and wall == int(wall)):
        raise ValueError("the wall value of uint8 maps must be an integer in 0..255")
    count = bits.shape[0]
    if env_ids is not None:
        if not isinstance(env_ids, torch.Tensor) or env_ids.dtype != torch.int64 or env_ids.dim() != 1:
            raise TypeError("env_ids must be a 1-d int64 tensor (or None)")
        count = env_ids.shape[0]
    shape = (count, bits.shape[1], width, 1)
    if out is not None and tuple(out.shape) not in (shape, shape[:3]):
        raise ValueError(f"out must have shape {shape}, got {tuple(out.shape)}")
    # (the device comes last: everything above is checked on tensors of any device)
    if bits.device.type != "cuda":
        raise ValueError(f"bits must be on a GPU device, got {bits.device} (there is no CPU fallback)")
    if not bits.is_contiguous():
        raise ValueError("bits must be contiguous")
    if env_ids is not None and (env_ids.device != bits.device or not env_ids.is_contiguous()):
        raise ValueError(f"env_ids must be contiguous and on {bits.device}")
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=bits.device)
    elif out.device != bits.device or not out.is_contiguous():
        raise ValueError(f"out must be contiguous and on {bits.device}")
    N.torch_ops().unpack_map_bits(bits, width, env_ids, out, wall, err)
    return out
