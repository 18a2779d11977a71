"""Glimpses, fused match scores and moves of the image envs at caller-chosen positions (the HIP kernels
k_glimpse_scores and k_image_move, csrc/apg_glimpse_poses.hip).

What would the sensor see at position (x, y) of this image?  `image_glimpses_at` answers with the env's own glimpse --
the reference's scipy RegularGridInterpolator "linear" in float64, clip(0, 1), float32, operation for operation the
code the env's step runs: at a sub-env's float64 position it equals obs["glimpse"], at its float32 target
obs["target_glimpse"], bit for bit -- for K positions per image at once.  `image_glimpse_scores` fuses the comparison
a template search or a belief model makes: np.mean((glimpse - observed) ** 2, axis=(-3, -2, -1)) in float32 exactly
as numpy evaluates it (the reference's uniqueness expression), one float per position instead of a glimpse.
`image_move_positions` applies the env's move (project_sphere, max_step_length, clip) to candidate action sequences.

Pools are what the envs hold on the device: uint8 [pool_len, H, W, 1 or 3] with N.APG_U8_POOL_PAD readable bytes
behind the last image (image_env.device_pool_u8 / padded_device_pool_u8), the flat uint8 RGBX tile layout of
image_env.device_pool_u8_tiled (`tiled=True`), or float32 [pool_len, H, W, 1 or 3].  Positions are normalised (x, y)
as obs["glimpse_pos"], float64 or float32.  Limits: sensor sides 1..256, at most 16384 values per glimpse, fewer than
2**31 pixels per call; the fused score takes glimpses of at most GLIMPSE_SCORES_MAX_L = 4096 values (32 x 32 x 3 fits),
because a workgroup keeps its glimpses and the observed block in LDS.  Domain: a position whose sampling coordinates
leave the image (the reference raises there) or that is not finite yields NaN and sets APG_ERR_OOB_X / APG_ERR_OOB_Y in
`err`; an index outside [0, pool_len) is never read, yields NaN and sets APG_ERR_INDEX.  Other positions are unaffected.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _native as N

GLIMPSE_SCORES_MAX_L = N.GLIMPSE_SCORES_MAX_L
MAX_SENSOR_SIDE = N.GLIMPSE_MAX_SIDE
MAX_GLIMPSE_L = N.GLIMPSE_MAX_L
MAX_T = N.IMAGE_MOVE_MAX_T


class ImageMoveResult(NamedTuple):
    pos: object          # float64 [M, K, T, 2] the position after each action
    glimpse_pos: object  # float32 [M, K, T, 2] obs["glimpse_pos"] after each action
    base_reward: object  # float32 [M, K, T]


def _tiled_image_bytes(h: int, w: int) -> int:
    return ((h + 3) // 4) * ((w + 7) // 8) * 128


def _check_common(pool, index, positions, image_size, sensor_size, sensor_scale, channels, tiled):
    """The checks every entry point shares, on tensors of any device; returns (geo, sensor_scale, M, K, glimpse
    shape (s0, s1, C))."""
    import torch

    if not isinstance(pool, torch.Tensor) or pool.dtype not in (torch.uint8, torch.float32):
        raise TypeError("pool must be a uint8 or float32 tensor")
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1:
        raise TypeError("index must be a 1-d int64 tensor [M]")
    if not isinstance(positions, torch.Tensor) or positions.dtype not in (torch.float64, torch.float32):
        raise TypeError("positions must be a float64 or float32 tensor [M, K, 2]")
    if positions.dim() != 3 or positions.shape[2] != 2:
        raise ValueError(f"positions must have shape [M, K, 2], got {tuple(positions.shape)}")
    m, k = positions.shape[0], positions.shape[1]
    if index.shape[0] != m:
        raise ValueError(f"index must have one pool image per position set ({m}), got {index.shape[0]}")
    h, w = (int(v) for v in image_size)
    if h < 2 or w < 2:
        raise ValueError("images must be at least 2 x 2")
    channels = int(channels)
    if channels not in (1, 3):
        raise ValueError(f"Target channels must be either 1 or 3 but is {channels}.")
    if tiled:
        if pool.dtype != torch.uint8 or pool.dim() != 1:
            raise ValueError("a tiled pool is the flat uint8 tensor of image_env.device_pool_u8_tiled")
        img = _tiled_image_bytes(h, w)
        if pool.numel() == 0 or pool.numel() % img:
            raise ValueError(f"a tiled pool of {h} x {w} images holds a multiple of {img} bytes, got {pool.numel()}")
        pc, pool_len, dtype = 3, pool.numel() // img, N.APG_POOL_U8_TILED
    else:
        if pool.dim() != 4 or tuple(pool.shape[1:3]) != (h, w) or pool.shape[3] not in (1, 3) or pool.shape[0] < 1:
            raise ValueError(f"pool must have shape [pool_len, {h}, {w}, 1 or 3], got {tuple(pool.shape)}")
        pc, pool_len = int(pool.shape[3]), int(pool.shape[0])
        dtype = N.APG_POOL_U8 if pool.dtype == torch.uint8 else N.APG_POOL_F32
    if pc != channels and not (pc == 1 and channels == 3):
        raise ValueError(f"Invalid image format. Expected {channels} channels but got {pc}")
    s0, s1 = (int(v) for v in sensor_size)
    if not (1 <= s0 <= MAX_SENSOR_SIDE and 1 <= s1 <= MAX_SENSOR_SIDE):
        raise ValueError(f"sensor sides must be in 1..{MAX_SENSOR_SIDE}, got {(s0, s1)}")
    if s0 * s1 * channels > MAX_GLIMPSE_L:
        raise ValueError(f"a glimpse holds at most {MAX_GLIMPSE_L} values, got {s0 * s1 * channels}")
    if m * k * s0 * s1 >= 2**31:
        raise ValueError(f"too many pixels in one call ({m * k * s0 * s1} >= 2**31): split the position sets")
    scale = float(sensor_scale)
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"sensor_scale must be positive and finite, got {sensor_scale}")
    return [h, w, pc, channels, dtype, s0, s1, pool_len], scale, m, k, (s0, s1, channels)


def _check_out(out, shape, name="out"):
    import torch

    if out is None:
        return
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor")
    if tuple(out.shape) != shape:
        raise ValueError(f"{name} must have shape {shape}, got {tuple(out.shape)}")


def _check_err(err, device):
    import torch

    if err is not None and (not isinstance(err, torch.Tensor) or err.dtype != torch.int32 or err.numel() != 1
                            or err.device != device):
        raise ValueError(f"err must be an int32 [1] tensor on {device}")


def _check_device(pool, err, **others):
    """The device and contiguity checks, last: everything else was checked on tensors of any device."""
    import torch

    if pool.device.type != "cuda":
        raise ValueError(f"pool must be on a GPU device, got {pool.device} (there is no CPU fallback)")
    if not pool.is_contiguous():
        raise ValueError("pool must be contiguous")
    if pool.dtype == torch.uint8 and (pool.untyped_storage().nbytes() - pool.storage_offset()
                                      < pool.numel() + N.APG_U8_POOL_PAD):
        raise ValueError(f"a uint8 pool needs {N.APG_U8_POOL_PAD} readable bytes behind its last image in its own "
                         "allocation (image_env.padded_device_pool_u8 makes such a pool)")
    for name, t in others.items():
        if t is not None and (t.device != pool.device or not t.is_contiguous()):
            raise ValueError(f"{name} must be contiguous and on {pool.device}")
    _check_err(err, pool.device)


def image_glimpses_at(pool, index, positions, *, image_size, sensor_size, sensor_scale: float = 1.0, channels: int,
                      tiled: bool = False, out=None, err=None):
    """Glimpses [M, K, s0, s1, C] (float32) at `positions` (float64 or float32 [M, K, 2], normalised (x, y)): position
    set m is taken on pool image `index[m]` (a 1-d int64 tensor, any order, duplicates allowed).

    image_size    (H, W) of the pool's images
    sensor_size   (s0, s1), sensor_scale: as ImagePerceptionConfig
    channels      the observation's channels C (1 or 3; a grey pool with C = 3 repeats its channel)
    tiled         the pool is image_env.device_pool_u8_tiled's flat RGBX tile layout
    out           a contiguous float32 [M, K, s0, s1, C] tensor on the pool's device to write into
    err           an int32 [1] device tensor for the APG_ERR_* bits (see the module text)

    Runs on the current stream without synchronising the host."""
    import torch

    geo, scale, m, k, g = _check_common(pool, index, positions, image_size, sensor_size, sensor_scale, channels, tiled)
    shape = (m, k, *g)
    _check_out(out, shape)
    _check_device(pool, err, index=index, positions=positions, out=out)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pool.device)
    N.torch_ops().image_glimpse_scores(pool, geo, scale, index, positions, None, None, out, err)
    return out


def image_glimpse_scores(pool, index, positions, observed, *, image_size, sensor_size, sensor_scale: float = 1.0,
                         channels: int, tiled: bool = False, out=None, glimpse_out=None, err=None):
    """Scores [M, K] (float32): np.mean((g - observed[m]) ** 2, axis=(-3, -2, -1)) between the glimpse g at each of
    `positions` and `observed` (float32 [M, s0, s1, C], e.g. obs["target_glimpse"] rows), in float32 as numpy
    evaluates it on a contiguous block (difference and square rounded in element order, numpy's pairwise sum, then
    (0 + sum) / L) -- 0.0 exactly where the position reproduces the observation, NaN where `observed[m]` holds a NaN.
    The glimpses are not written to memory unless `glimpse_out` (a contiguous float32 [M, K, s0, s1, C] tensor on the
    same device) is given: the same launch then stores them there too.  Glimpses of more than GLIMPSE_SCORES_MAX_L
    values are refused (ValueError): take them with image_glimpses_at and score them outside.  Other arguments as
    image_glimpses_at (`out`: float32 [M, K])."""
    import torch

    geo, scale, m, k, g = _check_common(pool, index, positions, image_size, sensor_size, sensor_scale, channels, tiled)
    if g[0] * g[1] * g[2] > GLIMPSE_SCORES_MAX_L:
        raise ValueError(f"the fused score takes glimpses of at most {GLIMPSE_SCORES_MAX_L} values (sensor_size[0] * "
                         f"sensor_size[1] * channels), got {g[0] * g[1] * g[2]}: get the glimpses with "
                         "image_glimpses_at and score them outside")
    if not isinstance(observed, torch.Tensor) or observed.dtype != torch.float32:
        raise TypeError("observed must be a float32 tensor [M, s0, s1, C]")
    if tuple(observed.shape) != (m, *g):
        raise ValueError(f"observed must have shape {(m, *g)}, got {tuple(observed.shape)}")
    _check_out(out, (m, k))
    _check_out(glimpse_out, (m, k, *g), "glimpse_out")
    _check_device(pool, err, index=index, positions=positions, observed=observed, out=out, glimpse_out=glimpse_out)
    if out is None:
        out = torch.empty((m, k), dtype=torch.float32, device=pool.device)
    N.torch_ops().image_glimpse_scores(pool, geo, scale, index, positions, observed, out, glimpse_out, err)
    return out


def image_move_positions(pos, actions, *, max_step_length, max_steps=None, err=None):
    """Where would these actions take the sensor?  `pos` float64 [M, 2] start positions, `actions` float32
    [M, K, T, 2] (1 <= T <= 4096): K candidate sequences per start, each applied with the env's move
    (ImagePerceptionModule.step: project_sphere in float32, max_step_length in float64, clip to [-1, 1]) exactly as
    step() does.  Returns an ImageMoveResult: pos float64 [M, K, T, 2], glimpse_pos float32 [M, K, T, 2] (the
    observation's value) and base_reward float32 [M, K, T] = -|action| * 1e-3.

    max_step_length  a float or (x, y), as ImagePerceptionConfig
    max_steps        None: all T actions; an int >= 0: after that many actions the position repeats and the base
                     reward is 0 (an episode that ends there)
    err              an int32 [1] device tensor: a NaN action gives NaN from that action on and sets
                     APG_ERR_NAN_ACTION

    Runs on the current stream without synchronising the host."""
    import torch

    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.float64:
        raise TypeError("pos must be a float64 tensor [M, 2]")
    if not isinstance(actions, torch.Tensor) or actions.dtype != torch.float32:
        raise TypeError("actions must be a float32 tensor [M, K, T, 2]")
    if pos.dim() != 2 or pos.shape[1] != 2:
        raise ValueError(f"pos must have shape [M, 2], got {tuple(pos.shape)}")
    if actions.dim() != 4 or actions.shape[3] != 2 or actions.shape[0] != pos.shape[0]:
        raise ValueError(f"actions must have shape [{pos.shape[0]}, K, T, 2], got {tuple(actions.shape)}")
    m, k, t = actions.shape[0], actions.shape[1], actions.shape[2]
    if not 1 <= t <= MAX_T:
        raise ValueError(f"T must be in 1..{MAX_T}, got {t}")
    if m * k >= 2**31:
        raise ValueError(f"too many candidates in one call ({m * k} >= 2**31)")
    msl = np.asarray(max_step_length, dtype=np.float64)
    msl = np.ones(2) * msl if msl.shape in ((), (1,), (2,)) else msl
    if msl.shape != (2,) or not np.isfinite(msl).all():
        raise ValueError(f"max_step_length must be a finite float or pair, got {max_step_length!r}")
    if max_steps is None:
        max_steps = t
    if not isinstance(max_steps, (int, np.integer)) or isinstance(max_steps, bool) or max_steps < 0:
        raise ValueError(f"max_steps must be None or an int >= 0, got {max_steps!r}")
    if pos.device.type != "cuda":
        raise ValueError(f"pos must be on a GPU device, got {pos.device} (there is no CPU fallback)")
    for name, x in dict(pos=pos, actions=actions).items():
        if x.device != pos.device or not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous and on {pos.device}")
    _check_err(err, pos.device)
    out = ImageMoveResult(torch.empty((m, k, t, 2), dtype=torch.float64, device=pos.device),
                          torch.empty((m, k, t, 2), dtype=torch.float32, device=pos.device),
                          torch.empty((m, k, t), dtype=torch.float32, device=pos.device))
    N.torch_ops().image_move(pos, actions, float(msl[0]), float(msl[1]), int(min(int(max_steps), 2**31 - 1)), out.pos,
                             out.glimpse_pos, out.base_reward, err)
    return out
