"""Exact LIDAR scans and fused scores at caller-chosen poses, on packed maps (the HIP kernel k_scan_poses,
csrc/apg_scan_poses.hip).

What would the LIDAR read from pose (x, y) on this map?  `lidar_scan_poses` answers with the env's own scan -- the
reference's `__lidar_scan` (shapely intersection with the union of unit boxes, the branch on the GEOS result type, the
1e-3 offset), bit for bit the value of obs["lidar"] at that pose -- for K poses per map at once.  `lidar_pose_scores`
fuses the comparison a particle filter or a pose-belief model makes: the squared error between each pose's scan and an
observed scan, one float per pose instead of B.

Maps are packed bit rows (map_bits.py: int64 [n_src, H, ceil(W / 64)], the layout of map_obs="bits"; the padding bits
at x >= W are ignored).  Poses are (x, y) in cells, the convention of the env's position.  Limits: map sides 1..511,
0 < lidar_range <= 60, beams 1..4096.  Pose domain: a pose with a non-finite coordinate is never scanned (NaN values
and score, APG_ERR_BAD_POSE in `err`); a finite pose further than 64 cells outside the map reaches no map cell, so
every beam reads the full beam length |q - p|, which is not an error.
"""

from __future__ import annotations

import numpy as np

from . import _native as N
from .map_bits import MAX_MAP_SIDE, words_per_row

MAX_BEAMS = 4096
MAX_LIDAR_RANGE = 60.0

_beam_dirs = {}


def beam_directions_on(beams: int, lidar_range: float, device):
    """The reference's beam directions (lidar_env.lidar_beam_directions) as a float32 [beams, 2] tensor on `device`,
    cached per (beams, range, device)."""
    import torch

    from .lidar_env import lidar_beam_directions

    key = (int(beams), float(lidar_range), str(device))
    t = _beam_dirs.get(key)
    if t is None:
        t = _beam_dirs[key] = torch.as_tensor(lidar_beam_directions(int(beams), lidar_range), device=device)
    return t


def _check_common(bits, width, poses, map_ids, beams, lidar_range):
    """The checks both entry points share, on tensors of any device; returns (width, beams, M, K)."""
    import torch

    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int64 or bits.dim() != 3:
        raise TypeError("bits must be an int64 tensor [n_src, H, ceil(width / 64)]")
    if not isinstance(poses, torch.Tensor) or poses.dtype != torch.float32:
        raise TypeError("poses must be a float32 tensor [M, K, 2]")
    if poses.dim() != 3 or poses.shape[2] != 2:
        raise ValueError(f"poses must have shape [M, K, 2], got {tuple(poses.shape)}")
    width = int(width)
    if not 1 <= width <= MAX_MAP_SIDE or not 1 <= bits.shape[1] <= MAX_MAP_SIDE:
        raise ValueError(f"map height and width must be in 1..{MAX_MAP_SIDE}")
    if bits.shape[2] != words_per_row(width):
        raise ValueError(f"bits has {bits.shape[2]} words per row, width {width} needs {words_per_row(width)}")
    beams = int(beams)
    if not 1 <= beams <= MAX_BEAMS:
        raise ValueError(f"beams must be in 1..{MAX_BEAMS}, got {beams}")
    if not 0 < float(np.float32(lidar_range)) <= MAX_LIDAR_RANGE:
        raise ValueError(f"lidar_range must be in (0, {MAX_LIDAR_RANGE:g}] (64-column scan windows), got {lidar_range}")
    m, k = poses.shape[0], poses.shape[1]
    if map_ids is not None:
        if not isinstance(map_ids, torch.Tensor) or map_ids.dtype != torch.int64 or map_ids.dim() != 1:
            raise TypeError("map_ids must be a 1-d int64 tensor (or None)")
        if map_ids.shape[0] != m:
            raise ValueError(f"map_ids must have one id per pose set ({m}), got {map_ids.shape[0]}")
    elif bits.shape[0] != 1 and bits.shape[0] != m:
        raise ValueError(f"without map_ids, bits must hold one map or one per pose set ({m}), got {bits.shape[0]}")
    return width, beams, m, k


def _check_out(out, shape, name="out"):
    import torch

    if out is None:
        return
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor")
    if tuple(out.shape) != shape:
        raise ValueError(f"{name} must have shape {shape}, got {tuple(out.shape)}")


def _check_device(bits, poses, map_ids, err, **others):
    """The device and contiguity checks, last: everything else was checked on tensors of any device."""
    import torch

    if bits.device.type != "cuda":
        raise ValueError(f"bits must be on a GPU device, got {bits.device} (there is no CPU fallback)")
    if not bits.is_contiguous():
        raise ValueError("bits must be contiguous")
    for name, t in dict(poses=poses, map_ids=map_ids, **others).items():
        if t is not None and (t.device != bits.device or not t.is_contiguous()):
            raise ValueError(f"{name} must be contiguous and on {bits.device}")
    if err is not None and (not isinstance(err, torch.Tensor) or err.dtype != torch.int32 or err.numel() != 1
                            or err.device != bits.device):
        raise ValueError(f"err must be an int32 [1] tensor on {bits.device}")


def _directions(beam_dirs, beams, lidar_range, device):
    """The cached reference directions, or the caller's own tensor (the env methods pass the env's)."""
    import torch

    if beam_dirs is None:
        return beam_directions_on(beams, lidar_range, device)
    if (not isinstance(beam_dirs, torch.Tensor) or beam_dirs.dtype != torch.float32
            or tuple(beam_dirs.shape) != (beams, 2) or beam_dirs.device != device or not beam_dirs.is_contiguous()):
        raise ValueError(f"beam_dirs must be a contiguous float32 [{beams}, 2] tensor on {device}")
    return beam_dirs


def lidar_scan_poses(bits, width: int, poses, map_ids=None, *, beams: int, lidar_range: float, normalize: bool = True,
                     out=None, err=None, beam_dirs=None):
    """Scans [M, K, beams] (float32) of the poses `poses` (float32 [M, K, 2], (x, y) in cells) on the packed maps
    `bits` (contiguous int64 [n_src, H, ceil(width / 64)] on a GPU device): pose set m is scanned on map `map_ids[m]`
    (a 1-d int64 tensor, any order, duplicates allowed; None: map m, or the one map when n_src == 1), along the
    reference's `beams` directions of length `lidar_range`.

    normalize  True: the observation's value, clip(d / lidar_range, -1, 1) -- equal to obs["lidar"] bit for bit at the
               env's position; False: the distance d in cells
    out        a contiguous float32 [M, K, beams] tensor on the same device to write into, at any element offset of its
               storage
    err        an int32 [1] device tensor: a map id outside [0, n_src) scans an all-zero map (it is never read) and
               sets APG_ERR_INDEX; a non-finite pose yields NaN and sets APG_ERR_BAD_POSE
    beam_dirs  None: the reference's directions for (beams, lidar_range), cached per device; or a float32 [beams, 2]
               device tensor that holds them already (the env methods pass the env's own)

    Runs on the current stream without synchronising the host."""
    import torch

    width, beams, m, k = _check_common(bits, width, poses, map_ids, beams, lidar_range)
    shape = (m, k, beams)
    _check_out(out, shape)
    _check_device(bits, poses, map_ids, err, out=out)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=bits.device)
    dirs = _directions(beam_dirs, beams, lidar_range, bits.device)
    N.torch_ops().lidar_scan_poses(bits, width, poses, map_ids, dirs, float(np.float32(lidar_range)), bool(normalize),
                                   None, out, None, err)
    return out


def lidar_pose_scores(bits, width: int, poses, observed, map_ids=None, *, beams: int, lidar_range: float, out=None,
                      err=None, scan_out=None, beam_dirs=None):
    """Scores [M, K] (float32): the squared error between each pose's normalised scan (lidar_scan_poses with
    normalize=True) and `observed` (float32 [M, beams], e.g. obs["lidar"] rows), sum_b (s_b - o_b)^2 accumulated in
    float32 in beam order -- 0.0 exactly where the pose reproduces the observation, NaN where `observed` holds one.
    The scans themselves are not written to memory unless `scan_out` (a contiguous float32 [M, K, beams] tensor on the
    same device) is given: the same launch then stores the normalised scans there too, which costs one pass instead
    of the two that lidar_scan_poses followed by this call take.  Other arguments as lidar_scan_poses (`out`: float32
    [M, K])."""
    import torch

    width, beams, m, k = _check_common(bits, width, poses, map_ids, beams, lidar_range)
    if not isinstance(observed, torch.Tensor) or observed.dtype != torch.float32:
        raise TypeError("observed must be a float32 tensor [M, beams]")
    if tuple(observed.shape) != (m, beams):
        raise ValueError(f"observed must have shape {(m, beams)}, got {tuple(observed.shape)}")
    shape = (m, k)
    _check_out(out, shape)
    _check_out(scan_out, (m, k, beams), "scan_out")
    _check_device(bits, poses, map_ids, err, observed=observed, out=out, scan_out=scan_out)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=bits.device)
    dirs = _directions(beam_dirs, beams, lidar_range, bits.device)
    N.torch_ops().lidar_scan_poses(bits, width, poses, map_ids, dirs, float(np.float32(lidar_range)), True, observed,
                                   scan_out, out, err)
    return out
