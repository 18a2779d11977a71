"""The scan spread of a particle belief per candidate action (the HIP kernel k_scan_spread,
csrc/apg_scan_spread.hip): how much would the belief's hypotheses disagree about what they see after this action?

For each pose set m and candidate a, the spread is the weighted variance of the hypotheses' normalised scans, summed
over the beams.  With normalised weights it is half the expected `lidar_pose_scores` value between two hypotheses drawn
from the belief, sum_jk w_j w_k |z_j - z_k|^2 = 2 sum_b Var_w(z_b): it is in the units of the score the particle
filter already uses, and an active localiser takes the candidate with the largest one, because that action tells the
hypotheses apart.  One launch scans and reduces; no scan is written to memory.  The result is reproducible by
construction: readings become integers (multiples of 2^-12) and weights the integers of `lidar_pf_resample` (multiples
of 2^-24) before anything is added, and every sum is exact integer arithmetic.  The definition, step by step, is the
comment of `apg_lidar_scan_spread` in include/apgym_capi.h.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _native as N
from .scan_poses import _check_common, _check_device, _check_out, _directions

MAX_HYPOTHESES = N.SCAN_SPREAD_MAX_K
MAX_SPREAD_BEAMS = N.SCAN_SPREAD_MAX_BEAMS


class ScanSpreadResult(NamedTuple):
    """spread float32 [M, A]; mean float32 [M, A, beams], the belief's expected normalised scan, or None."""

    spread: object
    mean: object


def lidar_scan_spread(bits, width: int, poses, weight=None, map_ids=None, *, beams: int, lidar_range: float,
                      mean: bool = False, out=None, err=None, beam_dirs=None):
    """Spread [M, A] (float32) of the hypotheses `poses` (float32 [M, A, K, 2], (x, y) in cells: hypothesis k of set m
    after candidate a; 1 <= K <= 4096) on the packed maps `bits` (contiguous int64 [n_src, H, ceil(width / 64)] on a GPU
    device), scanned as lidar_scan_poses scans them with normalize=True (1 <= beams <= 1024).

    weight     float32 [M, K] in [0, 1], the weight of hypothesis k of set m under every candidate (lidar_pf_resample's
               `weight`, or exp(logw)); None: all 1.  They need not sum to 1
    map_ids    a 1-d int64 tensor [M] (any order, duplicates allowed); None: map m, or the one map when n_src == 1
    mean       True: also return the belief's expected scan [M, A, beams]
    out        a contiguous float32 [M, A] tensor on the same device to write the spread into
    err        an int32 [1] device tensor: a hypothesis with a non-finite coordinate drops out of its own (m, a) only, a
               weight that is NaN or outside [0, 1] counts as 0, and both set APG_ERR_BAD_POSE; a map id outside
               [0, n_src) scans an all-zero map and sets APG_ERR_INDEX
    beam_dirs  as lidar_scan_poses

    Returns a ScanSpreadResult.  The spread is exactly 0 where every hypothesis of positive weight reads the same scan
    (to 2^-12 of the range), and NaN where no hypothesis has positive weight.

    Runs on the current stream without synchronising the host."""
    import torch

    if not isinstance(poses, torch.Tensor) or poses.dtype != torch.float32:
        raise TypeError("poses must be a float32 tensor [M, A, K, 2]")
    if poses.dim() != 4 or poses.shape[3] != 2:
        raise ValueError(f"poses must have shape [M, A, K, 2], got {tuple(poses.shape)}")
    m, a, k = poses.shape[0], poses.shape[1], poses.shape[2]
    if a < 1:
        raise ValueError(f"poses: A must be >= 1, got {a}")
    if not 1 <= k <= MAX_HYPOTHESES:
        raise ValueError(f"poses: K must be in 1..{MAX_HYPOTHESES}, got {k}")
    width, beams, _, _ = _check_common(bits, width, poses.reshape(m, a * k, 2), map_ids, beams, lidar_range)
    if beams > MAX_SPREAD_BEAMS:
        raise ValueError(f"beams must be in 1..{MAX_SPREAD_BEAMS}, got {beams}")
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32:
            raise TypeError("weight must be a float32 tensor [M, K]")
        if tuple(weight.shape) != (m, k):
            raise ValueError(f"weight must have shape {(m, k)}, got {tuple(weight.shape)}")
    _check_out(out, (m, a))
    _check_device(bits, poses, map_ids, err, weight=weight, out=out)
    f32 = dict(dtype=torch.float32, device=bits.device)
    if out is None:
        out = torch.empty((m, a), **f32)
    mean_out = torch.empty((m, a, beams), **f32) if mean else None
    dirs = _directions(beam_dirs, beams, lidar_range, bits.device)
    N.torch_ops().lidar_scan_spread(bits, width, poses, weight, map_ids, dirs, float(np.float32(lidar_range)), out,
                                    mean_out, err)
    return ScanSpreadResult(out, mean_out)
