"""Particle weights, the weighted-mean pose, the effective sample size and exact systematic resampling (the HIP kernel
k_pf_resample, csrc/apg_pf_resample.hip): the third stage of a particle filter, after the measurement update
(`lidar_pose_scores`) and the motion update (`lidar_move_poses`).

One launch turns log-weights and scores into normalised weights, the estimate, the ESS and -- for the sets whose ESS
fell below `ess_frac * K` -- the resampled particles.  The result is deterministic by construction: right after the
exponential the weights become integers in 0..2^24, and every sum, threshold and search after that is integer
arithmetic, so two runs (or two work splits) pick the same ancestors.  The definition, step by step, is the comment of
`apg_lidar_pf_resample` in include/apgym_capi.h.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _native as N

MAX_PARTICLES = N.PF_RESAMPLE_MAX_K


class PfResampleResult(NamedTuple):
    """weight float32 [M, K] (the maximum is 1); estimate float32 [M, 2]; ess float32 [M]; index int32 [M, K] (the
    ancestor of each output particle; j where the set was not resampled); poses float32 [M, K, 2] and logw float32
    [M, K], the particles to carry on with; resampled uint8 [M] (0 or 1: the kernel's own output, no extra launch)."""

    weight: object
    estimate: object
    ess: object
    index: object
    poses: object
    logw: object
    resampled: object


class PfUpdateResult(NamedTuple):
    """env.pf_update's result: the fields of PfResampleResult, then scores float32 [M, K] (pose_scores)."""

    weight: object
    estimate: object
    ess: object
    index: object
    poses: object
    logw: object
    resampled: object
    scores: object


def _check(poses, logw, scores, u, logw_out):
    """Everything that can be checked on tensors of any device; returns (M, K)."""
    import torch

    if not isinstance(poses, torch.Tensor) or poses.dtype != torch.float32:
        raise TypeError("poses must be a float32 tensor [M, K, 2]")
    if poses.dim() != 3 or poses.shape[2] != 2:
        raise ValueError(f"poses must have shape [M, K, 2], got {tuple(poses.shape)}")
    m, k = poses.shape[0], poses.shape[1]
    if not 1 <= k <= MAX_PARTICLES:
        raise ValueError(f"poses: K must be in 1..{MAX_PARTICLES}, got {k}")
    for name, x, shape in (("logw", logw, (m, k)), ("scores", scores, (m, k)), ("u", u, (m,)),
                           ("logw_out", logw_out, (m, k))):
        if x is None:
            continue
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor {list(shape)}")
        if tuple(x.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(x.shape)}")
    if logw_out is not None and poses.numel():
        a, b = logw_out.data_ptr(), poses.data_ptr()
        if a < b + 8 * m * k and b < a + 4 * m * k:
            raise ValueError("logw_out must not alias poses (it may be logw itself: in place)")
    return m, k


def lidar_pf_resample(poses, logw=None, scores=None, *, score_scale: float = 0.0, u=None, ess_frac: float = 0.5,
                      generator=None, err=None, logw_out=None):
    """Weights, estimate, ESS and systematic resampling of M particle sets of K particles (1 <= K <= 4096).

    poses        float32 [M, K, 2], contiguous, on a GPU device
    logw         float32 [M, K] log-weights carried over from the last call, or None (all 0)
    scores       float32 [M, K], e.g. lidar_pose_scores' squared errors, or None; the new log-weight is
                 logw - score_scale * scores in float32 (a Gaussian likelihood: score_scale = 1 / (2 sigma^2))
    u            float32 [M] in [0, 1), the one random number systematic resampling takes per set; None: drawn with
                 torch.rand on the device from `generator` (not drawn at all when ess_frac <= 0)
    ess_frac     a set is resampled when its ESS is below ess_frac * K: 0 never, 1 every set whose weights are not
                 uniform, above 1 always
    err          an int32 [1] device tensor: a particle with a NaN or +inf log-weight or a non-finite pose has weight
                 0, is never selected and sets APG_ERR_BAD_POSE (-inf is legal: a dead particle)
    logw_out     a float32 [M, K] tensor to write the new log-weights into; it may be `logw` itself

    Returns a PfResampleResult.  `weight`, `estimate` and `ess` describe the particles that went IN (weights normalised
    to a maximum of 1; a set without a live particle restarts with uniform weights); `poses` and `logw` are the
    particles to carry on with: the ancestors `poses[m, index[m, j]]` with log-weight 0 where `resampled[m]`, else the
    input poses with their max-normalised log-weights.

    Runs on the current stream without synchronising the host."""
    import torch

    m, k = _check(poses, logw, scores, u, logw_out)
    score_scale = float(np.float32(score_scale))
    ess_frac = float(np.float32(ess_frac))
    # the device and contiguity checks, last: everything else was checked on tensors of any device
    if poses.device.type != "cuda":
        raise ValueError(f"poses must be on a GPU device, got {poses.device} (there is no CPU fallback)")
    dev = poses.device
    for name, x in dict(poses=poses, logw=logw, scores=scores, u=u, logw_out=logw_out).items():
        if x is not None and (x.device != dev or not x.is_contiguous()):
            raise ValueError(f"{name} must be contiguous and on {dev}")
    if err is not None and (not isinstance(err, torch.Tensor) or err.dtype != torch.int32 or err.numel() != 1
                            or err.device != dev):
        raise ValueError(f"err must be an int32 [1] tensor on {dev}")
    if u is None and ess_frac > 0:
        u = torch.rand(m, dtype=torch.float32, device=dev, generator=generator)
    f32 = dict(dtype=torch.float32, device=dev)
    weight = torch.empty((m, k), **f32)
    estimate = torch.empty((m, 2), **f32)
    ess = torch.empty((m,), **f32)
    index = torch.empty((m, k), dtype=torch.int32, device=dev)
    poses_out = torch.empty((m, k, 2), **f32)
    if logw_out is None:
        logw_out = torch.empty((m, k), **f32)
    resampled = torch.empty((m,), dtype=torch.uint8, device=dev)
    N.torch_ops().lidar_pf_resample(poses, logw, scores, u, score_scale, ess_frac, weight, estimate, ess, index,
                                    poses_out, logw_out, resampled, err)
    return PfResampleResult(weight, estimate, ess, index, poses_out, logw_out, resampled)
