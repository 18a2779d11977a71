"""Target-position evidence from what a localization agent itself observes (the HIP kernel k_overlap_scores,
csrc/apg_overlap_scores.hip).

An agent in a *Loc-v0 env sees its glimpse g, the glimpse's position q and the target glimpse G it has to localise; it
never sees the image.  The only evidence these carry about the target position is what the two sensor windows agree on
where they overlap: under the hypothesis "the target is at h" the windows are shifted against each other by
d = (q - h) * sensor_pos_lim_pixels / sensor_scale sensor pixels, and inside the overlap g must equal G resampled
(bilinear, float32) at that shift.  `image_overlap_scores` returns, for K hypotheses per observation, the sum of the
squared differences over the overlap (`sse`), the number of values compared (`count`), and optionally the fused belief
update logw + gain * (tau * count - sse): an overlapping value that matches better than tau is evidence for the
hypothesis, one that matches worse is evidence against it, a hypothesis without overlap keeps its weight.  The
definition, operation for operation (it is matched bit for bit by a numpy restatement in the tests), is the comment of
`apg_image_overlap_scores` in include/apgym_capi.h.

No pool image is read: this is the measurement update an agent can compute; `glimpse_poses.image_glimpse_scores` is the
one a planner with access to the image computes.  Limits: a glimpse of at most OVERLAP_SCORES_MAX_L = 4096 values (both
glimpses of a set live in LDS).  Domain: a glimpse position or hypothesis with a non-finite coordinate yields sse = NaN,
count = 0 (and a NaN log-weight, which `lidar_pf_resample` treats as a dead particle) and sets APG_ERR_BAD_POSE in
`err`; other hypotheses are unaffected.
"""

from __future__ import annotations

from typing import NamedTuple

from . import _native as N

OVERLAP_SCORES_MAX_L = N.OVERLAP_SCORES_MAX_L


class OverlapScoresResult(NamedTuple):
    sse: object    # float32 [M, K] sum of squared differences over the overlap (+0.0 without overlap)
    count: object  # int32 [M, K] values compared: C * samples in the overlap
    logw: object   # float32 [M, K] the updated log-weights, or None when no logw was given


def _overlaps(a, b) -> bool:
    """True when the memory of the tensors a and b intersects (any device: data_ptr arithmetic only)."""
    if a is None or b is None or a.numel() == 0 or b.numel() == 0 or a.device != b.device:
        return False
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


def image_overlap_scores(glimpse, glimpse_pos, target_glimpse, hypotheses, *, image_size, sensor_size,
                         sensor_scale: float = 1.0, logw=None, gain: float = 0.0, tau: float = 0.0, logw_out=None,
                         err=None) -> OverlapScoresResult:
    """Overlap scores of K hypotheses of the target position for each of M observations.

    glimpse         float32 [M, s0, s1, C], obs["glimpse"]
    glimpse_pos     float32 or float64 [M, 2], obs["glimpse_pos"] (normalised (x, y))
    target_glimpse  float32 [M, s0, s1, C], obs["target_glimpse"]
    hypotheses      float32 or float64 [M, K, 2], or [K, 2] shared by every observation (normalised (x, y), the env's
                    prediction space)
    image_size      (H, W) of the env's images; sensor_size (s0, s1) and sensor_scale as ImagePerceptionConfig
    logw            float32 [M, K] log-weights to update, or None
    gain, tau       the update logw + gain * (tau * count - sse), each operation rounded to float32; a Gaussian
                    likelihood of standard deviation sigma per value has gain = 1 / (2 sigma^2)
    logw_out        a contiguous float32 [M, K] tensor for the updated log-weights (needs logw; it may be logw itself:
                    in place; any other overlap with an input is refused)
    err             an int32 [1] device tensor for the APG_ERR_* bits (see the module text)

    Returns an OverlapScoresResult(sse, count, logw).  Runs on the current stream without synchronising the host."""
    import torch

    for name, x in (("glimpse", glimpse), ("target_glimpse", target_glimpse)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor [M, s0, s1, C]")
    for name, x in (("glimpse_pos", glimpse_pos), ("hypotheses", hypotheses)):
        if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float64, torch.float32):
            raise TypeError(f"{name} must be a float64 or float32 tensor")
    s0, s1 = (int(v) for v in sensor_size)
    if s0 < 1 or s1 < 1:
        raise ValueError(f"sensor sides must be positive, got {(s0, s1)}")
    if glimpse.dim() != 4 or tuple(glimpse.shape[1:3]) != (s0, s1) or glimpse.shape[3] < 1:
        raise ValueError(f"glimpse must have shape [M, {s0}, {s1}, C], got {tuple(glimpse.shape)}")
    m, c = int(glimpse.shape[0]), int(glimpse.shape[3])
    if tuple(target_glimpse.shape) != tuple(glimpse.shape):
        raise ValueError(f"target_glimpse must have the glimpse's shape {tuple(glimpse.shape)}, got "
                         f"{tuple(target_glimpse.shape)}")
    if s0 * s1 * c > OVERLAP_SCORES_MAX_L:
        raise ValueError(f"a glimpse holds at most {OVERLAP_SCORES_MAX_L} values (sensor_size[0] * sensor_size[1] * "
                         f"channels), got {s0 * s1 * c}")
    if tuple(glimpse_pos.shape) != (m, 2):
        raise ValueError(f"glimpse_pos must have shape {(m, 2)}, got {tuple(glimpse_pos.shape)}")
    if not ((hypotheses.dim() == 3 and hypotheses.shape[0] == m and hypotheses.shape[2] == 2)
            or (hypotheses.dim() == 2 and hypotheses.shape[1] == 2)):
        raise ValueError(f"hypotheses must have shape [{m}, K, 2] or [K, 2], got {tuple(hypotheses.shape)}")
    k = int(hypotheses.shape[-2])
    h, w = (int(v) for v in image_size)
    if h < 2 or w < 2:
        raise ValueError("images must be at least 2 x 2")
    scale = float(sensor_scale)
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"sensor_scale must be positive and finite, got {sensor_scale}")
    chunk = N.overlap_scores_chunk(m, k)
    if chunk and m * ((k + chunk - 1) // chunk) >= 2**31:
        raise ValueError(f"too many hypotheses in one call ({m} sets of {k}): split the sets")
    gain, tau = float(gain), float(tau)
    if logw is None and logw_out is not None:
        raise ValueError("logw_out needs logw")
    for name, x in (("logw", logw), ("logw_out", logw_out)):
        if x is None:
            continue
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor [M, K]")
        if tuple(x.shape) != (m, k):
            raise ValueError(f"{name} must have shape {(m, k)}, got {tuple(x.shape)}")
    if logw_out is not None:
        same = (logw_out.data_ptr() == logw.data_ptr() and logw_out.device == logw.device
                and logw_out.stride() == logw.stride())
        if not same and _overlaps(logw_out, logw):
            raise ValueError("logw_out overlaps logw partially (it may be logw itself)")
        for name, x in (("glimpse", glimpse), ("target_glimpse", target_glimpse), ("glimpse_pos", glimpse_pos),
                        ("hypotheses", hypotheses)):
            if _overlaps(logw_out, x):
                raise ValueError(f"logw_out overlaps {name}")
    # the device and contiguity checks, last: everything above was checked on tensors of any device
    dev = glimpse.device
    if dev.type != "cuda":
        raise ValueError(f"glimpse must be on a GPU device, got {dev} (there is no CPU fallback)")
    for name, x in (("glimpse", glimpse), ("glimpse_pos", glimpse_pos), ("target_glimpse", target_glimpse),
                    ("hypotheses", hypotheses), ("logw", logw), ("logw_out", logw_out)):
        if x is not None and (x.device != dev or not x.is_contiguous()):
            raise ValueError(f"{name} must be contiguous and on {dev}")
    if err is not None and (not isinstance(err, torch.Tensor) or err.dtype != torch.int32 or err.numel() != 1
                            or err.device != dev):
        raise ValueError(f"err must be an int32 [1] tensor on {dev}")
    sse = torch.empty((m, k), dtype=torch.float32, device=dev)
    count = torch.empty((m, k), dtype=torch.int32, device=dev)
    if logw is not None and logw_out is None:
        logw_out = torch.empty((m, k), dtype=torch.float32, device=dev)
    N.torch_ops().image_overlap_scores(glimpse, glimpse_pos, target_glimpse, hypotheses, [h, w], scale, logw, gain, tau,
                                       sse, count, logw_out, err)
    return OverlapScoresResult(sse, count, logw_out)
