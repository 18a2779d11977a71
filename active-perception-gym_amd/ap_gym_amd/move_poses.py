"""Exact open-loop rollouts of candidate actions from caller-chosen poses, on packed maps (the HIP kernel k_move_poses,
csrc/apg_move_poses.hip).

Where would this action take the agent?  `lidar_move_poses` answers with the env's own movement -- the reference's
`_step` (clamp to unit length, scan to the first wall, slide along the positive components of what remains, the 1e-5
thresholds, the clip) in the float32 operation order of the step kernel, bit for bit -- for K candidates per map and
T actions per candidate at once, without an env being advanced.  With `lidar_scan_poses` on the resulting poses a
planner, a particle filter's motion update or a model-based method gets what `step()` would observe after each
candidate action.

Maps are packed bit rows (map_bits.py: int64 [n_src, H, ceil(W / 64)], the layout of map_obs="bits"; the padding bits
at x >= W are ignored).  Poses are (x, y) in cells.  Limits: map sides 1..511, 1 <= T <= 4096.  Domain: a candidate
with a non-finite start pose or action is not moved from that action on (NaN outputs, APG_ERR_BAD_POSE in `err`); a
finite start pose outside the map is legal and terminates with its first action.
"""

from __future__ import annotations

from typing import NamedTuple

from . import _native as N
from .map_bits import MAX_MAP_SIDE, words_per_row

MAX_ACTIONS = N.MOVE_POSES_MAX_T


class MovePosesResult(NamedTuple):
    """pos float32 [M, K, T, 2]; steps int32 [M, K]; terminated uint8 [M, K]; base_reward float32 [M, K, T] or None;
    odometry float32 [M, K, T, 2] or None."""

    pos: object
    steps: object
    terminated: object
    base_reward: object
    odometry: object


def _check(bits, width, poses, actions, map_ids, max_steps, origin, origin_alias, odometry):
    """Everything that can be checked on tensors of any device; returns (width, M, K, T)."""
    import torch

    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int64 or bits.dim() != 3:
        raise TypeError("bits must be an int64 tensor [n_src, H, ceil(width / 64)]")
    if not isinstance(poses, torch.Tensor) or poses.dtype != torch.float32:
        raise TypeError("poses must be a float32 tensor [M, K, 2]")
    if poses.dim() != 3 or poses.shape[2] != 2:
        raise ValueError(f"poses must have shape [M, K, 2], got {tuple(poses.shape)}")
    m, k = poses.shape[0], poses.shape[1]
    if not isinstance(actions, torch.Tensor) or actions.dtype != torch.float32:
        raise TypeError("actions must be a float32 tensor [M, K, T, 2]")
    if actions.dim() != 4 or tuple(actions.shape[:2]) != (m, k) or actions.shape[3] != 2:
        raise ValueError(f"actions must have shape [{m}, {k}, T, 2], got {tuple(actions.shape)}")
    t = actions.shape[2]
    if not 1 <= t <= MAX_ACTIONS:
        raise ValueError(f"actions: T must be in 1..{MAX_ACTIONS}, got {t}")
    width = int(width)
    if not 1 <= width <= MAX_MAP_SIDE or not 1 <= bits.shape[1] <= MAX_MAP_SIDE:
        raise ValueError(f"map height and width must be in 1..{MAX_MAP_SIDE}")
    if bits.shape[2] != words_per_row(width):
        raise ValueError(f"bits has {bits.shape[2]} words per row, width {width} needs {words_per_row(width)}")
    if map_ids is not None:
        if not isinstance(map_ids, torch.Tensor) or map_ids.dtype != torch.int64 or map_ids.dim() != 1:
            raise TypeError("map_ids must be a 1-d int64 tensor (or None)")
        if map_ids.shape[0] != m:
            raise ValueError(f"map_ids must have one id per candidate set ({m}), got {map_ids.shape[0]}")
    elif bits.shape[0] != 1 and bits.shape[0] != m:
        raise ValueError(f"without map_ids, bits must hold one map or one per candidate set ({m}), got {bits.shape[0]}")
    for name, x, dtype, shape in (("max_steps", max_steps, torch.int32, (m,)),
                                  ("origin", origin, torch.float32, (m, 2)),
                                  ("origin_alias", origin_alias, torch.uint8, (m,))):
        if x is None:
            continue
        if not isinstance(x, torch.Tensor) or x.dtype != dtype:
            raise TypeError(f"{name} must be a {str(dtype).replace('torch.', '')} tensor {list(shape)}")
        if tuple(x.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(x.shape)}")
    if origin is None and (odometry or origin_alias is not None):
        raise ValueError("odometry and origin_alias need origin (the odometry origin of each candidate set)")
    return width, m, k, t


def lidar_move_poses(bits, width: int, poses, actions, map_ids=None, *, max_steps=None, origin=None,
                     origin_alias=None, base_reward: bool = True, odometry: bool | None = None, err=None):
    """Roll the candidate actions `actions` (float32 [M, K, T, 2]) out from the start poses `poses` (float32 [M, K, 2],
    (x, y) in cells) on the packed maps `bits` (contiguous int64 [n_src, H, ceil(width / 64)] on a GPU device):
    candidate set m moves on map `map_ids[m]` (a 1-d int64 tensor, any order, duplicates allowed; None: map m, or the
    one map when n_src == 1).  Each action is the env's movement, bit for bit: clamp to unit length, the exact scan to
    the first wall, the slide, `left the map` before the clip.  A candidate terminates at the first action t (1-based)
    after which it has left the map or t >= max_steps[m].

    max_steps     int32 [M] or None: TimeLimit with issue_termination=True; values <= 0 mean no limit
    origin        float32 [M, 2] or None: the odometry origin of each set
    origin_alias  uint8 [M] or None (needs origin): where set, the origin of every candidate of the set is that
                  candidate's own pose after its first action, before the clip -- the reference's `initial_pos`
                  aliases `pos` during the first step of an episode
    base_reward   False: the base rewards are not computed
    odometry      None: computed when `origin` is given; True needs `origin`
    err           an int32 [1] device tensor: a map id outside [0, n_src) moves on an all-zero map (it is never read)
                  and sets APG_ERR_INDEX; a non-finite start pose or action sets APG_ERR_BAD_POSE

    Returns a MovePosesResult:
      pos          float32 [M, K, T, 2], the pose after each action; entries after the terminating action repeat the
                   final (clipped) pose
      steps        int32 [M, K], the number of actions applied: the terminating t, or T
      terminated   uint8 [M, K]
      base_reward  float32 [M, K, T] = 0.1 - 0.001 |a|^2 of the unclamped action, 0 after termination (or None)
      odometry     float32 [M, K, T, 2], the observation's normalised odometry, repeated after termination (or None)
    A candidate with a non-finite start pose or action has NaN pos / base_reward / odometry from that action on,
    `steps` = the valid actions before it and terminated = 0.

    Runs on the current stream without synchronising the host."""
    import torch

    if odometry is None:
        odometry = origin is not None
    width, m, k, t = _check(bits, width, poses, actions, map_ids, max_steps, origin, origin_alias, odometry)
    # the device and contiguity checks, last: everything else was checked on tensors of any device
    if bits.device.type != "cuda":
        raise ValueError(f"bits must be on a GPU device, got {bits.device} (there is no CPU fallback)")
    if not bits.is_contiguous():
        raise ValueError("bits must be contiguous")
    for name, x in dict(poses=poses, actions=actions, map_ids=map_ids, max_steps=max_steps, origin=origin,
                        origin_alias=origin_alias).items():
        if x is not None and (x.device != bits.device or not x.is_contiguous()):
            raise ValueError(f"{name} must be contiguous and on {bits.device}")
    if err is not None and (not isinstance(err, torch.Tensor) or err.dtype != torch.int32 or err.numel() != 1
                            or err.device != bits.device):
        raise ValueError(f"err must be an int32 [1] tensor on {bits.device}")
    dev = bits.device
    pos = torch.empty((m, k, t, 2), dtype=torch.float32, device=dev)
    steps = torch.empty((m, k), dtype=torch.int32, device=dev)
    terminated = torch.empty((m, k), dtype=torch.uint8, device=dev)
    br = torch.empty((m, k, t), dtype=torch.float32, device=dev) if base_reward else None
    odo = torch.empty((m, k, t, 2), dtype=torch.float32, device=dev) if odometry else None
    N.torch_ops().lidar_move_poses(bits, width, poses, actions, map_ids, max_steps, origin, origin_alias, pos, steps,
                                   terminated, br, odo, err)
    return MovePosesResult(pos, steps, terminated, br, odo)
