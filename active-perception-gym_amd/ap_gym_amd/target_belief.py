"""A belief over the target position of the image localization envs, built from what the agent itself observes: two
device launches per step and no host synchronisation.

    update   image_overlap_scores  where the glimpse and the target glimpse would overlap under each hypothesis, how
                                   well do they agree?  Fused: logw += (tau * count - sse) / (2 sigma^2)
             lidar_pf_resample     weights, the weighted-mean estimate, the effective sample size (ess_frac = 0: the
                                   hypotheses are a fixed set and are never resampled)

    env = ap.make_vec("TinyImageNetLoc-v0", num_envs=1024, array_backend="torch")
    belief = ap.ImageTargetBelief(env, grid=(32, 32), sigma=0.1, tau=0.01)
    obs, _ = env.reset(seed=0)
    belief.reset()
    belief.update()
    for _ in range(steps):
        obs, *_ = env.step({"action": belief.choose_action(), "prediction": belief.prediction})
        belief.update()

The belief reads the env's device buffers (obs["glimpse"], obs["glimpse_pos"], obs["target_glimpse"]) and never the
image: it is a non-learning baseline an agent could run, and a belief to feed a policy.  It works on a torch-backend
ImageLocalizationVectorEnv.  ShardedVectorEnv does not forward it (build one belief per shard's env).
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np


class TargetBeliefResult(NamedTuple):
    weight: object    # float32 [N, K] exp(logw - max logw): the maximum is 1
    estimate: object  # float32 [N, 2] the weighted-mean hypothesis, in the env's prediction space
    ess: object       # float32 [N] the effective sample size of the weights
    logw: object      # float32 [N, K] the belief's log-weights after this update (the belief's own buffer)
    sse: object       # float32 [N, K] this update's sum of squared differences over the overlap
    count: object     # int32 [N, K] this update's number of compared values


class ImageTargetBelief:
    """Log-weights over a fixed set of K <= 4096 hypotheses of the target position for each sub-env of `env`.

    hypotheses  None: the grid below; or float [K, 2] (shared by every sub-env) or [num_envs, K, 2], normalised (x, y)
    grid        (gx, gy): the hypotheses (x_i, y_j) = (linspace(-1, 1, gx)[i], linspace(-1, 1, gy)[j]), hypothesis
                j * gx + i
    sigma       standard deviation of the Gaussian likelihood of one compared value: log-weights change by
                (tau * count - sse) / (2 sigma^2)
    tau         the squared difference per compared value at which an overlap is neither evidence for nor against a
                hypothesis (an overlap that matches better raises its weight)
    """

    def __init__(self, env, hypotheses=None, *, grid=(32, 32), sigma: float, tau: float):
        import torch

        from . import _native as N
        from .pf_resample import MAX_PARTICLES

        if (getattr(env, "array_backend", None) != "torch" or not hasattr(env, "target_overlap")
                or getattr(env, "kind", None) != N.APG_IMAGE_LOCALIZE):
            raise ValueError("ImageTargetBelief needs an image localization env with array_backend='torch'")
        if not 0.0 < float(sigma) < float("inf"):
            raise ValueError(f"sigma must be positive and finite, got {sigma}")
        if not 0.0 <= float(tau) < float("inf"):
            raise ValueError(f"tau must be >= 0 and finite, got {tau}")
        self.env = env
        self.sigma = float(sigma)
        self.tau = float(tau)
        self.gain = float(np.float32(1.0 / (2.0 * self.sigma * self.sigma)))
        self._dev = dev = env._dev
        n = env.num_envs
        if hypotheses is None:
            gx, gy = (int(v) for v in grid)
            if gx < 1 or gy < 1:
                raise ValueError(f"grid must hold positive sizes, got {grid}")
            # (numpy's linspace, evaluated in float64 and rounded once: symmetric about 0)
            xs = torch.from_numpy(np.linspace(-1.0, 1.0, gx).astype(np.float32))
            ys = torch.from_numpy(np.linspace(-1.0, 1.0, gy).astype(np.float32))
            h = torch.stack([xs[None, :].expand(gy, gx), ys[:, None].expand(gy, gx)], dim=-1).reshape(gx * gy, 2)
        else:
            h = torch.as_tensor(hypotheses).to(torch.float32)
        if not ((h.dim() == 2 and h.shape[1] == 2) or (h.dim() == 3 and tuple(h.shape[::2]) == (n, 2))):
            raise ValueError(f"hypotheses must have shape [K, 2] or [{n}, K, 2], got {tuple(h.shape)}")
        k = int(h.shape[-2])
        if not 1 <= k <= MAX_PARTICLES:
            raise ValueError(f"the belief holds 1..{MAX_PARTICLES} hypotheses, got {k}")
        h = h.to(dev).contiguous().clone()
        self._h = h  # what the overlap kernel reads: [K, 2] when the set is shared
        self.hypotheses = h if h.dim() == 3 else h[None].expand(n, k, 2).contiguous()  # [N, K, 2] (lidar_pf_resample)
        self.num_hypotheses = k
        msl = env._cfg.max_step
        self._msl = torch.tensor([msl[0], msl[1]], dtype=torch.float32, device=dev)
        self.logw = None
        self.last = None
        self._batch = None

    def reset(self):
        """Start over: every log-weight 0."""
        import torch

        if self.logw is None:
            self.logw = torch.zeros((self.env.num_envs, self.num_hypotheses), dtype=torch.float32, device=self._dev)
        else:
            self.logw.zero_()
        self._batch = self.env.batch_count
        self.last = None
        return self

    def update(self):
        """The measurement update against the env's current observation; returns a TargetBeliefResult.  When the env
        has drawn a new batch since the last update (its last step was the batch autoreset: new images and targets),
        the log-weights start from 0 again; the env knows that on the host, so nothing is read from the device."""
        from .overlap_scores import image_overlap_scores
        from .pf_resample import lidar_pf_resample

        if self.logw is None:
            raise RuntimeError("call reset() first")
        env = self.env
        if env.batch_count != self._batch:
            self.logw.zero_()
            self._batch = env.batch_count
        T, c, err = env._t, env._cfg, env._t["err"]
        res = image_overlap_scores(T["glimpse"].contiguous(), T["glimpse_pos"].contiguous(),
                                   T["target_glimpse"].contiguous(), self._h, image_size=env.image_size,
                                   sensor_size=(c.sensor_h, c.sensor_w), sensor_scale=c.sensor_scale, logw=self.logw,
                                   gain=self.gain, tau=self.tau, logw_out=self.logw, err=err)
        pf = lidar_pf_resample(self.hypotheses, self.logw, ess_frac=0.0, err=err)
        self.last = TargetBeliefResult(pf.weight, pf.estimate, pf.ess, self.logw, res.sse, res.count)
        return self.last

    @property
    def prediction(self):
        """The weighted-mean hypothesis [num_envs, 2] of the last update(): already in the env's prediction space, the
        value to pass as `prediction` to env.step()."""
        if self.last is None:
            raise RuntimeError("no estimate yet: call update()")
        return self.last.estimate

    @property
    def best(self):
        """The hypothesis of largest log-weight [num_envs, 2] (the lowest index among equals; a NaN never wins)."""
        import torch

        if self.logw is None:
            raise RuntimeError("call reset() first")
        lw = torch.where(torch.isnan(self.logw), torch.full_like(self.logw, float("-inf")), self.logw)
        idx = lw.argmax(dim=1)
        return self.hypotheses[torch.arange(idx.shape[0], device=self._dev), idx]

    def choose_action(self):
        """A plain baseline policy, float32 [num_envs, 2]: head for the best hypothesis, (best - glimpse_pos) /
        max_step_length per component, divided by max(1, its norm).  Unvisited hypotheses tie at 0 and refuted ones
        fall below, so the sensor sweeps the hypotheses in index order until something matches, and then stays.
        Never synchronises the host."""
        import torch

        a = (self.best - self.env._t["glimpse_pos"]) / self._msl
        return a / torch.linalg.vector_norm(a, dim=1, keepdim=True).clamp(min=1.0)
