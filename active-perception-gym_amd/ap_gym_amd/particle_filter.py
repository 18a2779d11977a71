"""A particle filter for the LIDAR localisation envs, three device launches per step and no host synchronisation:

    predict   lidar_move_poses   every particle makes the env's own move (clamp, collide, slide, clip), bit for bit
    update    lidar_pose_scores  the squared error between each particle's exact scan and the observed one
              lidar_pf_resample  weights, estimate, effective sample size, systematic resampling (deterministic)

    env = ap.make_vec("LIDARLocRooms-v0", num_envs=1024, array_backend="torch")
    pf = ap.LidarParticleFilter(env, 256, sigma=0.05, motion_noise=0.02)
    obs, _ = env.reset(seed=0)
    pf.reset()
    pf.update()
    for _ in range(steps):
        obs, *_ = env.step({"action": action, "prediction": pf.prediction})
        pf.predict(action)
        pf.update()

`pf.choose_action(candidates)` closes the loop from the belief to the next action: the candidate after which the
particles would disagree most about what they see (lidar_scan_spread, two more launches).

The filter reads the env's device buffers (occupancy rows, obs["lidar"], reset_mask): it works on a torch-backend
LIDARLocalization2DVectorEnv, in both map_obs modes and for every map source.  ShardedVectorEnv does not forward it
(build one filter per shard's env).
"""

from __future__ import annotations

from .move_poses import lidar_move_poses


class LidarParticleFilter:
    """`num_particles` (1..4096) particles for each sub-env of `env`.

    sigma         standard deviation of the Gaussian likelihood of the summed squared scan error (normalised readings):
                  log-weights fall by score / (2 sigma^2)
    motion_noise  standard deviation, in cells, of the Gaussian noise added to the action of each particle in
                  predict(); 0: none is drawn
    ess_frac      a set is resampled when its effective sample size falls below ess_frac * num_particles
    generator     a torch.Generator on the env's device for every draw (None: the device's default generator)
    """

    def __init__(self, env, num_particles: int, *, sigma: float, motion_noise: float = 0.0, ess_frac: float = 0.5,
                 generator=None):
        import torch

        from .pf_resample import MAX_PARTICLES

        if getattr(env, "array_backend", None) != "torch" or not hasattr(env, "pf_update"):
            raise ValueError("LidarParticleFilter needs a LIDAR env with array_backend='torch'")
        if not 1 <= int(num_particles) <= MAX_PARTICLES:
            raise ValueError(f"num_particles must be in 1..{MAX_PARTICLES}, got {num_particles}")
        if not 0.0 < float(sigma) < float("inf"):
            raise ValueError(f"sigma must be positive and finite, got {sigma}")
        if not 0.0 <= float(motion_noise) < float("inf"):
            raise ValueError(f"motion_noise must be >= 0 and finite, got {motion_noise}")
        self.env = env
        self.num_particles = int(num_particles)
        self.sigma = float(sigma)
        self.motion_noise = float(motion_noise)
        self.ess_frac = float(ess_frac)
        self.generator = generator
        self._dev = env._dev
        w, h = env.dataset.map_width, env.dataset.map_height
        self._size = torch.tensor([w, h], dtype=torch.float32, device=self._dev)
        # the step kernel's target is float32(float64(pos) * (1.0 / float64(float32(side)))) * 2 - 1
        self._inv_size = torch.tensor([1.0 / w, 1.0 / h], dtype=torch.float64, device=self._dev)
        self.particles = None
        self.logw = None
        self.last = None

    def _uniform(self):
        import torch

        n, k = self.env.num_envs, self.num_particles
        return torch.rand((n, k, 2), dtype=torch.float32, device=self._dev, generator=self.generator) * self._size

    def reset(self, particles=None):
        """Start over: `particles` float32 [num_envs, num_particles, 2] in cells, or None for a uniform draw over the
        map rectangle.  Uniform particles that fall inside walls are not removed: they score badly at the first
        update() and die there."""
        import torch

        n, k = self.env.num_envs, self.num_particles
        if particles is None:
            particles = self._uniform()
        else:
            particles = torch.as_tensor(particles, dtype=torch.float32, device=self._dev).contiguous().clone()
            if tuple(particles.shape) != (n, k, 2):
                raise ValueError(f"particles must have shape {(n, k, 2)}, got {tuple(particles.shape)}")
        self.particles = particles
        self.logw = torch.zeros((n, k), dtype=torch.float32, device=self._dev)
        self.last = None
        return self

    def predict(self, action):
        """The motion update after env.step(action): `action` float32 [num_envs, 2].  The sets of the sub-envs that
        autoreset in that step (the env's reset_mask) are drawn anew, uniformly, with log-weights 0, and their action
        counts as zero (the env ignores the action of such a step).  Then every particle makes the env's own move
        under action[m] + motion_noise * randn, without a step limit."""
        import torch

        if self.particles is None:
            raise RuntimeError("call reset() first")
        env, n, k = self.env, self.env.num_envs, self.num_particles
        a = torch.as_tensor(action, dtype=torch.float32, device=self._dev)
        if tuple(a.shape) != (n, 2):
            raise ValueError(f"action must have shape {(n, 2)}, got {tuple(a.shape)}")
        fresh = env.device_outputs()["reset_mask"].bool()
        start = torch.where(fresh[:, None, None], self._uniform(), self.particles)
        self.logw = torch.where(fresh[:, None], torch.zeros_like(self.logw), self.logw)
        a = torch.where(fresh[:, None], torch.zeros_like(a), a)[:, None, :].expand(n, k, 2)
        if self.motion_noise > 0.0:
            a = a + self.motion_noise * torch.randn((n, k, 2), dtype=torch.float32, device=self._dev,
                                                    generator=self.generator)
        bits, start, map_ids, _ = env._pose_query(start, None)
        res = lidar_move_poses(bits, env.dataset.map_width, start, a[:, :, None, :].contiguous(), map_ids,
                               base_reward=False, err=env._t["err"])
        self.particles = res.pos.view(n, k, 2)
        return self.particles

    def update(self):
        """The measurement update against the env's current obs["lidar"], and resampling (env.pf_update).  Keeps the
        resampled particles and log-weights; returns the PfUpdateResult."""
        import torch

        if self.particles is None:
            raise RuntimeError("call reset() first")
        u = torch.rand(self.env.num_envs, dtype=torch.float32, device=self._dev, generator=self.generator)
        res = self.env.pf_update(self.particles, self.logw, sigma=self.sigma, ess_frac=self.ess_frac, u=u)
        self.particles, self.logw, self.last = res.poses, res.logw, res
        return res

    def action_spread(self, candidates, *, mean: bool = False):
        """env.action_spread of the filter's particles with the weights exp(logw), for the candidate actions
        `candidates` float32 [num_envs, A, 2] or [num_envs, A, T, 2]: how much the belief's hypotheses would disagree
        about what they see after each candidate.  Changes neither the filter nor the env."""
        import torch

        if self.particles is None:
            raise RuntimeError("call reset() first")
        return self.env.action_spread(self.particles, candidates, torch.exp(self.logw), mean=mean)

    def choose_action(self, candidates):
        """The candidate that tells the belief's hypotheses apart best: (action [num_envs, 2], spread [num_envs, A]),
        where `action` is the first action of the candidate with the largest spread (the lowest index among equals).
        A NaN spread (no particle of positive weight under that candidate) never wins; where every spread is NaN the
        first candidate is returned."""
        import torch

        c = torch.as_tensor(candidates, dtype=torch.float32, device=self._dev)
        spread = self.action_spread(c)["spread"]
        best = torch.where(torch.isnan(spread), torch.full_like(spread, -1.0), spread).argmax(dim=1)  # (spread >= 0)
        first = c if c.dim() == 3 else c[:, :, 0, :]
        return first[torch.arange(first.shape[0], device=self._dev), best], spread

    @property
    def estimate(self):
        """The weighted-mean pose [num_envs, 2] in cells of the last update() (before its resampling)."""
        if self.last is None:
            raise RuntimeError("no estimate yet: call update()")
        return self.last.estimate

    @property
    def prediction(self):
        """The estimate in the env's prediction space, [-1, 1]^2: the value to pass as `prediction` to the next
        env.step(), computed with the float32 operations the step kernel applies to its `target` (the position
        before the move), so a filter that holds the true position predicts the next step's target bit for bit."""
        return (self.estimate.double() * self._inv_size).float() * 2.0 - 1.0
