"""Host-side checks of the step kernel's resident window cache (no GPU): its size per configuration, the unchanged
apg_lidar_query_sizes, and a CPU replay of the zone rule over the oracle's positions."""

import ctypes

import numpy as np


def _cfg(N, **kw):
    base = dict(num_envs=4, height=64, width=64, map_kind=N.APG_MAP_ROOMS, is_static=0, beams=32, step_limit=100,
                max_rooms=10, door_width=3, lidar_range=5.0, loss_scale=3.0, branching_prob=1.0)
    base.update(kw)
    return N.LidarConfig(**base)


def _zone(N, cfg, inner):
    z, drift = (ctypes.c_int32 * 4)(), ctypes.c_int32()
    rc = N.lib().apg_lidar_window_cache_zone(ctypes.byref(cfg), inner, z, ctypes.byref(drift))
    return rc, list(z), drift.value


def test_window_cache_bytes_and_zones():
    from ap_gym_amd import _native as N

    nbytes = N.lib().apg_lidar_window_cache_bytes
    # 32 rows of u32 and one origin word per env
    assert nbytes(ctypes.byref(_cfg(N))) == 4 * 33 * 4
    assert nbytes(ctypes.byref(_cfg(N, num_envs=65536))) == 65536 * 132
    assert nbytes(ctypes.byref(_cfg(N, map_kind=N.APG_MAP_MAZE, height=127, width=127, num_envs=300))) == 300 * 132
    assert nbytes(ctypes.byref(_cfg(N, is_static=1))) == 4 * 132
    # the inner zone is empty above range 6; above 10 the step reads its rows from global memory (GR instances)
    for r, want in ((0.5, 528), (5.5, 528), (6.0, 528), (6.5, 0), (7.0, 0), (10.0, 0), (10.5, 0), (28.0, 0), (60.0, 0)):
        assert nbytes(ctypes.byref(_cfg(N, lidar_range=r))) == want, r
    assert nbytes(ctypes.byref(_cfg(N, height=512))) == 0  # an invalid configuration
    assert nbytes(None) == 0
    # query_sizes is what it was: the cache is not part of it
    sz = N.LidarSizes()
    assert N.lib().apg_lidar_query_sizes(ctypes.byref(_cfg(N)), ctypes.byref(sz)) == 0
    assert sz.scratch_bytes == 0 and sz.occ_bytes == 4 * 64 * 8 and sz.stack_bytes == 0 and sz.prefetch_bytes == 0
    assert b" 0.4.0 " in N.lib().apg_version()
    # zones: offsets floor(pos) - origin; rows need R + 7 on both sides of 32, columns R + 5; the inner zone is 2 in
    assert _zone(N, _cfg(N), 0) == (0, [10, 21, 12, 19], 2)
    assert _zone(N, _cfg(N), 1) == (0, [12, 19, 14, 17], 2)
    assert _zone(N, _cfg(N, lidar_range=6.0), 1) == (0, [13, 18, 15, 16], 2)
    for r in (1.0, 3.0, 5.0, 6.0):  # a freshly centred window (offset 15) is inside the inner zone
        _, z, _ = _zone(N, _cfg(N, lidar_range=r), 1)
        assert z[0] <= 15 <= z[1] and z[2] <= 15 <= z[3], (r, z)
    assert _zone(N, _cfg(N, lidar_range=7.0), 0)[0] == N.APG_E_INVALID
    assert b"window cache" in N.lib().apg_last_error()


def test_zone_rule_replayed_over_oracle_positions(oracle_mod):
    """The cache's rule, replayed per env over the oracle's trajectory (rooms 64 x 64, 512 envs, 100 steps, uniform
    actions): a window is centred on the env's position at a reset and re-centred when the pre-move position lies
    outside the inner zone.  No step may start outside the hard zone, and floor(pos) may not change by more than the
    bound the inner zone is built on."""
    from ap_gym_amd import _native as N

    n, steps = 512, 100
    cfg = _cfg(N, num_envs=n)
    _, hard, drift = _zone(N, cfg, 0)
    _, inner, _ = _zone(N, cfg, 1)
    ref = oracle_mod.OracleLidarVectorEnv(n, "rooms", 64, False, 0, 32, lidar_range=5.0, step_limit=100)
    ref.reset(0)
    rng = np.random.default_rng(1)
    cell = np.floor(ref.state()["pos"]).astype(np.int64)
    origin = cell - 15
    recentred = max_change = 0
    for t in range(steps):
        a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        pending = ref.state()["autoreset"].astype(bool)  # these envs reset at this step: their workgroup falls back
        off = cell - origin
        in_hard = (off[:, 0] >= hard[0]) & (off[:, 0] <= hard[1]) & (off[:, 1] >= hard[2]) & (off[:, 1] <= hard[3])
        assert (in_hard | pending).all(), f"step {t}: envs {np.nonzero(~(in_hard | pending))[0][:8]} outside the hard zone"
        in_inner = (off[:, 0] >= inner[0]) & (off[:, 0] <= inner[1]) & (off[:, 1] >= inner[2]) & (off[:, 1] <= inner[3])
        ref.step(a, a)
        new_cell = np.floor(ref.state()["pos"]).astype(np.int64)
        moved = ~pending
        max_change = max(max_change, int(np.abs(new_cell - cell)[moved].max()))
        # a reset env does not move at its reset step: the fallback centres the window on its new position
        origin = np.where(pending[:, None], new_cell - 15, np.where(in_inner[:, None], origin, cell - 15))
        recentred += int((~in_inner & ~pending).sum())
        cell = new_cell
    ref.close()
    print(f"re-centred {recentred / (n * steps):.3f} of the env steps, largest floor change {max_change}")
    assert max_change <= drift
    assert 0 < recentred < n * steps // 2
