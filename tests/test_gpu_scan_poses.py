"""lidar_scan_poses / lidar_pose_scores and the kernel k_scan_poses (csrc/apg_scan_poses.hip) on the GPU.

The op is compared bit for bit with the numpy restatements of tests/test_scan_poses_host.py (the oracle's segment
scan per ray, themselves checked against the oracle env's observation) at the smallest shapes that cross each of
the kernel's boundaries, with apg_lidar_scan_batch on the device, and -- the test that ties the feature to the
product -- with the env's own obs["lidar"] at the env's own position, for every map source, map_obs mode and backend.
"""

import functools

import numpy as np
import pytest

from test_gpu_lidar_pool import random_pool
from test_map_bits_host import pack_bits_np
from test_oracle_golden import scan_wide
from test_scan_poses_host import normalize_np, pose_scores_np, scan_poses_np

pytestmark = pytest.mark.gpu

MAPS = [(1, 1), (5, 7), (21, 21), (32, 32), (9, 64), (6, 65), (4, 130), (33, 31), (40, 511)]
WIDEST = [(4, 130), (40, 511)]


def oracle():
    from oracle import oracle as o

    o.build()
    return o


def dirs_of(beams, lidar_range):
    from ap_gym_amd.lidar_env import lidar_beam_directions

    return lidar_beam_directions(beams, lidar_range)


@functools.lru_cache(maxsize=None)
def make_maps(h, w):
    """Four maps bool [4, h, w]: oracle mazes / rooms at their registered sizes, else 35 % and 2 % noise."""
    o = oracle()
    if (h, w) == (21, 21):
        return np.stack([o.maze_map(i, 21) for i in range(4)]).astype(bool)
    if (h, w) == (32, 32):
        return np.stack([o.rooms_map(i, 32) for i in range(4)]).astype(bool)
    rng = np.random.default_rng(1000 * h + w)
    return np.stack([rng.random((h, w)) < (0.35 if i % 2 == 0 else 0.02) for i in range(4)])


@functools.lru_cache(maxsize=None)
def make_poses(h, w):
    """float32 [4, 5, 2]: generic interior points, lattice points, a cell centre inside a wall of the set's map,
    points on the map border, points outside the map within 3 cells, (-70, 5) and (1e6, 1e6)."""
    rng = np.random.default_rng(7 * h + w)
    maps = make_maps(h, w)

    def gen():
        return rng.uniform(0, [w, h])

    poses = [gen(), gen(), gen(), gen(), gen(), gen(), gen(),
             (w // 2, h // 2), (w // 2, gen()[1]), (gen()[0], (h + 1) // 2),
             "wall", "wall",
             (0.0, gen()[1]), (float(w), gen()[1]), (gen()[0], float(h)),
             (-1.5, gen()[1]), (w + 2.25, h + 1.0), (gen()[0], -3.0),
             (-70.0, 5.0), (1e6, 1e6)]
    order = rng.permutation(len(poses))
    out = np.zeros((20, 2), np.float32)
    for slot, i in enumerate(order):
        p = poses[i]
        if isinstance(p, str):  # the centre of a wall cell of this set's map (a free map: its first cell)
            ys, xs = np.nonzero(maps[slot // 5])
            j = int(rng.integers(0, len(ys))) if len(ys) else 0
            p = (xs[j] + 0.5, ys[j] + 0.5) if len(ys) else (0.5, 0.5)
        out[slot] = p
    return out.reshape(4, 5, 2)


@functools.lru_cache(maxsize=None)
def expected_scans(h, w, beams, lidar_range, normalize):
    """The restatement's scans of the case, computed once and shared (read-only) by the tests that need it."""
    e = scan_poses_np(oracle(), make_maps(h, w), make_poses(h, w), dirs_of(beams, lidar_range), lidar_range,
                      normalize=normalize)
    e.setflags(write=False)
    return e


def dev_bits(maps, gpu, garbage_seed=None):
    """Packed maps on the device; garbage_seed: random bits at x >= W in every row."""
    import torch

    rows = pack_bits_np(np.asarray(maps, bool))
    if garbage_seed is not None:
        valid = pack_bits_np(np.ones(maps.shape, bool))
        noise = np.random.default_rng(garbage_seed).integers(0, 2**64, rows.shape, dtype=np.uint64)
        rows = rows | (noise & ~valid)
    return torch.as_tensor(rows.view(np.int64), device=gpu)


def dev(a, gpu):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device=gpu)


def raw(t):
    """float32 values as raw bits on the host (tensor or array)."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(got, want):
    """Bit-equal where `want` is a number, NaN where it is NaN."""
    g = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    nan = np.isnan(want)
    return g.shape == want.shape and np.array_equal(np.isnan(g), nan) and np.array_equal(raw(g)[~nan], raw(want)[~nan])


def ranges_of(h, w):
    return (5, 60) if (h, w) in WIDEST else (5,)


# ------------------------------------------------------------------ 1, 2: the op against the restatement
@pytest.mark.parametrize("beams", [1, 7, 32])
@pytest.mark.parametrize("h,w", MAPS)
def test_scans_match_the_restatement_bit_for_bit(gpu, h, w, beams):
    import ap_gym_amd as ap

    bits, poses = dev_bits(make_maps(h, w), gpu), dev(make_poses(h, w), gpu)
    for lidar_range in ranges_of(h, w):
        for normalize in (True, False):
            got = ap.lidar_scan_poses(bits, w, poses, beams=beams, lidar_range=lidar_range, normalize=normalize)
            want = expected_scans(h, w, beams, lidar_range, normalize)
            assert got.shape == (4, 5, beams) and np.array_equal(raw(got), raw(want)), (lidar_range, normalize)


@pytest.mark.parametrize("h,w", MAPS)
def test_padding_bits_are_ignored(gpu, h, w):
    """Random bits at x >= W in every row: identical output (read as they are they would be walls)."""
    import ap_gym_amd as ap

    bits, poses = dev_bits(make_maps(h, w), gpu, garbage_seed=h + w), dev(make_poses(h, w), gpu)
    for beams in (7, 32):
        for lidar_range in ranges_of(h, w):
            got = ap.lidar_scan_poses(bits, w, poses, beams=beams, lidar_range=lidar_range)
            assert np.array_equal(raw(got), raw(expected_scans(h, w, beams, lidar_range, True))), (beams, lidar_range)


# ------------------------------------------------------------------ 3: map ids
def test_map_ids(gpu):
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    h, w, beams = 6, 65, 7
    maps, poses = make_maps(h, w), make_poses(h, w)
    bits, poses_t, dirs = dev_bits(maps, gpu), dev(poses, gpu), dirs_of(beams, 5)
    kw = dict(beams=beams, lidar_range=5)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    want = expected_scans(h, w, beams, 5, True)
    assert np.array_equal(raw(ap.lidar_scan_poses(bits, w, poses_t, None, err=err, **kw)), raw(want))
    ids = [3, 0, 3, 1]  # any order, duplicates
    got = ap.lidar_scan_poses(bits, w, poses_t, torch.tensor(ids, device=gpu), err=err, **kw)
    assert np.array_equal(raw(got), raw(scan_poses_np(oracle(), maps, poses, dirs, 5, ids)))
    one = ap.lidar_scan_poses(bits[2:3].contiguous(), w, poses_t, None, err=err, **kw)  # n_src == 1: every set
    assert np.array_equal(raw(one), raw(scan_poses_np(oracle(), maps[2:3], poses, dirs, 5)))
    assert int(err.item()) == 0
    bad = [0, -1, 2, 4]  # -1 and n_src: never read, scanned against an all-zero map; the others unaffected
    got = ap.lidar_scan_poses(bits, w, poses_t, torch.tensor(bad, device=gpu), err=err, **kw)
    ref = scan_poses_np(oracle(), maps, poses, dirs, 5, bad)
    assert np.array_equal(raw(got), raw(ref))
    assert np.array_equal(raw(ref[[1, 3]]), raw(scan_poses_np(oracle(), np.zeros((2, h, w), bool), poses[[1, 3]], dirs, 5)))
    assert np.array_equal(raw(got[[0, 2]]), raw(want[[0, 2]]))
    assert int(err.item()) == N.APG_ERR_INDEX
    obs = dev(ref[:, 0, :].copy(), gpu)
    err.zero_()
    sc = ap.lidar_pose_scores(bits, w, poses_t, obs, torch.tensor(bad, device=gpu), err=err, **kw)
    assert same_bits(sc, pose_scores_np(ref, ref[:, 0, :])) and int(err.item()) == N.APG_ERR_INDEX
    ap.lidar_scan_poses(bits, w, poses_t, torch.tensor(bad, device=gpu), **kw)  # no error word: nothing else happens


# ------------------------------------------------------------------ 4: bad poses
def test_non_finite_poses_are_nan_and_flagged(gpu):
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    h, w, beams = 33, 31, 7
    bits = dev_bits(make_maps(h, w), gpu)
    want = expected_scans(h, w, beams, 5, True)
    obs = np.ascontiguousarray(want[:, 3, :])
    want_sc = pose_scores_np(want, obs)
    kw = dict(beams=beams, lidar_range=5)
    for value in (np.nan, np.inf, -np.inf):
        for coord in (0, 1):
            poses = make_poses(h, w).copy()
            assert np.isfinite(poses[1, 2]).all()
            poses[1, 2, coord] = value
            err = torch.zeros(1, dtype=torch.int32, device=gpu)
            got = ap.lidar_scan_poses(bits, w, dev(poses, gpu), err=err, **kw).cpu().numpy()
            sc = ap.lidar_pose_scores(bits, w, dev(poses, gpu), dev(obs, gpu), err=err, **kw).cpu().numpy()
            assert int(err.item()) == N.APG_ERR_BAD_POSE, (value, coord)
            assert np.isnan(got[1, 2]).all() and np.isnan(sc[1, 2])
            keep = np.ones((4, 5), bool)
            keep[1, 2] = False
            assert np.array_equal(raw(got[keep]), raw(want[keep])), (value, coord)
            assert np.array_equal(raw(sc[keep]), raw(want_sc[keep])), (value, coord)
    env = ap.make_vec("LIDARLocRooms-v0", num_envs=4, device=gpu, array_backend="torch")
    env.reset(seed=1)
    p = env._t["pos"][:, None, :].clone()
    p[2, 0, 1] = float("nan")
    s = env.scan_poses(p)
    assert torch.isnan(s[2]).all() and torch.equal(s[[0, 1, 3], 0], env.device_outputs()["lidar"][[0, 1, 3]])
    with pytest.raises(ValueError, match="pose"):
        env.check_errors()
    env.check_errors()  # raised once, then clear
    env.close()
    npenv = ap.make_vec("LIDARLocRooms-v0", num_envs=4, device=gpu)
    npenv.reset(seed=1)
    with pytest.raises(ValueError, match="pose"):  # the numpy backend checks at once
        npenv.pose_scores(p.cpu().numpy())
    with pytest.raises(IndexError):
        npenv.scan_poses(p.cpu().numpy()[:2], [0, 4])
    npenv.close()


# ------------------------------------------------------------------ 5: scores
@pytest.mark.parametrize("beams", [1, 7, 33])
def test_scores_match_the_restatement(gpu, beams):
    import torch

    import ap_gym_amd as ap

    h, w = 32, 32
    bits, poses = dev_bits(make_maps(h, w), gpu), dev(make_poses(h, w), gpu)
    scans = expected_scans(h, w, beams, 5, True)
    obs = np.random.default_rng(beams).uniform(-1, 1, (4, beams)).astype(np.float32)
    obs[0] = scans[0, 2]  # set 0: pose 2 reproduces the observation
    obs[1, beams // 2] = np.nan  # set 1: a NaN in observed
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    got = ap.lidar_pose_scores(bits, w, poses, dev(obs, gpu), beams=beams, lidar_range=5, err=err).cpu().numpy()
    want = pose_scores_np(scans, obs)
    assert got.dtype == np.float32 and same_bits(got, want)
    assert got[0, 2] == 0.0 and not np.signbit(got[0, 2])
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2, 3]]).any()
    assert int(err.item()) == 0  # a NaN observation is not an error
    # scan_out: the same launch also stores the normalised scans; the scores are the same
    scan_out = torch.full((4, 5, beams), -7.0, dtype=torch.float32, device=gpu)
    both = ap.lidar_pose_scores(bits, w, poses, dev(obs, gpu), beams=beams, lidar_range=5, scan_out=scan_out)
    assert same_bits(both, want) and np.array_equal(raw(scan_out), raw(scans))


# ------------------------------------------------------------------ 6: boundaries of the work split
def _check_split(gpu, h, w, m, k, beams, seed):
    import ap_gym_amd as ap

    o, rng = oracle(), np.random.default_rng(seed)
    maps = rng.random((m, h, w)) < 0.2
    poses = rng.uniform(-1, [w + 1, h + 1], (m, k, 2)).astype(np.float32)
    import time

    t0 = time.perf_counter()
    want = scan_poses_np(o, maps, poses, dirs_of(beams, 5), 5)
    print(f"split m={m} k={k} beams={beams}: {want.size} rays, {int((want < 1).sum())} hit a wall, "
          f"oracle {time.perf_counter() - t0:.3f} s")
    obs = np.ascontiguousarray(want[:, k // 2, :])
    bits, poses_t = dev_bits(maps, gpu, garbage_seed=seed), dev(poses, gpu)
    got = ap.lidar_scan_poses(bits, w, poses_t, beams=beams, lidar_range=5)
    assert np.array_equal(raw(got), raw(want)), (m, k, beams)
    sc = ap.lidar_pose_scores(bits, w, poses_t, dev(obs, gpu), beams=beams, lidar_range=5).cpu().numpy()
    assert np.array_equal(raw(sc), raw(pose_scores_np(want, obs))), (m, k, beams)
    assert np.all(sc[:, k // 2] == 0.0)


def test_work_split_boundaries(gpu):
    from ap_gym_amd import _native as N

    T = N.SCAN_POSES_TILE
    assert T == 256
    # K * B one below, at and one above a tile (whole poses per tile: 15 x 17 = 255, 16 x 16, 257 x 1, 1 x 257)
    for k, beams in ((15, 17), (16, 16), (T + 1, 1), (1, T + 1), (T - 1, 1), (T, 1)):
        _check_split(gpu, 9, 11, 2, k, beams, seed=k * 1000 + beams)
    # around the small-set threshold (2 K B <= tile: several sets per workgroup), ragged last group
    for k, beams in ((T // 2, 1), (T // 2 + 1, 1), (4, T // 8), (3, 5), (1, 1)):
        _check_split(gpu, 9, 11, 5, k, beams, seed=k * 1000 + beams + 1)
    _check_split(gpu, 9, 11, 2, 2, T + 44, seed=3)  # B larger than a tile: one pose takes several passes
    _check_split(gpu, 12, 70, 1, 1000, 8, seed=4)  # M = 1, K large: 32 tiles of one map


def test_more_small_sets_than_the_grid_holds(gpu):
    """K = 1, B = 1 on 3 x 3 maps, M three more than the grid cap times the sets per workgroup: the workgroups take
    more than one group each, and the last group is ragged."""
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    o, rng = oracle(), np.random.default_rng(12)
    m = N.SCAN_POSES_MAX_GRID * N.SCAN_POSES_MAX_MPW + 3
    maps = rng.random((6, 3, 3)) < 0.3
    distinct = rng.uniform(-0.5, 3.5, (40, 2)).astype(np.float32)
    dirs = dirs_of(1, 5)
    table = np.stack([scan_poses_np(o, maps[i:i + 1], distinct[None], dirs, 5)[0, :, 0] for i in range(6)])  # [6, 40]
    ids, which = rng.integers(0, 6, m), rng.integers(0, 40, m)
    poses = distinct[which][:, None, :]
    obs = np.full((m, 1), 0.25, np.float32)
    bits = dev_bits(maps, gpu, garbage_seed=1)
    got = ap.lidar_scan_poses(bits, 3, dev(poses, gpu), torch.as_tensor(ids, device=gpu), beams=1, lidar_range=5)
    want = table[ids, which]
    assert np.array_equal(raw(got[:, 0, 0]), raw(want))
    sc = ap.lidar_pose_scores(bits, 3, dev(poses, gpu), dev(obs, gpu), torch.as_tensor(ids, device=gpu), beams=1,
                              lidar_range=5)
    assert np.array_equal(raw(sc), raw(pose_scores_np(want[:, None, None], obs)))


def test_empty_queries_launch_nothing(gpu):
    import torch

    import ap_gym_amd as ap

    bits = dev_bits(make_maps(5, 7), gpu)
    assert ap.lidar_scan_poses(bits, 7, torch.zeros((4, 0, 2), device=gpu), beams=3, lidar_range=5).shape == (4, 0, 3)
    none = torch.zeros(0, dtype=torch.int64, device=gpu)
    assert ap.lidar_scan_poses(bits, 7, torch.zeros((0, 2, 2), device=gpu), none, beams=3,
                               lidar_range=5).shape == (0, 2, 3)
    assert ap.lidar_pose_scores(bits, 7, torch.zeros((0, 2, 2), device=gpu), torch.zeros((0, 3), device=gpu), none,
                                beams=3, lidar_range=5).shape == (0, 2)


# ------------------------------------------------------------------ 7: out=
def test_out_at_any_element_offset(gpu):
    import torch

    import ap_gym_amd as ap

    h, w, beams = 5, 7, 7
    bits, poses = dev_bits(make_maps(h, w), gpu), dev(make_poses(h, w), gpu)
    want = expected_scans(h, w, beams, 5, True)
    obs = np.ascontiguousarray(want[:, 1, :])
    want_sc = pose_scores_np(want, obs)
    for offset in (0, 1, 3):
        for shape, ref, call in (
                ((4, 5, beams), want, lambda out: ap.lidar_scan_poses(bits, w, poses, beams=beams, lidar_range=5,
                                                                      out=out)),
                ((4, 5), want_sc, lambda out: ap.lidar_pose_scores(bits, w, poses, dev(obs, gpu), beams=beams,
                                                                   lidar_range=5, out=out))):
            numel = int(np.prod(shape))
            buf = torch.full((numel + offset + 37,), -7.0, dtype=torch.float32, device=gpu)
            out = buf[offset:offset + numel].view(shape)
            assert call(out) is out
            after = buf.cpu().numpy()
            assert np.array_equal(raw(after[offset:offset + numel].reshape(shape)), raw(ref)), (offset, shape)
            assert np.all(after[:offset] == -7.0) and np.all(after[offset + numel:] == -7.0), (offset, shape)


# ------------------------------------------------------------------ 8: against apg_lidar_scan_batch on the device
def test_distances_equal_scan_batch(gpu, oracle_mod):
    """20 000 random poses x 8 beams on the 64 x 64 maps of test_device_scan_matches_oracle_generic_and_near_grid."""
    import ap_gym_amd as ap
    from test_gpu_lidar import _scan_gpu

    rng = np.random.default_rng(11)
    size = 64
    noise = [rng.random((size, size)) < 0.35 for _ in range(2)]
    maps = np.stack([oracle_mod.rooms_map(0, size), oracle_mod.rooms_map(1, size),
                     np.pad(oracle_mod.maze_map(2, size - 1), ((0, 1), (0, 1))), *noise]).astype(bool)
    k, beams = 4000, 8
    poses = rng.uniform(-2, size + 2, (5, k, 2)).astype(np.float32)
    poses[:, ::7] = np.floor(poses[:, ::7]) + rng.choice(np.array([0, 0.5], np.float32), (5, len(poses[0, ::7]), 2))
    dirs = dirs_of(beams, 5)
    q = (poses[:, :, None, :] + dirs[None, None]).astype(np.float32)
    segs = np.concatenate([np.broadcast_to(poses[:, :, None, :], q.shape), q], axis=-1).reshape(-1, 4)
    mi = np.repeat(np.arange(5), k * beams)
    dist, _ = _scan_gpu(gpu, maps, mi, segs)
    got = ap.lidar_scan_poses(dev_bits(maps, gpu), size, dev(poses, gpu), beams=beams, lidar_range=5, normalize=False)
    assert np.array_equal(raw(got).reshape(-1), raw(dist))


# ------------------------------------------------------------------ 8b: against the reference's scan over the model
@pytest.mark.parametrize("mi", range(5))
def test_scans_and_scores_equal_the_reference_model_on_wide_maps(gpu, mi):
    """The pose group of tests/golden/lidar_scan_wide.npz (maps up to 511 wide or high, directions 1..60 long, from
    the fixture): distances, normalised values and scores against the reference's own __lidar_scan over the GEOS model
    -- no oracle in between."""
    import torch

    import ap_gym_amd as ap

    g = scan_wide()
    m, want = g.maps[mi], g.pose_distance[mi][None]  # [1, K, B]
    w, beams = m.shape[1], want.shape[2]
    bits, poses, dirs = dev_bits(m[None], gpu), dev(g.poses[mi][None].copy(), gpu), dev(g.dirs[mi].copy(), gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    kw = dict(beams=beams, lidar_range=g.pose_range, beam_dirs=dirs, err=err)
    got = ap.lidar_scan_poses(bits, w, poses, normalize=False, **kw)
    assert got.shape == want.shape and np.array_equal(raw(got), raw(want))
    norm = normalize_np(want, g.pose_range)
    assert np.array_equal(raw(ap.lidar_scan_poses(bits, w, poses, normalize=True, **kw)), raw(norm))
    obs = np.ascontiguousarray(norm[:, 0, :])  # pose 0's own scan
    sc = ap.lidar_pose_scores(bits, w, poses, dev(obs, gpu), **kw).cpu().numpy()
    assert np.array_equal(raw(sc), raw(pose_scores_np(norm, obs)))
    assert sc[0, 0] == 0.0 and not np.signbit(sc[0, 0]) and (sc[0, 1:] > 0).any()
    assert int(err.item()) == 0


# ------------------------------------------------------------------ 9: the env's own observation
def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _env(ap, source, n, beams, gpu, backend, map_obs):
    kw = dict(num_envs=n, device=gpu, array_backend=backend, lidar_beam_count=beams, max_episode_steps=3)
    if source == "pool":
        return ap.LIDARLocalization2DVectorEnv(dataset=ap.ArrayFloorMapDataset(random_pool(11, 9, 70, seed=4)),
                                               map_obs=map_obs, **kw)
    if "Static" not in source:
        kw["map_obs"] = map_obs
    return ap.make_vec(source, **kw)


ENV_CASES = [(s, n, b, mode) for s, n, b in (("LIDARLocRooms-v0", 70, 8), ("LIDARLocRooms-v0", 70, 33),
                                             ("LIDARLocMaze-v0", 5, 8), ("pool", 70, 8))
             for mode in ("dense", "bits")] + [("LIDARLocRoomsStatic-v0", 9, 8, "dense")]  # (static ids: one mode)


@pytest.mark.parametrize("backend", ["torch", "numpy"])
@pytest.mark.parametrize("source,n,beams,map_obs", ENV_CASES)
def test_scan_at_the_envs_position_is_its_observation(gpu, source, n, beams, map_obs, backend):
    import ap_gym_amd as ap

    env = _env(ap, source, n, beams, gpu, backend, map_obs)
    h, w = env.dataset.map_height, env.dataset.map_width
    rng = np.random.default_rng(n + beams)
    ids = np.array([n - 1, 0, 2, n - 1])
    wpr = (w + 63) // 64

    def give(a):  # the backend's array type
        return a if backend == "numpy" else dev(a, gpu)

    def check(obs, where):
        pos = env._t["pos"].cpu().numpy()
        lidar = host(obs["lidar"])
        got = env.scan_poses(give(pos[:, None, :]))
        assert type(got) is (np.ndarray if backend == "numpy" else type(env._t["pos"]))
        assert np.array_equal(raw(got)[:, 0, :], raw(lidar)), where
        # pose 0 the true position, the others elsewhere: column 0 exactly 0, the others the restatement's
        poses = np.stack([pos, pos + np.float32(0.61), rng.uniform(0, [w, h], (n, 2)).astype(np.float32)], axis=1)
        sc = host(env.pose_scores(give(poses)))
        assert sc.shape == (n, 3) and np.all(sc[:, 0] == 0.0), where
        scans = host(env.scan_poses(give(poses)))
        assert np.array_equal(raw(sc), raw(pose_scores_np(scans, lidar))), where
        rows = env._t["occ"].view(-1, h, wpr).cpu().numpy().view(np.uint64)
        maps = np.unpackbits(rows.view(np.uint8).reshape(len(rows), h, -1), axis=-1, bitorder="little")[..., :w]
        some = [0, n // 2, n - 1]
        ref = scan_poses_np(oracle(), maps if env.static_map else maps[some], poses[some], dirs_of(beams, 5), 5)
        print(f"{where}: lidar {lidar.shape}, {int((lidar < 1).sum())} beams hit a wall, {ref.size} rays restated, "
              f"{int(maps.sum())} wall cells in {len(maps)} maps")
        assert np.array_equal(raw(scans[some]), raw(ref)), where
        # env_ids: subsets, any order, duplicates; observed given or taken from the env
        sub = host(env.scan_poses(give(poses[ids]), ids, normalize=False))
        assert np.array_equal(raw(np.clip(sub / np.float32(5), -1, 1)), raw(scans[ids])), where
        assert np.array_equal(raw(host(env.pose_scores(give(poses[ids]), None, ids))), raw(sc[ids])), where
        shifted = np.roll(lidar, 1, axis=0)
        assert np.array_equal(raw(host(env.pose_scores(give(poses[ids]), give(shifted[ids]), ids))),
                              raw(pose_scores_np(scans[ids], shifted[ids]))), where

    obs, _ = env.reset(seed=17)
    check(obs, "reset")
    for t in range(6):  # max_episode_steps = 3: the fourth step is the autoreset step
        a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        p = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        obs = env.step({"action": a, "prediction": p})[0]
        check(obs, f"step {t}")
    out = env.scan_poses(give(env._t["pos"].cpu().numpy()[:, None, :]),
                         out=give(np.zeros((n, 1, beams), np.float32)))
    assert np.array_equal(raw(out)[:, 0, :], raw(host(obs["lidar"])))
    env.check_errors()
    env.close()


# ------------------------------------------------------------------ 10: graph capture
def test_op_is_graph_capturable(gpu):
    """The op captured in a CUDA graph: replays after changing `poses` in place equal eager calls."""
    import torch

    import ap_gym_amd as ap

    h, w, beams = 32, 32, 8
    bits = dev_bits(make_maps(h, w), gpu)
    poses = dev(make_poses(h, w), gpu).clone()
    obs = dev(np.ascontiguousarray(expected_scans(h, w, beams, 5, True)[:, 0, :]), gpu)
    kw = dict(beams=beams, lidar_range=5)
    scan = torch.zeros((4, 5, beams), dtype=torch.float32, device=gpu)
    score = torch.zeros((4, 5), dtype=torch.float32, device=gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    ap.lidar_scan_poses(bits, w, poses, out=scan, err=err, **kw)  # (loads the library, caches the directions)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ap.lidar_scan_poses(bits, w, poses, out=scan, err=err, **kw)
            ap.lidar_pose_scores(bits, w, poses, obs, out=score, err=err, **kw)
    torch.cuda.current_stream(gpu).wait_stream(side)
    g = torch.Generator(device=gpu).manual_seed(5)
    for t in range(3):
        poses.copy_(torch.rand((4, 5, 2), device=gpu, generator=g) * (w + 4) - 2)
        graph.replay()
        assert torch.equal(scan, ap.lidar_scan_poses(bits, w, poses, **kw)), t
        assert torch.equal(score, ap.lidar_pose_scores(bits, w, poses, obs, **kw)), t
    assert torch.equal(scan[:, :, 0], ap.lidar_scan_poses(bits, w, poses, beams=beams, lidar_range=5)[:, :, 0])
    assert int(err.item()) == 0
