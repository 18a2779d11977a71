"""lidar_scan_spread, the kernel k_scan_spread (csrc/apg_scan_spread.hip), env.action_spread and
LidarParticleFilter.choose_action on the GPU.

The kernel is compared bit for bit with the restatement of tests/test_scan_spread_host.py applied to
lidar_scan_poses' normalised scans of the same poses, at the smallest shapes that cross each boundary of its work
split once; then its invariances (order, weight splitting, identical poses), the bound of its integer sums, its input
domain, the tie to the env and the meaning of the number: the candidate that tells two hypotheses apart wins.
"""

import functools

import numpy as np
import pytest

from test_gpu_scan_poses import dev, dev_bits, host, oracle
from test_oracle_golden import scan_wide
from test_scan_poses_host import normalize_np
from test_scan_spread_host import F, scan_spread_np

pytestmark = pytest.mark.gpu

SIDE, RANGE = 24, 5.0


def same(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_values(got, want):
    """Bit-equal float32 arrays, NaN matching NaN (the kernel's and numpy's NaN may differ in payload)."""
    got, want = host(got), np.asarray(want)
    nan = np.isnan(want)
    return (got.dtype == want.dtype == F and got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


@functools.lru_cache(maxsize=None)
def rooms24():
    maps = np.stack([oracle().rooms_map(i, SIDE) for i in range(4)]).astype(bool)
    maps.setflags(write=False)
    return maps


def ppt_of(beams):
    from ap_gym_amd import _native as N

    return max(1, N.SCAN_SPREAD_TILE // beams)


def ragged_m(a):
    """The smallest M whose M * a items leave the last workgroup a shorter run than the others."""
    from ap_gym_amd import _native as N

    m = N.SCAN_SPREAD_MAX_GRID // a + 1
    items = m * a
    per = -(-items // N.SCAN_SPREAD_MAX_GRID)
    assert per == 2 and items % per != 0
    return m


# (beams, K or its offset from ppt, A, M or "ragged", map ids, weights): every boundary of the issue's list once
CASES = [
    (1, 1000, 1, 1, "one", False),
    (3, "ppt-1", 3, 1, "one", True),
    (3, "ppt", 1, 4, "none", False),
    (3, "ppt+1", 1, 3, "dup", True),
    (3, 2, 3, "ragged", "dup", True),
    (32, 1, 3, 1, "one", True),
    (32, 2, 1, 4, "rev", False),
    (32, "ppt-1", 1, 1, "one", True),
    (32, "ppt", 1, 2, "dup", False),
    (32, "ppt+1", 3, 2, "rev", True),
    (32, 1000, 1, 1, "one", True),
    (32, 4096, 1, 1, "one", False),
    (33, "ppt", 1, 1, "one", True),
    (33, "ppt+1", 1, 2, "rev", False),
    (255, "ppt", 3, 1, "one", True),
    (255, "ppt+1", 1, 2, "dup", False),
    (256, "ppt", 1, 1, "one", False),
    (256, "ppt+1", 1, 1, "one", True),
    (257, 1, 1, 1, "one", False),
    (257, 2, 3, 1, "one", True),
    (1024, 2, 1, 2, "rev", True),
]


def make_case(ci):
    beams, k, a, m, ids, weighted = CASES[ci]
    if isinstance(k, str):
        k = ppt_of(beams) + {"ppt-1": -1, "ppt": 0, "ppt+1": 1}[k]
    if m == "ragged":
        m = ragged_m(a)
    rng = np.random.default_rng(100 + ci)
    poses = rng.uniform(0, SIDE, (m, a, k, 2)).astype(F)
    weight = None
    if weighted:
        weight = rng.random((m, k)).astype(F)
        weight[:, 0] = 1.0
        weight[:, 1:][rng.random((m, k - 1)) < 0.2] = 0.0
        weight[:, k // 2] = F(0.5)  # (K = 1: the one weight)
    map_ids = dict(one=None, none=None, rev=np.arange(m)[::-1] % 4, dup=rng.integers(0, 4, m))[ids]
    maps = rooms24()[2:3] if ids == "one" else rooms24()
    assert ids != "none" or m == len(maps)
    return beams, k, a, m, maps, poses, weight, map_ids


def run(gpu, maps, poses, weight, map_ids, beams, lidar_range=RANGE, mean=True, width=None, use_err=True):
    """lidar_scan_spread, and the restatement on lidar_scan_poses' scans of the same poses: (result, error word,
    restatement)."""
    import torch

    import ap_gym_amd as ap

    m, a, k = poses.shape[:3]
    width = maps.shape[2] if width is None else width
    bits, poses_t = dev_bits(maps, gpu), dev(poses, gpu)
    ids_t = None if map_ids is None else dev(np.asarray(map_ids, np.int64), gpu)
    weight_t = None if weight is None else dev(weight, gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu) if use_err else None
    res = ap.lidar_scan_spread(bits, width, poses_t, weight_t, ids_t, beams=beams, lidar_range=lidar_range, mean=mean,
                               err=err)
    scans = ap.lidar_scan_poses(bits, width, poses_t.view(m, a * k, 2), ids_t, beams=beams, lidar_range=lidar_range)
    want = scan_spread_np(host(scans).reshape(m, a, k, beams), weight)
    return res, (int(err.item()) if use_err else None), want


# ------------------------------------------------------------------ 1: bit for bit against the restatement
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_spread_and_mean_equal_the_restatement_bit_for_bit(gpu, ci):
    beams, k, a, m, maps, poses, weight, map_ids = make_case(ci)
    res, err, want = run(gpu, maps, poses, weight, map_ids, beams)
    assert res.spread.shape == (m, a) and res.mean.shape == (m, a, beams)
    assert same_values(res.spread, want["spread"]), CASES[ci]
    assert same_values(res.mean, want["mean"]), CASES[ci]
    assert err == 0 and want["err"] == 0
    assert not np.isnan(want["spread"]).any() and (k == 1 or (want["spread"] > 0).any())
    if k == 1:
        assert (want["spread"] == 0).all()


@pytest.mark.parametrize("mi", range(5))
def test_spread_equals_the_restatement_on_the_reference_models_scans(gpu, mi):
    """The pose group of tests/golden/lidar_scan_wide.npz as two candidates of K / 2 hypotheses each, uniform weights:
    the restatement is fed the reference's own scans over the GEOS model (the fixture's distances), not the kernel's
    or the oracle's."""
    import torch

    import ap_gym_amd as ap

    g = scan_wide()
    m, dist = g.maps[mi], g.pose_distance[mi]
    (k, beams), w = dist.shape, m.shape[1]
    assert k % 2 == 0 and k // 2 <= 4096 and beams <= 1024
    poses = g.poses[mi].reshape(1, 2, k // 2, 2).copy()  # (the shared fixture arrays are read-only)
    weight = np.full((1, k // 2), 0.5, F)
    want = scan_spread_np(normalize_np(dist, g.pose_range).reshape(1, 2, k // 2, beams), weight)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    res = ap.lidar_scan_spread(dev_bits(m[None], gpu), w, dev(poses, gpu), dev(weight, gpu), beams=beams,
                               lidar_range=g.pose_range, mean=True, err=err, beam_dirs=dev(g.dirs[mi].copy(), gpu))
    assert same_values(res.spread, want["spread"]) and same_values(res.mean, want["mean"])
    assert int(err.item()) == 0 and want["err"] == 0 and (want["spread"] > 0).all()


def test_spread_alone_and_into_out(gpu):
    import torch

    import ap_gym_amd as ap

    beams, k, a, m, maps, poses, weight, map_ids = make_case(9)
    res, _, want = run(gpu, maps, poses, weight, map_ids, beams, mean=False)
    assert res.mean is None and same_values(res.spread, want["spread"])
    buf = torch.full((m * a + 3,), -7.0, device=gpu)
    out = buf[2:2 + m * a].view(m, a)  # at an odd element offset of its storage
    got = ap.lidar_scan_spread(dev_bits(maps, gpu), SIDE, dev(poses, gpu), dev(weight, gpu),
                               dev(np.asarray(map_ids, np.int64), gpu), beams=beams, lidar_range=RANGE, out=out)
    assert got.spread is out and same_values(out, want["spread"])
    assert (host(buf)[[0, 1, -1]] == -7).all()
    empty = ap.lidar_scan_spread(dev_bits(maps, gpu), SIDE, torch.zeros((0, 2, 3, 2), device=gpu),
                                 map_ids=torch.zeros(0, dtype=torch.int64, device=gpu), beams=beams, lidar_range=RANGE,
                                 mean=True)
    assert empty.spread.shape == (0, 2) and empty.mean.shape == (0, 2, beams)


# ------------------------------------------------------------------ 2: order, weight splitting, identical poses
def test_order_independence_and_weight_splitting(gpu):
    rng = np.random.default_rng(2)
    m, a, k, beams = 2, 2, 37, 7
    maps = rooms24()[:2]
    poses = rng.uniform(0, SIDE, (m, a, k, 2)).astype(F)
    weight = rng.random((m, k)).astype(F)
    weight[:, 5] = 1.0
    base, err, want = run(gpu, maps, poses, weight, None, beams)
    assert err == 0 and same_values(base.spread, want["spread"]) and (host(base.spread) > 0).all()
    perm = rng.permutation(k)
    other, _, _ = run(gpu, maps, poses[:, :, perm], weight[:, perm], None, beams)
    assert same(other.spread, base.spread) and same(other.mean, base.mean)
    split_poses = np.concatenate([poses, poses[:, :, 5:6]], axis=2)  # weight 1 -> two of weight 0.5, same pose
    split_w = np.concatenate([weight, np.full((m, 1), 0.5, F)], axis=1)
    split_w[:, 5] = 0.5
    other, _, _ = run(gpu, maps, split_poses, split_w, None, beams)
    assert same(other.spread, base.spread) and same(other.mean, base.mean)
    # identical poses: no disagreement, whatever the weights; the mean is the quantised scan itself
    one = np.broadcast_to(poses[:, :, :1], poses.shape).copy()
    res, err, want = run(gpu, maps, one, weight, None, beams)
    assert err == 0 and (host(res.spread) == 0).all() and not np.signbit(host(res.spread)).any()
    assert same_values(res.mean, want["mean"])
    import ap_gym_amd as ap

    scan = host(ap.lidar_scan_poses(dev_bits(maps, gpu), SIDE, dev(one[:, :, 0], gpu), beams=beams, lidar_range=RANGE))
    assert np.array_equal(host(res.mean), (np.rint(scan * F(4096)) / 4096).astype(F))


# ------------------------------------------------------------------ 3: the bound of the integer sums
def test_the_largest_sums_stay_exact(gpu):
    """K = 4096 hypotheses of weight 1 that all read 1.0: S0 = 2^36, S1_b = 2^48, S2_b = 2^60, N = 0."""
    import ap_gym_amd as ap

    k, beams = 4096, 4
    empty = np.zeros((1, 8, 8), bool)
    poses = np.full((1, 1, k, 2), 4.0, F)
    res, err, want = run(gpu, empty, poses, None, None, beams, lidar_range=2.0)
    assert want["S2"][0][0] == [1 << 60] * beams and want["S0"][0][0] == 1 << 36 and want["N"][0][0] == 0
    assert err == 0 and host(res.spread)[0, 0] == 0 and (host(res.mean) == 1).all()
    # one wall cell out of the centre's reach, and one pose moved next to it
    walled = empty.copy()
    walled[0, 0, 0] = True
    res, err, want = run(gpu, walled, poses, None, None, beams, lidar_range=2.0)
    assert err == 0 and host(res.spread)[0, 0] == 0 and want["S2"][0][0] == [1 << 60] * beams
    poses[0, 0, 1234] = (1.5, 0.5)
    res, err, want = run(gpu, walled, poses, None, None, beams, lidar_range=2.0)
    assert err == 0 and want["spread"][0, 0] > 0 and want["N"][0][0] > 0
    assert same_values(res.spread, want["spread"]) and same_values(res.mean, want["mean"])
    assert isinstance(res, ap.ScanSpreadResult)


# ------------------------------------------------------------------ 4: the domain
def test_bad_poses_weights_and_map_ids(gpu):
    from ap_gym_amd import _native as N

    rng = np.random.default_rng(4)
    m, a, k, beams = 2, 2, 5, 7
    maps = rooms24()
    poses = rng.uniform(0, SIDE, (m, a, k, 2)).astype(F)
    weight = rng.uniform(0.1, 1, (m, k)).astype(F)
    clean, err, want = run(gpu, maps, poses, weight, [1, 3], beams)
    assert err == 0 and same_values(clean.spread, want["spread"])
    # a non-finite pose drops out of its own (i, c) only
    for value in (np.inf, -np.inf, np.nan):
        p = poses.copy()
        p[0, 1, 2, rng.integers(0, 2)] = value
        res, err, want = run(gpu, maps, p, weight, [1, 3], beams)
        assert err == N.APG_ERR_BAD_POSE and want["err"] == N.APG_ERR_BAD_POSE
        assert same_values(res.spread, want["spread"]) and same_values(res.mean, want["mean"])
        keep = np.ones((m, a), bool)
        keep[0, 1] = False
        assert np.array_equal(host(res.spread)[keep], host(clean.spread)[keep])
        assert host(res.spread)[0, 1] != host(clean.spread)[0, 1]
        left, _, _ = run(gpu, maps, np.delete(p, 2, axis=2), np.delete(weight, 2, axis=1), [1, 3], beams)
        assert host(res.spread)[0, 1] == host(left.spread)[0, 1]  # as if the hypothesis were not there
    # a NaN, negative or > 1 weight is q = 0 and flagged
    for value in (np.nan, -0.25, 1.5, np.inf):
        w = weight.copy()
        w[1, 3] = value
        res, err, want = run(gpu, maps, poses, w, [1, 3], beams)
        assert err == N.APG_ERR_BAD_POSE and want["err"] == N.APG_ERR_BAD_POSE
        assert same_values(res.spread, want["spread"]) and same_values(res.mean, want["mean"])
        assert np.array_equal(host(res.spread)[0], host(clean.spread)[0])
        w[1, 3] = 0.0
        zero, err, _ = run(gpu, maps, poses, w, [1, 3], beams)
        assert err == 0 and same(zero.spread, res.spread)
    # an all-dead set is NaN (weights of exactly 0 are legal: no flag)
    w = weight.copy()
    w[0] = 0.0
    res, err, want = run(gpu, maps, poses, w, [1, 3], beams)
    assert err == 0 and np.isnan(host(res.spread)[0]).all() and np.isnan(host(res.mean)[0]).all()
    assert same_values(res.spread, want["spread"]) and same_values(res.mean, want["mean"])
    # a bad map id: an all-zero map, as lidar_scan_poses scans it, and the flag; err=None is accepted
    for ids in ([1, 4], [-1, 3]):
        res, err, want = run(gpu, maps, poses, weight, ids, beams)
        assert err == N.APG_ERR_INDEX
        assert same_values(res.spread, want["spread"]) and same_values(res.mean, want["mean"])
    res, err, want = run(gpu, maps, poses, weight, [1, 4], beams, use_err=False)
    assert err is None and same_values(res.spread, want["spread"])


# ------------------------------------------------------------------ 5: the env
STATE_KEYS = ("pos", "init_pos", "elapsed", "flags", "rng", "it_rng", "occ", "lidar", "odometry", "time_step", "reward",
              "terminated", "base_reward", "err")


def _env(ap, kind, gpu, backend, n=5):
    kw = dict(num_envs=n, device=gpu, array_backend=backend, lidar_beam_count=8)
    if kind == "bits":
        kw["map_obs"] = "bits"
    return ap.make_vec("LIDARLocRoomsStatic-v0" if kind == "static" else "LIDARLocRooms-v0", **kw)


@pytest.mark.parametrize("kind", ["dense", "bits", "static"])
def test_action_spread_is_move_poses_then_scan_spread(gpu, kind):
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd.map_bits import words_per_row

    env, env_np = _env(ap, kind, gpu, "torch"), _env(ap, kind, gpu, "numpy")
    for e in (env, env_np):
        e.reset(seed=5)
        e.step({"action": np.full((5, 2), 0.5, F), "prediction": np.zeros((5, 2), F)})
    h, w = env.dataset.map_height, env.dataset.map_width
    rng = np.random.default_rng(len(kind))
    k, na = 6, 3
    for ids, t in ((None, 1), (np.array([3, 0, 3, 4]), 2)):
        m = 5 if ids is None else len(ids)
        particles = rng.uniform(0, [w, h], (m, k, 2)).astype(F)
        actions = rng.uniform(-1.2, 1.2, (m, na, t, 2)).astype(F)
        actions[:, 0] = 0
        weight = rng.random((m, k)).astype(F)
        before = {name: host(env._t[name]).copy() for name in STATE_KEYS if name in env._t}
        got = env.action_spread(dev(particles, gpu), dev(actions if t > 1 else actions[:, :, 0], gpu),
                                dev(weight, gpu), ids, mean=True)
        for name, x in before.items():
            assert np.array_equal(host(env._t[name]), x), name
        assert sorted(got) == ["mean", "pos", "spread", "terminated"] and type(got["spread"]) is torch.Tensor
        assert got["terminated"].dtype == torch.bool and got["terminated"].shape == (m, na, k)
        # the same from the public pieces
        static = kind == "static"
        bits = env._t["occ"].view(1 if static else 5, h, words_per_row(w))
        map_ids = None if static or ids is None else dev(ids.astype(np.int64), gpu)
        start = np.broadcast_to(particles[:, None], (m, na, k, 2)).reshape(m, na * k, 2)
        acts = np.broadcast_to(actions[:, :, None], (m, na, k, t, 2)).reshape(m, na * k, t, 2)
        moved = ap.lidar_move_poses(bits, w, dev(start, gpu), dev(acts, gpu), map_ids, base_reward=False)
        pos = moved.pos[:, :, -1].reshape(m, na, k, 2).contiguous()
        want = ap.lidar_scan_spread(bits, w, pos, dev(weight, gpu), map_ids, beams=8, lidar_range=env.lidar_range,
                                    mean=True)
        assert same(got["pos"], pos) and same(got["spread"], want.spread) and same(got["mean"], want.mean)
        assert np.array_equal(host(got["terminated"]), host(moved.terminated).reshape(m, na, k).astype(bool))
        assert (host(got["spread"]) >= 0).all()
        no_mean = env.action_spread(dev(particles, gpu), dev(actions, gpu), None, ids)
        assert sorted(no_mean) == ["pos", "spread", "terminated"]
        # the numpy backend: numpy in, numpy out, the same bits
        got_np = env_np.action_spread(particles, actions, weight, ids, mean=True)
        assert all(type(v) is np.ndarray for v in got_np.values())
        for name in got:
            assert same(got_np[name], got[name]), name
    env.check_errors()
    with pytest.raises(ValueError, match="actions must have shape"):
        env.action_spread(dev(particles, gpu), dev(actions[:2], gpu), None, ids)
    with pytest.raises(IndexError):  # raised at once
        env_np.action_spread(particles[:2], actions[:2], None, [0, 5])
    env.action_spread(dev(particles[:2], gpu), dev(actions[:2], gpu), None, [0, 5])
    with pytest.raises(IndexError):
        env.check_errors()
    env.check_errors()
    env.close()
    env_np.close()


# ------------------------------------------------------------------ 6: the meaning
def test_the_candidate_that_tells_the_hypotheses_apart_wins(gpu):
    import torch

    import ap_gym_amd as ap

    maps = np.zeros((1, 32, 32), bool)
    maps[0, 15:17, 15:17] = True  # one 2 x 2 block
    env = ap.LIDARLocalization2DVectorEnv(num_envs=1, dataset=ap.ArrayFloorMapDataset(maps), lidar_beam_count=8,
                                          lidar_range=2.0, device=gpu, array_backend="torch")
    env.reset(seed=0)
    # both further than 4 cells from the block and from the border
    particles = np.array([[[10.5, 15.5], [24.5, 24.5]]], F)
    # four unit steps each: stay; east (the first particle ends half a cell from the block); north (nothing in reach)
    cands = np.zeros((1, 3, 4, 2), F)
    cands[0, 1, :, 0] = 1.0
    cands[0, 2, :, 1] = 1.0
    res = env.action_spread(dev(particles, gpu), dev(cands, gpu))
    spread = host(res["spread"])[0]
    assert np.array_equal(host(res["pos"])[0, 1], F([[14.5, 15.5], [28.5, 24.5]])) and not host(res["terminated"]).any()
    assert spread[0] == 0 and spread[2] == 0 and spread[1] > 0
    pf = ap.LidarParticleFilter(env, 2, sigma=0.1)
    pf.reset(particles)
    action, sp = pf.choose_action(dev(cands, gpu))
    assert action.shape == (1, 2) and np.array_equal(host(action), F([[1, 0]])) and same(sp, res["spread"])
    assert same(pf.action_spread(dev(cands, gpu))["spread"], res["spread"])
    # a candidate whose every hypothesis is dead (NaN spread) never wins; single-step candidates are [N, A, 2]
    pf.logw = torch.tensor([[0.0, -np.inf]], device=gpu)
    action, sp = pf.choose_action(dev(cands[:, :, 0], gpu))
    assert (host(sp) == 0).all() and np.array_equal(host(action), F([[0, 0]]))  # one live hypothesis: no disagreement
    bad = cands.copy()
    bad[0, 1, 0, 0] = np.nan  # every particle's pose under candidate 1 is NaN
    pf.logw = torch.zeros((1, 2), device=gpu)
    action, sp = pf.choose_action(dev(bad, gpu))
    assert np.isnan(host(sp)[0, 1]) and np.array_equal(host(action), F([[0, 0]]))
    with pytest.raises(ValueError):
        env.check_errors()
    env.close()


# ------------------------------------------------------------------ 7: graph capture
def test_graph_capture_and_replay(gpu):
    import torch

    import ap_gym_amd as ap

    beams, k, a, m, maps, poses, weight, map_ids = make_case(9)
    bits, poses_t, weight_t = dev_bits(maps, gpu), dev(poses, gpu), dev(weight, gpu)
    ids_t = dev(np.asarray(map_ids, np.int64), gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    kw = dict(beams=beams, lidar_range=RANGE, mean=True, err=err)
    ap.lidar_scan_spread(bits, SIDE, poses_t, weight_t, ids_t, **kw)  # (loads the op and the directions first)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        res = ap.lidar_scan_spread(bits, SIDE, poses_t, weight_t, ids_t, **kw)
    torch.cuda.current_stream(gpu).wait_stream(side)
    rng = np.random.default_rng(70)
    poses_t.copy_(dev(rng.uniform(0, SIDE, poses.shape).astype(F), gpu))
    weight_t.copy_(dev(rng.random(weight.shape).astype(F), gpu))
    graph.replay()
    eager = ap.lidar_scan_spread(bits, SIDE, poses_t, weight_t, ids_t, **kw)
    assert same(res.spread, eager.spread) and same(res.mean, eager.mean)
    assert int(err.item()) == 0
