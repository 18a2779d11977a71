"""lidar_move_poses, the kernel k_move_poses (csrc/apg_move_poses.hip) and env.lookahead on the GPU.

The op is compared bit for bit, on every output, with the numpy restatement of tests/test_move_poses_host.py (itself
checked there against oracle envs that are actually stepped) at the smallest shapes that cross each of the kernel's
boundaries; env.lookahead is tied to the product: candidate 0 against what env.step() then really returns, every
candidate against replayed oracle envs, for every map source, both map_obs modes and both backends.
"""

import functools

import numpy as np
import pytest

from test_gpu_scan_poses import dev, dev_bits, make_maps, oracle
from test_move_poses_host import (F, assert_rollout_equals_oracles, bits_equal, move_poses_np, open_pool,
                                  replay_oracles)

pytestmark = pytest.mark.gpu

MAPS = [(1, 1), (5, 7), (21, 21), (32, 32), (9, 64), (6, 65), (4, 130), (40, 511)]
PROCEDURAL = [(21, 21), (32, 32)]
T_MAX = 7
FLOATS = ("pos", "base_reward", "odometry")


def split_of(h, w, k):
    """(sets per workgroup item, M with a ragged last item) of k_move_poses for K = k on h x w maps."""
    from ap_gym_amd import _native as N

    if k > N.MOVE_POSES_SMALL_K:
        return 1, 3
    mpw = max(1, min(N.MOVE_POSES_MAX_MPW, N.MOVE_POSES_TILE // k, 32768 // (8 * h * ((w + 63) // 64))))
    return mpw, 2 * mpw + 1


def k_values():
    from ap_gym_amd import _native as N

    return [1, 5, N.MOVE_POSES_SMALL_K, N.MOVE_POSES_SMALL_K + 1, N.MOVE_POSES_TILE + 1]


@functools.lru_cache(maxsize=None)
def make_case(h, w, k):
    """Inputs of one case (read-only): map ids (any order, duplicates), start poses [M, K, 2] -- uniform in the map,
    and for a quarter of them lattice points, wall-cell centres, border points, points up to 3 cells outside, plus
    (-70, 5) and (1e6, 1e6) -- actions [M, K, T_MAX, 2] -- uniform(-1.5, 1.5), and for a sixth of them the zero action,
    axis-aligned actions in both signs, 1e-6-sized and length-1e3 actions -- step limits (some <= 0: none), odometry
    origins and alias flags."""
    rng = np.random.default_rng(100000 * k + 1000 * h + w)
    maps = make_maps(h, w)
    m = split_of(h, w, k)[1]
    ids = rng.permutation(np.r_[np.arange(m - 1) % len(maps), 0])  # any order, map 0 at least twice
    poses = rng.uniform(0, [w, h], (m, k, 2))
    kind = np.where(rng.random((m, k)) < 0.25, rng.integers(0, 4, (m, k)), -1)
    for i, j in zip(*np.nonzero(kind >= 0)):
        p = poses[i, j]
        if kind[i, j] == 0:  # a lattice point, or on one grid line
            p[:] = np.floor(p) if rng.random() < 0.5 else (np.floor(p[0]), p[1])
        elif kind[i, j] == 1:  # the centre of a wall cell of this set's map
            ys, xs = np.nonzero(maps[ids[i]])
            if len(ys):
                q = int(rng.integers(0, len(ys)))
                p[:] = (xs[q] + 0.5, ys[q] + 0.5)
        elif kind[i, j] == 2:  # on the border
            p[int(rng.integers(0, 2))] = 0.0 if rng.random() < 0.5 else None
            p[:] = (w if np.isnan(p[0]) else p[0], h if np.isnan(p[1]) else p[1])
        else:  # up to 3 cells outside
            c = int(rng.integers(0, 2))
            p[c] = -rng.uniform(0, 3) if rng.random() < 0.5 else (w, h)[c] + rng.uniform(0, 3)
    flat = poses.reshape(-1, 2)
    if len(flat) >= 8:
        flat[len(flat) // 3] = (-70.0, 5.0)
        flat[2 * len(flat) // 3] = (1e6, 1e6)
    actions = rng.uniform(-1.5, 1.5, (m, k, T_MAX, 2))
    akind = np.where(rng.random((m, k, T_MAX)) < 1 / 6, rng.integers(0, 7, (m, k, T_MAX)), -1)
    size = rng.uniform(0.05, 1.5, (m, k, T_MAX))
    table = {0: (0, 0), 1: (1, 0), 2: (-1, 0), 3: (0, 1), 4: (0, -1)}
    for i, j, t in zip(*np.nonzero(akind >= 0)):
        a = actions[i, j, t]
        if akind[i, j, t] in table:
            a[:] = np.array(table[akind[i, j, t]]) * size[i, j, t]
        elif akind[i, j, t] == 5:
            a[:] = a * 1e-6
        else:
            a[:] = a / np.hypot(*a) * 1e3
    out = dict(ids=ids, poses=poses.astype(F), actions=actions.astype(F),
               max_steps=rng.integers(-1, T_MAX + 2, m).astype(np.int32),
               origin=rng.uniform(0, [w, h], (m, 2)).astype(F), alias=rng.integers(0, 2, m).astype(np.uint8))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(h, w, k, t):
    """The restatement's outputs of the case for its first t actions, computed once and shared (read-only)."""
    c = make_case(h, w, k)
    e = move_poses_np(oracle(), make_maps(h, w), c["poses"], c["actions"][:, :, :t], c["ids"], c["max_steps"],
                      c["origin"], c["alias"])
    for v in e.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return e


def run_op(gpu, bits, w, poses, actions, ids=None, max_steps=None, origin=None, alias=None, **kw):
    """lidar_move_poses on numpy inputs; returns (outputs as numpy arrays, error word)."""
    import torch

    import ap_gym_amd as ap

    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    def put(a):  # (a copy: the cases' arrays are read-only)
        return None if a is None else dev(np.array(a), gpu)

    res = ap.lidar_move_poses(bits, w, put(poses), put(actions), put(ids), max_steps=put(max_steps), origin=put(origin),
                              origin_alias=put(alias), err=err, **kw)
    got = {name: None if v is None else v.cpu().numpy() for name, v in res._asdict().items()}
    return got, int(err.item())


def assert_same(got, want, where=""):
    assert got["steps"].dtype == np.int32 and got["terminated"].dtype == np.uint8
    assert np.array_equal(got["steps"], want["steps"]), where
    assert np.array_equal(got["terminated"], want["terminated"]), where
    for name in FLOATS:
        if want[name] is None:
            assert got[name] is None, (where, name)
        else:
            assert got[name].dtype == np.float32 and bits_equal(got[name], want[name]), (where, name)


# ------------------------------------------------------------------ 1: the op against the restatement
@pytest.mark.parametrize("k", k_values())
@pytest.mark.parametrize("h,w", MAPS)
def test_rollouts_match_the_restatement_bit_for_bit(gpu, h, w, k):
    """Every output, the frozen tail after termination included, for T = 1, 2 and 7; garbage in the padding bits."""
    c = make_case(h, w, k)
    bits = dev_bits(make_maps(h, w), gpu, garbage_seed=h + w + k)
    total = dict(applied=0, hits=0, slides=0, second=0, exits=0)
    for t in (1, 2, T_MAX):
        want = expected(h, w, k, t)
        for name, v in want["stats"].items():
            total[name] += v
        got, err = run_op(gpu, bits, w, c["poses"], c["actions"][:, :, :t], c["ids"], c["max_steps"], c["origin"],
                          c["alias"])
        assert got["pos"].shape == c["actions"][:, :, :t].shape and err == 0, t
        assert_same(got, want, (h, w, k, t))
    # the conditions, on the restatement alone: the case cannot pass vacuously
    a = total["applied"]
    print(f"{h}x{w} K={k} M={len(c['ids'])}: {a} applied actions, hits {total['hits'] / a:.1%}, slides "
          f"{total['slides'] / a:.1%} ({total['second']} along candidate 1), exits {total['exits'] / a:.1%}")
    if (h, w) in PROCEDURAL:
        assert total["hits"] >= 0.05 * a and total["slides"] >= 0.03 * a
    elif (h, w) != (1, 1):
        assert total["hits"] >= 0.10 * a and total["slides"] >= 0.05 * a and total["exits"] >= 0.01 * a


def test_some_slide_takes_the_second_candidate(gpu):
    """d0 == 0: the slide goes along candidate 1 (the cases above compare those moves too)."""
    assert expected(21, 21, 5, T_MAX)["stats"]["second"] > 0 and expected(6, 65, 5, T_MAX)["stats"]["second"] > 0


def test_optional_arguments_and_shared_maps(gpu):
    """No ids with a map per set and with one map for every set; no limits, no origin (no odometry), no base reward."""
    h, w, k = 6, 65, 5
    maps = make_maps(h, w)
    c = make_case(h, w, k)
    poses, actions = c["poses"][:4], c["actions"][:4, :, :3]
    bits = dev_bits(maps, gpu, garbage_seed=3)
    got, err = run_op(gpu, bits, w, poses, actions)
    want = move_poses_np(oracle(), maps, poses, actions)
    assert err == 0 and got["odometry"] is None
    assert_same(got, want, "a map per set")
    got, err = run_op(gpu, bits[2:3].contiguous(), w, poses, actions, max_steps=c["max_steps"][:4], base_reward=False)
    want = dict(move_poses_np(oracle(), maps[2:3], poses, actions, max_steps=c["max_steps"][:4]), base_reward=None)
    assert err == 0
    assert_same(got, want, "one map for every set")
    got, err = run_op(gpu, bits, w, poses, actions, origin=c["origin"][:4])  # origin without alias flags
    assert_same(got, move_poses_np(oracle(), maps, poses, actions, origin=c["origin"][:4]), "origin only")
    got, err = run_op(gpu, bits, w, poses, actions, origin=c["origin"][:4], odometry=False)
    assert got["odometry"] is None


# ------------------------------------------------------------------ 2: the grid cap
def test_more_items_than_the_grid_holds(gpu):
    """K = 1 on 3 x 3 maps with M three more than the grid cap times the sets per item, and one set of five more
    candidates than the grid cap times a tile: the workgroups take several items each, the last one ragged.  Expected
    values come from a table of the distinct (map, pose, action) moves."""
    from ap_gym_amd import _native as N

    o, rng = oracle(), np.random.default_rng(12)
    maps = rng.random((6, 3, 3)) < 0.3
    poses = rng.uniform(-0.5, 3.5, (24, 2)).astype(F)
    acts = rng.uniform(-1.5, 1.5, (8, 2)).astype(F)
    grid_p = np.repeat(poses[None, :, None, :], 8, axis=2).reshape(1, -1, 2)  # [1, 24 * 8, 2]
    grid_a = np.tile(acts[None, None], (1, 24, 1, 1)).reshape(1, -1, 1, 2)
    table = [move_poses_np(o, maps[i:i + 1], grid_p, grid_a) for i in range(6)]
    bits = dev_bits(maps, gpu, garbage_seed=1)
    grid = N.MOVE_POSES_MAX_GRID
    for m, k in ((grid * N.MOVE_POSES_MAX_MPW + 3, 1), (1, grid * N.MOVE_POSES_TILE + 5)):
        ids = rng.integers(0, 6, m)
        pi, ai = rng.integers(0, 24, (m, k)), rng.integers(0, 8, (m, k))
        got, err = run_op(gpu, bits, 3, poses[pi], acts[ai][:, :, None, :], ids)
        assert err == 0
        for name in ("pos", "steps", "terminated", "base_reward"):
            want = np.stack([t[name][0] for t in table])[ids[:, None], pi * 8 + ai]
            assert np.array_equal(got[name].view(np.int32) if name in FLOATS else got[name],
                                  want.view(np.int32) if name in FLOATS else want), (m, k, name)


# ------------------------------------------------------------------ 3: the input domain
def test_non_finite_poses_and_actions_are_nan_from_there_on(gpu):
    from ap_gym_amd import _native as N

    h, w, k = 9, 64, 5
    maps, c = make_maps(h, w), make_case(h, w, k)
    bits = dev_bits(maps, gpu)
    args = (c["ids"], c["max_steps"] * 0, c["origin"], c["alias"])
    clean = expected(h, w, k, T_MAX)
    for value in (np.nan, np.inf, -np.inf):
        poses, actions = c["poses"].copy(), c["actions"].copy()
        poses[1, 2, 0] = value  # from the start
        poses[3, 0, 1] = value
        actions[0, 1, 0, 1] = value  # the first action
        actions[2, 4, 3, 0] = value  # a later one
        actions[4, 3, T_MAX - 1, 1] = value  # the last one
        got, err = run_op(gpu, bits, w, poses, actions, *args)
        want = move_poses_np(oracle(), maps, poses, actions, *args)
        assert err == N.APG_ERR_BAD_POSE, value
        assert_same(got, want, value)
        for (i, j), first in {(1, 2): 0, (3, 0): 0, (0, 1): 0, (2, 4): 3, (4, 3): T_MAX - 1}.items():
            if not np.isnan(want["pos"][i, j, first]).all():
                continue  # (terminated before the bad action: it is never read)
            assert got["steps"][i, j] == first and got["terminated"][i, j] == 0, (value, i, j)
            for name in FLOATS:
                assert np.isnan(got[name][i, j, first:]).all() and not np.isnan(got[name][i, j, :first]).any()
    got, err = run_op(gpu, bits, w, c["poses"], c["actions"], *args)  # the same launch shape without them: clean
    assert err == 0 and not any(np.isnan(got[name]).any() for name in FLOATS)
    assert bits_equal(got["pos"][:, :, 0], clean["pos"][:, :, 0])  # (no limits here: only the first step is shared)


def test_map_ids_out_of_range_move_on_an_empty_map(gpu):
    from ap_gym_amd import _native as N

    h, w, k = 6, 65, 5
    maps, c = make_maps(h, w), make_case(h, w, k)
    poses, actions = c["poses"][:4], c["actions"][:4, :, :2]
    bits = dev_bits(maps, gpu, garbage_seed=9)
    bad = np.array([0, -1, 2, 4])
    got, err = run_op(gpu, bits, w, poses, actions, bad)
    want = move_poses_np(oracle(), maps, poses, actions, bad)
    assert err == N.APG_ERR_INDEX
    assert_same(got, want)
    free = move_poses_np(oracle(), np.zeros((1, h, w), bool), poses[[1, 3]], actions[[1, 3]])
    assert bits_equal(got["pos"][[1, 3]], free["pos"])
    import ap_gym_amd as ap

    ap.lidar_move_poses(bits, w, dev(np.array(poses), gpu), dev(np.array(actions), gpu), dev(bad, gpu))  # no error word


def test_empty_queries_launch_nothing(gpu):
    import torch

    import ap_gym_amd as ap

    bits = dev_bits(make_maps(5, 7), gpu)
    r = ap.lidar_move_poses(bits, 7, torch.zeros((4, 0, 2), device=gpu), torch.zeros((4, 0, 3, 2), device=gpu))
    assert r.pos.shape == (4, 0, 3, 2) and r.steps.shape == (4, 0) and r.base_reward.shape == (4, 0, 3)
    none = torch.zeros(0, dtype=torch.int64, device=gpu)
    r = ap.lidar_move_poses(bits, 7, torch.zeros((0, 2, 2), device=gpu), torch.zeros((0, 2, 3, 2), device=gpu), none,
                            origin=torch.zeros((0, 2), device=gpu))
    assert r.pos.shape == (0, 2, 3, 2) and r.odometry.shape == (0, 2, 3, 2) and r.terminated.shape == (0, 2)


# ------------------------------------------------------------------ 4: env.lookahead
def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


N_ENVS, K_CAND, T_CAND, BEAMS = 64, 5, 3, 8
ENV_KINDS = ["rooms", "maze", "pool", "static", "bits"]


def _pool():
    return open_pool(9, 6, 7, seed=2)


def _make_env(ap, kind, gpu, backend, step_limit):
    kw = dict(num_envs=N_ENVS, device=gpu, array_backend=backend, lidar_beam_count=BEAMS, max_episode_steps=step_limit)
    if kind == "pool":
        return ap.LIDARLocalization2DVectorEnv(dataset=ap.ArrayFloorMapDataset(_pool()), **kw)
    if kind == "bits":
        kw["map_obs"] = "bits"
    return ap.make_vec({"rooms": "LIDARLocRooms-v0", "bits": "LIDARLocRooms-v0", "maze": "LIDARLocMaze-v0",
                        "static": "LIDARLocRoomsStatic-v0"}[kind], **kw)


def _make_oracle(o, kind, step_limit):
    kw = dict(beams=BEAMS, lidar_range=5, step_limit=step_limit)
    if kind == "pool":
        return o.OracleLidarVectorEnv(N_ENVS, map_kind="pool", pool=_pool(), **kw)
    if kind == "maze":
        return o.OracleLidarVectorEnv(N_ENVS, map_kind="maze", size=21, **kw)
    return o.OracleLidarVectorEnv(N_ENVS, map_kind="rooms", size=32, static_map=kind == "static", **kw)


STATE_KEYS = ("pos", "init_pos", "elapsed", "flags", "rng", "it_rng", "occ", "lidar", "odometry", "time_step", "reward",
              "terminated", "base_reward", "err")


@pytest.mark.parametrize("backend", ["torch", "numpy"])
@pytest.mark.parametrize("step_limit", [100, 3])
@pytest.mark.parametrize("kind", ENV_KINDS)
def test_lookahead_is_what_step_then_does(gpu, oracle_mod, kind, step_limit, backend):
    import ap_gym_amd as ap

    env = _make_env(ap, kind, gpu, backend, step_limit)
    h, w = env.dataset.map_height, env.dataset.map_width
    wpr = (w + 63) // 64
    rng = np.random.default_rng(len(kind) + step_limit)
    seed, n, zeros = 23, N_ENVS, np.zeros((N_ENVS, 2), F)
    history = []

    def give(a):  # the backend's array type
        return a if backend == "numpy" else dev(a, gpu)

    def checkpoint(where):
        cand = rng.uniform(-1.5, 1.5, (n, K_CAND, T_CAND, 2)).astype(F)
        before = {name: env._t[name].clone() for name in STATE_KEYS}
        look = env.lookahead(give(cand), scans="all")
        again = env.lookahead(give(cand), scans="all")
        for name in STATE_KEYS:  # untouched
            assert (env._t[name] == before[name]).all(), (where, name)
        assert type(look["pos"]) is (np.ndarray if backend == "numpy" else type(env._t["pos"]))
        got = {name: host(v) for name, v in look.items()}
        for name, v in again.items():  # a second identical call: identical results
            assert np.array_equal(got[name], host(v), equal_nan=True), (where, name)
        assert got["lidar"].shape == (n, K_CAND, T_CAND, BEAMS) and got["pending_reset"].dtype == bool
        assert got["terminated"].dtype == bool and got["steps"].dtype == np.int32
        last = host(env.lookahead(give(cand))["lidar"])  # scans="last"
        assert np.array_equal(last.view(np.int32), got["lidar"][:, :, -1].view(np.int32)), where
        assert "lidar" not in env.lookahead(give(cand), scans=None)
        one = env.lookahead(give(cand[:, :, 0]), scans=None)  # [M, K, 2]: T = 1
        assert host(one["pos"]).shape == (n, K_CAND, 1, 2)
        assert np.array_equal(host(one["pos"])[:, :, 0].view(np.int32), got["pos"][:, :, 0].view(np.int32)), where
        # every candidate against K oracle envs replayed through the same history
        start, rec = replay_oracles(oracle_mod, lambda: _make_oracle(oracle_mod, kind, step_limit), seed,
                                    history, cand)
        pending = got["pending_reset"]
        assert np.array_equal(pending, start["autoreset"] != 0), where
        compared = assert_rollout_equals_oracles(got, start, rec, where)
        # every sub-env, the pending ones on their old map, against the restatement
        rows = env._t["occ"].view(-1, h, wpr).cpu().numpy().view(np.uint64)
        maps = np.unpackbits(rows.view(np.uint8).reshape(len(rows), h, -1), axis=-1, bitorder="little")[..., :w]
        st = {name: env._t[name].cpu().numpy() for name in ("pos", "init_pos", "elapsed", "flags")}
        want = move_poses_np(oracle_mod, maps, np.repeat(st["pos"][:, None], K_CAND, axis=1), cand,
                             None, step_limit - st["elapsed"], st["init_pos"], (st["flags"] & 4) != 0)
        assert np.array_equal(got["steps"], want["steps"]), where
        assert np.array_equal(got["terminated"], want["terminated"] != 0), where
        for name in FLOATS:
            assert bits_equal(got[name], want[name]), (where, name)
        # env_ids: a subset, any order, duplicates
        ids = np.array([n - 1, 0, 2, n - 1, 7])
        sub = env.lookahead(give(cand[ids]), ids, scans="all")
        for name in got:
            assert np.array_equal(host(sub[name]), got[name][ids], equal_nan=True), (where, name)
        # candidate 0, applied: what step() really returns, up to each sub-env's termination
        alive = ~pending
        stepped = 0
        for t in range(T_CAND):
            a = np.ascontiguousarray(cand[:, 0, t])
            obs, _, term, _, _ = env.step({"action": give(a), "prediction": give(zeros)})
            history.append(a)
            on = alive & (got["steps"][:, 0] > t)
            ends = on & (got["steps"][:, 0] == t + 1) & got["terminated"][:, 0]
            assert bits_equal(host(obs["lidar"])[on], got["lidar"][on, 0, t]), (where, t)
            assert bits_equal(host(obs["odometry"])[on], got["odometry"][on, 0, t]), (where, t)
            assert bits_equal(env._t["base_reward"].cpu().numpy()[on], got["base_reward"][on, 0, t]), (where, t)
            assert np.array_equal(host(term)[on], ends[on]), (where, t)
            assert bits_equal(env._t["pos"].cpu().numpy()[on], got["pos"][on, 0, t]), (where, t)
            stepped += int(on.sum())
            alive &= ~host(term).astype(bool)
        print(f"{kind} limit {step_limit} {backend} {where}: {int(pending.sum())} pending resets, {compared} candidate "
              f"steps against oracles, {stepped} against step(), {want['stats']['hits']} wall hits, "
              f"{want['stats']['exits']} exits, {int(got['terminated'].sum())} candidates terminated")
        return pending, compared, stepped

    env.reset(seed=seed)
    pending, compared, stepped = checkpoint("after reset")
    assert not pending.any() and compared >= n * K_CAND and stepped >= n
    pending, compared, stepped = checkpoint("after three steps")
    if step_limit == 3:
        # every episode that ran its three steps has ended (on the open pool maps some left the map earlier and
        # have begun a new one): those rollouts start on the old maps, and step() autoresets
        assert pending.sum() >= n // 2 and (pending.all() or kind == "pool")
        assert (compared, stepped) == (0, 0) or not pending.all()
        pending, compared, stepped = checkpoint("after the autoreset and two steps")
        assert not pending.all()
    assert compared >= n and stepped >= n // 2
    env.check_errors()
    env.close()


def test_lookahead_errors(gpu):
    import torch

    import ap_gym_amd as ap

    env = ap.make_vec("LIDARLocRooms-v0", num_envs=4, device=gpu, array_backend="torch")
    env.reset(seed=1)
    a = torch.zeros((2, 3, 2, 2), device=gpu)
    res = env.lookahead(a, [0, 4])  # an id out of range: an empty map, raised lazily
    assert res["pos"].shape == (2, 3, 2, 2)
    with pytest.raises(IndexError):
        env.check_errors()
    env.check_errors()  # raised once, then clear
    bad = torch.zeros((4, 3, 2, 2), device=gpu)
    bad[1, 2, 1, 0] = float("nan")
    res = env.lookahead(bad)
    assert torch.isnan(res["pos"][1, 2, 1:]).all() and not torch.isnan(res["pos"][1, 2, 0]).any()
    assert torch.isnan(res["lidar"][1, 2]).all() and int(res["steps"][1, 2]) == 1
    with pytest.raises(ValueError, match="pose"):
        env.check_errors()
    with pytest.raises(ValueError, match="actions must have shape"):
        env.lookahead(torch.zeros((4, 3, 2, 3), device=gpu))
    with pytest.raises(ValueError, match="one candidate set per chosen sub-env"):
        env.lookahead(torch.zeros((3, 3, 2, 2), device=gpu))
    with pytest.raises(ValueError, match="scans"):
        env.lookahead(torch.zeros((4, 3, 2, 2), device=gpu), scans="first")
    env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.lookahead(torch.zeros((4, 3, 2, 2), device=gpu))
    static = ap.make_vec("LIDARLocRoomsStatic-v0", num_envs=4, device=gpu)  # numpy backend: at once
    static.reset(seed=1)
    with pytest.raises(IndexError):
        static.lookahead(np.zeros((2, 3, 2, 2), F), [0, 4])
    with pytest.raises(ValueError, match="pose"):
        static.lookahead(bad.cpu().numpy())
    static.close()
