"""lidar_move_poses: what needs no GPU -- the numpy float32 restatement of the candidate-action rollout over the
oracle's segment scan that tests/test_gpu_move_poses.py compares the kernel with (itself checked here, bit for bit,
against oracle envs that are actually stepped with the candidates' actions), the argument checks of the public
function, the C ABI's host-side validation (it returns before any HIP call) and the ctypes layout of its struct."""

import ctypes

import numpy as np
import pytest

F = np.float32
EPS = F(1e-5)


def _norm(x, y):
    """numpy's norm of a float32 2-vector: float32 products, float32 sum, float32 square root."""
    return np.sqrt(F(F(x * x) + F(y * y)))


def move_one_np(oracle, occ, px, py, ax, ay):
    """One action (float32 scalars) applied to a pose on the map occ (uint8 [H, W]): step_one's movement of
    oracle/apg_oracle_lidar.c (lidar_localization2d.py:330-364) up to, not including, the clip.  Returns (x, y,
    base_reward, hit a wall, slid, slid along candidate 1)."""
    br = F(F(0.1) - F(F(0.001) * F(F(ax * ax) + F(ay * ay))))
    mag = _norm(ax, ay)
    if mag > F(1):
        ax, ay = F(ax / mag), F(ay / mag)
    tx, ty = F(px + ax), F(py + ay)
    dx, dy = F(tx - px), F(ty - py)
    total = _norm(dx, dy)
    hit = slid = second = False
    if total > F(0):
        dx, dy = F(dx / total), F(dy / total)
        d = F(oracle.lidar_scan(occ, (px, py), (tx, ty))[0])
        px, py = F(px + F(dx * d)), F(py + F(dy * d))
        rem = F(total - d)
        if rem > EPS:
            hit = True
            kept = [v for v in (F(dx * rem), F(dy * rem)) if v > EPS]
            if kept:  # eye(2) * kept: with one kept component both candidates use it
                slid = True
                c0, c1 = (kept[0], F(0)), (F(0), kept[-1])
                d0 = F(oracle.lidar_scan(occ, (px, py), (F(px + c0[0]), F(py + c0[1])))[0])
                d1 = F(oracle.lidar_scan(occ, (px, py), (F(px + c1[0]), F(py + c1[1])))[0])
                second = not d0 > F(0)
                (cx, cy), dd = (c1, d1) if second else (c0, d0)
                nrm = _norm(cx, cy)
                px, py = F(px + F(F(cx / nrm) * dd)), F(py + F(F(cy / nrm) * dd))
    return px, py, br, hit, slid, second


def move_poses_np(oracle, maps, poses, actions, map_ids=None, max_steps=None, origin=None, origin_alias=None):
    """numpy restatement of apg_lidar_move_poses.  maps: bool / uint8 [n_src, H, W]; poses float32 [M, K, 2]; actions
    float32 [M, K, T, 2]; max_steps int [M] (<= 0: no limit); origin float32 [M, 2]; origin_alias [M].  Returns a
    dict of pos [M, K, T, 2], steps [M, K], terminated [M, K], base_reward [M, K, T], odometry [M, K, T, 2] (None
    without origin) and `stats`: counts of applied actions, wall hits, slides, slides along candidate 1, exits."""
    maps = np.asarray(maps).astype(np.uint8)
    poses = np.asarray(poses, dtype=F)
    actions = np.asarray(actions, dtype=F)
    n_src, h, w = maps.shape
    m, k, t_n, _ = actions.shape
    ids = (np.zeros(m, np.int64) if n_src == 1 else np.arange(m)) if map_ids is None else np.asarray(map_ids)
    empty = np.zeros((h, w), np.uint8)
    mw, mh = F(w), F(h)
    pos = np.zeros((m, k, t_n, 2), F)
    steps = np.zeros((m, k), np.int32)
    term = np.zeros((m, k), np.uint8)
    br = np.zeros((m, k, t_n), F)
    odo = np.zeros((m, k, t_n, 2), F) if origin is not None else None
    stats = dict(applied=0, hits=0, slides=0, second=0, exits=0)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(m):
            occ = np.ascontiguousarray(maps[ids[i]]) if 0 <= ids[i] < n_src else empty
            limit = 0 if max_steps is None else int(max_steps[i])
            for j in range(k):
                px, py = poses[i, j]
                ox, oy = (F(origin[i][0]), F(origin[i][1])) if origin is not None else (F(0), F(0))
                alias = origin_alias is not None and bool(origin_alias[i])
                bad = not (np.isfinite(px) and np.isfinite(py))
                done = False
                o = (F(0), F(0))
                for t in range(t_n):
                    if not bad and not done:
                        ax, ay = actions[i, j, t]
                        bad = not (np.isfinite(ax) and np.isfinite(ay))
                    if bad:
                        pos[i, j, t] = br[i, j, t] = np.nan
                        if odo is not None:
                            odo[i, j, t] = np.nan
                        continue
                    if not done:
                        px, py, b, hit, slid, second = move_one_np(oracle, occ, px, py, ax, ay)
                        stats["applied"] += 1
                        stats["hits"] += hit
                        stats["slides"] += slid
                        stats["second"] += second
                        if alias and t == 0:  # initial_pos aliases pos until np.clip rebinds it
                            ox, oy = px, py
                        left = bool(px < 0 or py < 0 or px >= mw or py >= mh)
                        stats["exits"] += left
                        px, py = min(max(px, F(0)), mw), min(max(py, F(0)), mh)
                        steps[i, j] = t + 1
                        done = left or (limit > 0 and t + 1 >= limit)
                        term[i, j] = done
                        br[i, j, t] = b
                        # write_obs: (odo - (-max)) / (max - (-max)) * 2 - 1
                        o = (F(F(F(F(F(px - ox) - F(-mw)) / F(mw - F(-mw))) * F(2)) - F(1)),
                             F(F(F(F(F(py - oy) - F(-mh)) / F(mh - F(-mh))) * F(2)) - F(1)))
                    pos[i, j, t] = (px, py)
                    if odo is not None:
                        odo[i, j, t] = o
    return dict(pos=pos, steps=steps, terminated=term, base_reward=br, odometry=odo, stats=stats)


def bits_equal(a, b):
    """float32 arrays equal bit for bit (NaNs of any payload count as equal to each other)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.int32)[~nan],
                                                                                      b.view(np.int32)[~nan])


def open_pool(n, h, w, seed):
    """n maps bool [n, h, w] without border walls and with few wall cells: first moves can leave the map."""
    rng = np.random.default_rng(seed)
    maps = rng.random((n, h, w)) < 0.12
    maps[:, h // 2, w // 2] = False
    return maps


def replay_oracles(oracle_mod, make, seed, history, cand):
    """K + 1 oracle envs made by `make()`, reset with `seed` and stepped through the same `history` [S, N, 2] actions;
    oracle 0 gives the start state, oracle 1 + k is then stepped with candidate k's actions cand[:, k] ([N, K, T, 2]).
    Returns (start: maps, pos, init_pos, elapsed, autoreset; per-step [T][K] records of pos, terminated, base_reward,
    odometry, lidar, each [N, ...])."""
    n, k, t_n, _ = cand.shape
    envs = [make() for _ in range(k + 1)]
    zeros = np.zeros((n, 2), F)
    for e in envs:
        e.reset(seed)
        for a in history:
            e.step(a, zeros)
    st = envs[0].state()
    start = dict(st, maps=(envs[0].map != 0) if envs[0].map is not None else None)
    rec = []
    for t in range(t_n):
        row = []
        for j in range(k):
            e = envs[1 + j]
            e.step(np.ascontiguousarray(cand[:, j, t]), zeros)
            row.append(dict(pos=e.state()["pos"], terminated=e.terminated.copy(), base_reward=e.base_reward.copy(),
                            odometry=e.odometry.copy(), lidar=e.lidar.copy()))
        rec.append(row)
    for e in envs:
        e.close()
    return start, rec


def assert_rollout_equals_oracles(got, start, rec, where=""):
    """`got` (move_poses_np's or the op's outputs as numpy arrays) against the replayed oracles, for the sub-envs
    that were not waiting for an autoreset, each candidate up to its number of applied steps.  Returns how many
    (candidate, step) pairs were compared."""
    n, k, t_n = got["base_reward"].shape
    live = start["autoreset"] == 0
    compared = 0
    for t in range(t_n):
        for j in range(k):
            r = rec[t][j]
            on = live & (got["steps"][:, j] > t)
            last = on & (got["steps"][:, j] == t + 1) & (got["terminated"][:, j] != 0)
            assert bits_equal(got["pos"][on, j, t], r["pos"][on]), (where, t, j)
            assert bits_equal(got["base_reward"][on, j, t], r["base_reward"][on]), (where, t, j)
            assert bits_equal(got["odometry"][on, j, t], r["odometry"][on]), (where, t, j)
            assert np.array_equal(last[on], r["terminated"][on] != 0), (where, t, j)
            if got.get("lidar") is not None:  # [N, K, T, beams]: what step() observes after the action
                assert bits_equal(got["lidar"][on, j, t], r["lidar"][on]), (where, t, j)
            compared += int(on.sum())
    return compared


ORACLE_CASES = {
    "rooms32": dict(kw=dict(map_kind="rooms", size=32), history=4, step_limit=100),
    "maze21": dict(kw=dict(map_kind="maze", size=21), history=4, step_limit=100),
    "rooms32_limit": dict(kw=dict(map_kind="rooms", size=32), history=4, step_limit=6),  # ends inside T
    "maze21_limit": dict(kw=dict(map_kind="maze", size=21), history=2, step_limit=3),
    "open_pool_first": dict(kw=dict(map_kind="pool"), history=0, step_limit=100),  # origin_alias, first-move exits
}


def oracle_case(oracle_mod, name, n=64, k=8, t_n=3, seed=3):
    """The start state, the candidates and the replayed oracles of one case."""
    c = ORACLE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    kw = dict(c["kw"])
    if kw["map_kind"] == "pool":
        kw["pool"] = open_pool(9, 6, 7, seed=2)

    def make():
        return oracle_mod.OracleLidarVectorEnv(n, beams=8, lidar_range=5, step_limit=c["step_limit"], **kw)

    history = rng.uniform(-1.5, 1.5, (c["history"], n, 2)).astype(F)
    cand = rng.uniform(-1.5, 1.5, (n, k, t_n, 2)).astype(F)
    start, rec = replay_oracles(oracle_mod, make, seed, history, cand)
    return c, start, cand, rec


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_restated_move_equals_the_oracle_env(oracle_mod, name):
    c, start, cand, rec = oracle_case(oracle_mod, name)
    n, k, t_n, _ = cand.shape
    poses = np.repeat(start["pos"][:, None, :], k, axis=1)
    got = move_poses_np(oracle_mod, start["maps"], poses, cand, max_steps=c["step_limit"] - start["elapsed"],
                        origin=start["init_pos"], origin_alias=start["elapsed"] == 0)
    compared = assert_rollout_equals_oracles(got, start, rec, name)
    s = got["stats"]
    print(f"{name}: {compared} candidate steps compared, {s['applied']} applied: {s['hits']} hit a wall, "
          f"{s['slides']} slid ({s['second']} along candidate 1), {s['exits']} left the map; "
          f"{int((start['autoreset'] != 0).sum())} sub-envs waited for an autoreset")
    assert compared >= n * k  # the comparison is not vacuous
    live = start["autoreset"] == 0
    if "limit" in name:  # the TimeLimit ends candidates inside T
        left = c["step_limit"] - start["elapsed"][live]
        assert 0 < left.min() < t_n and np.all(got["steps"][live] <= np.minimum(left, t_n)[:, None])
        assert np.all(got["terminated"][live][left <= t_n] == 1)
    elif name == "open_pool_first":
        assert np.all(start["elapsed"] == 0) and s["exits"] > 0
        first_exit = (got["steps"] == 1) & (got["terminated"] == 1)
        assert first_exit.any()
        # the quirk: the origin is the unclipped pose after the first action, so the first odometry is not 0 exactly
        # where the clip moved the pose, and 0 (x and y) where it did not
        stay = got["steps"] > 1
        assert np.all(got["odometry"][stay][:, 0, :] == 0.0) and np.any(got["odometry"][first_exit][:, 0, :] != 0.0)
    else:
        assert s["hits"] > 0 and s["slides"] > 0
    # after termination: the final pose and odometry repeat, the base reward is 0
    for i, j in zip(*np.nonzero(got["steps"] < t_n)):
        sj = got["steps"][i, j]
        assert got["terminated"][i, j] == 1
        assert np.all(got["pos"][i, j, sj:] == got["pos"][i, j, sj - 1])
        assert np.all(got["odometry"][i, j, sj:] == got["odometry"][i, j, sj - 1])
        assert np.all(got["base_reward"][i, j, sj:] == 0.0)


def test_restatement_conventions(oracle_mod):
    """Non-finite poses and actions are NaN from there on, ids outside the batch an empty map, max_steps <= 0 no
    limit, a start pose outside the map ends with its first action."""
    maps = np.zeros((2, 5, 7), bool)
    maps[0, :, 4] = True  # a wall across map 0 at x = 4
    poses = np.array([[[1.5, 2.5], [np.nan, 1.0], [1.5, 2.5], [-2.0, 1.0]]] * 2, F)
    actions = np.zeros((2, 4, 3, 2), F)
    actions[:, :, :, 0] = 1.0  # three steps along +x
    actions[:, 2, 1, 1] = np.inf
    got = move_poses_np(oracle_mod, maps, poses, actions, max_steps=[0, 2])
    assert got["odometry"] is None
    assert np.isnan(got["pos"][:, 1]).all() and np.all(got["steps"][:, 1] == 0) and np.all(got["terminated"][:, 1] == 0)
    assert not np.isnan(got["pos"][:, 2, 0]).any() and np.isnan(got["pos"][:, 2, 1:]).all()
    assert np.isnan(got["base_reward"][:, 2, 1:]).all() and np.all(got["steps"][:, 2] == 1)
    assert np.all(got["steps"][:, 3] == 1) and np.all(got["terminated"][:, 3] == 1)  # from outside: left, clipped
    assert np.all(got["pos"][:, 3, :, 0] == 0.0)
    assert got["steps"][0, 0] == 3 and got["terminated"][0, 0] == 0 and got["pos"][0, 0, -1, 0] < 4  # the wall stops it
    assert got["steps"][1, 0] == 2 and got["terminated"][1, 0] == 1  # map 1 is free; max_steps = 2
    assert np.all(got["pos"][1, 0, :, 0] == [2.5, 3.5, 3.5]) and got["base_reward"][1, 0, 2] == 0.0
    off = move_poses_np(oracle_mod, maps, poses[:1], actions[:1], map_ids=[2])  # an id outside: the empty map
    assert np.all(off["pos"][0, 0, :, 0] == [2.5, 3.5, 4.5])
    assert bits_equal(got["base_reward"][0, 0], np.full(3, F(0.1) - F(0.001), F))


def test_move_poses_argument_checks():
    """Dtype, rank and shape errors come first, on tensors of any device; the device is refused last."""
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    bits = torch.zeros((3, 4, 2), dtype=torch.int64)
    poses = torch.zeros((3, 5, 2))
    actions = torch.zeros((3, 5, 2, 2))

    def bad(exc, match, b=bits, w=70, p=poses, a=actions, ids=None, **kw):
        with pytest.raises(exc, match=match):
            ap.lidar_move_poses(b, w, p, a, ids, **kw)

    bad(TypeError, "int64", b=bits.to(torch.int32))
    bad(TypeError, "int64", b=bits[0])
    bad(TypeError, "int64", b=bits.numpy())
    bad(TypeError, "poses must be a float32", p=poses.double())
    bad(TypeError, "poses must be a float32", p=poses.numpy())
    bad(ValueError, r"\[M, K, 2\]", p=poses[0])
    bad(ValueError, r"\[M, K, 2\]", p=torch.zeros((3, 5, 3)))
    bad(TypeError, "actions must be a float32", a=actions.double())
    bad(TypeError, "actions must be a float32", a=actions.numpy())
    bad(ValueError, r"actions must have shape", a=actions[:, :, 0])
    bad(ValueError, r"actions must have shape", a=torch.zeros((3, 4, 2, 2)))
    bad(ValueError, r"actions must have shape", a=torch.zeros((3, 5, 2, 3)))
    bad(ValueError, "T must be in", a=torch.zeros((3, 5, 0, 2)))
    bad(ValueError, "T must be in", a=torch.zeros((3, 5, N.MOVE_POSES_MAX_T + 1, 2)))
    bad(ValueError, "words per row", w=64)
    bad(ValueError, "1..511", b=torch.zeros((3, 4, 8), dtype=torch.int64), w=512)
    bad(ValueError, "1..511", b=torch.zeros((3, 0, 2), dtype=torch.int64))
    bad(TypeError, "map_ids", ids=torch.zeros(3, dtype=torch.int32))
    bad(TypeError, "map_ids", ids=[0, 1, 2])
    bad(ValueError, "map_ids", ids=torch.zeros(2, dtype=torch.int64))
    bad(ValueError, "without map_ids", p=torch.zeros((2, 5, 2)), a=torch.zeros((2, 5, 2, 2)))
    bad(TypeError, "max_steps", max_steps=torch.zeros(3, dtype=torch.int64))
    bad(ValueError, "max_steps", max_steps=torch.zeros(4, dtype=torch.int32))
    bad(TypeError, "origin", origin=torch.zeros((3, 2), dtype=torch.float64))
    bad(ValueError, "origin", origin=torch.zeros((3, 3)))
    bad(TypeError, "origin_alias", origin=torch.zeros((3, 2)), origin_alias=torch.zeros(3, dtype=torch.bool))
    bad(ValueError, "origin_alias", origin=torch.zeros((3, 2)), origin_alias=torch.zeros(2, dtype=torch.uint8))
    bad(ValueError, "need origin", odometry=True)
    bad(ValueError, "need origin", origin_alias=torch.zeros(3, dtype=torch.uint8))
    # every check above came first: there is no CPU fallback
    bad(ValueError, "GPU")
    bad(ValueError, "GPU", b=bits[:1])  # one map for every candidate set
    bad(ValueError, "GPU", ids=torch.tensor([2, 0, 2]), max_steps=torch.zeros(3, dtype=torch.int32),
        origin=torch.zeros((3, 2)), origin_alias=torch.zeros(3, dtype=torch.uint8), base_reward=False)
    assert (N.MOVE_POSES_TILE, N.MOVE_POSES_SMALL_K, N.MOVE_POSES_MAX_MPW, N.MOVE_POSES_MAX_GRID,
            N.MOVE_POSES_MAX_T) == (256, 128, 32, 8192, 4096)


def test_move_poses_c_abi_validates_on_the_host():
    from ap_gym_amd import _native as N

    fn = N.lib().apg_lidar_move_poses
    buf = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(buf)

    def call(**over):
        a = N.MovePosesArgs(occ=p, map_ids=None, poses=p, actions=p, max_steps=p, origin=p, origin_alias=p, pos=p,
                            steps=p, terminated=p, base_reward=p, odometry=p, err=None, n_src=1, m=1, height=4,
                            width=70, k=1, t=1)
        for name, v in over.items():
            setattr(a, name, v)
        return fn(ctypes.byref(a), None)

    def last():
        return N.lib().apg_last_error().decode()

    for kw, text in ((dict(height=0), "1..511"), (dict(height=512), "1..511"), (dict(width=0), "1..511"),
                     (dict(width=512), "1..511"), (dict(t=0), "t must be"), (dict(t=4097), "t must be"),
                     (dict(m=-1), ">= 0"), (dict(k=-1), ">= 0"), (dict(n_src=-1), ">= 0"),
                     (dict(poses=None), "null occ / poses / actions"),
                     (dict(actions=None), "null occ / poses / actions"),
                     (dict(occ=None), "null occ / poses / actions"), (dict(pos=None), "null pos / steps / terminated"),
                     (dict(steps=None), "null pos / steps / terminated"),
                     (dict(terminated=None), "null pos / steps / terminated"),
                     (dict(origin=None), "odometry needs origin"),
                     (dict(origin=None, odometry=None), "origin_alias needs origin"),
                     (dict(n_src=2, m=3), "without map_ids")):
        assert call(**kw) == N.APG_E_INVALID, kw
        assert text in last() and last().startswith("move_poses:"), (kw, last())
    assert fn(None, None) == N.APG_E_INVALID and "null arguments" in last()
    assert call(m=0) == N.APG_OK and call(k=0) == N.APG_OK  # launches nothing
    assert call(m=0, origin=None) == N.APG_E_INVALID  # ... but is validated first
    assert ctypes.sizeof(N.MovePosesArgs) == 13 * 8 + 2 * 8 + 4 * 4


def test_move_poses_struct_layout_matches_the_c_header(tmp_path):
    """The ctypes mirror of apg_move_poses_args has the size and field offsets gcc gives include/apgym_capi.h."""
    import os
    import shutil
    import subprocess

    from ap_gym_amd import _native as N

    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cname, py = "apg_move_poses_args", N.MovePosesArgs
    lines = ["#include <stdio.h>", "#include \"apgym_capi.h\"", "int main(void) {",
             f'  printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                              text=True).stdout.splitlines())
    assert int(got[cname]) == ctypes.sizeof(py)
    for fname, _ in py._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, fname
