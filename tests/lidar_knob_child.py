"""Child process of tests/test_gpu_lidar_knobs.py: runs every case of CASES with the numpy backend under
whatever APG_* tuning knobs its environment sets (the library reads them once per process) and saves every
output of every step, and the envs-per-workgroup value the step launcher reports, to the .npz named by argv[1].
The parent imports CASES / make_pool / inputs from here, runs the oracle on the same inputs and compares; this
file does not import the oracle.

Every case has N = 300 envs: one full 256-env workgroup plus 44 envs (APG_STEP_EPB=256) or four full 64-env
workgroups plus 44."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_ENVS = 300
SEED = 31
STAT_KEYS = ("avg_euclidean_distance", "avg_mse", "final_euclidean_distance", "final_mse")

# kind, size: the dataset; the rest are LIDARLocalization2DVectorEnv / OracleLidarVectorEnv parameters
CASES = {
    # fused GEN_ROOMS, staged lidar rows, 16-byte lidar stores, ActiveRegressionLogWrapper stats
    "rooms32_b32_stats": dict(kind="rooms", size=32, beams=32, log_stats=True),
    # sparse outputs (weight, NaN rewards of overflowing losses)
    "rooms32_b8_sparse": dict(kind="rooms", size=32, beams=8, sparse=True),
    # fused GEN_POOL, H != W, two words per row, 10-row beam boxes (the 4-row table's middle-row loop)
    "pool40x70_b16_r8": dict(kind="pool", size=0, beams=16, lidar_range=8.0),
    # GEN_NONE, beams % 4 != 0: the scalar lidar store loop
    "rooms32_static_b6": dict(kind="rooms", size=32, beams=6, static=True),
    # more than 64 beams: the instance without staged rows
    "rooms32_b72": dict(kind="rooms", size=32, beams=72),
    # max_rooms > 17: k_lidar_reset, then the unfused step
    "rooms64_mr24_b16": dict(kind="rooms", size=64, beams=16, max_rooms=24),
    # GEN_PF: the maze prefetch kernels at a ragged count, many autoresets
    "maze21_b8_limit7": dict(kind="maze", size=21, beams=8, step_limit=7, steps=40),
    # packed output rows (ROWP)
    "rooms32_b16_packed": dict(kind="rooms", size=32, beams=16, packed=True),
}
DEFAULTS = dict(static=False, lidar_range=5.0, step_limit=100, steps=110, log_stats=False, sparse=False,
                max_rooms=10, packed=False)


def case_params(name: str) -> dict:
    return {**DEFAULTS, **CASES[name]}


def make_pool() -> np.ndarray:
    from test_gpu_lidar_pool import random_pool

    return random_pool(23, 40, 70, SEED)


def inputs(name: str):
    """(actions, predictions), float32 [steps, N, 2]."""
    c = case_params(name)
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    a = rng.uniform(-1.5, 1.5, (c["steps"], N_ENVS, 2)).astype(np.float32)
    p = rng.uniform(-1, 1, (c["steps"], N_ENVS, 2)).astype(np.float32)
    if c["sparse"]:  # a few overflowing losses: inf * weight 0 is NaN in the sparse reward
        p[rng.random((c["steps"], N_ENVS)) < 0.01] = np.float32(3e19)
    return a, p


def run_case(ap, name: str) -> dict:
    c = case_params(name)
    n = N_ENVS
    if c["kind"] == "pool":
        ds = ap.ArrayFloorMapDataset(make_pool())
    elif c["kind"] == "rooms":
        ds = ap.FloorMapDatasetRooms(c["size"], c["size"], max_rooms=c["max_rooms"])
    else:
        ds = ap.FloorMapDatasetMaze(c["size"], c["size"])
    env = ap.LIDARLocalization2DVectorEnv(num_envs=n, dataset=ds, static_map=c["static"], lidar_beam_count=c["beams"],
                                          lidar_range=c["lidar_range"], max_episode_steps=c["step_limit"],
                                          device="cuda:0", log_stats=c["log_stats"], sparse=c["sparse"],
                                          sparse_reset_info=c["sparse"], packed_outputs=c["packed"])
    assert (env.output_rows is not None) == c["packed"]
    out = {}
    obs, info = env.reset(seed=SEED)
    out["reset_lidar"], out["reset_odometry"], out["reset_time_step"] = obs["lidar"], obs["odometry"], obs["time_step"]
    out["reset_map_idx"] = info["map_idx"]
    if not c["static"]:
        out["reset_map"] = np.packbits(obs["map"][..., 0] > 0, axis=-1)
        assert set(np.unique(obs["map"])) <= {np.float32(0), np.float32(1) / np.float32(255)}
    names = ["lidar", "odometry", "time_step", "reward", "terminated", "truncated", "info_mask", "base_reward",
             "target", "loss", "map_idx", "map_idx_mask"]
    names += ["map"] if not c["static"] else []
    names += ["weight"] if c["sparse"] else []
    names += ["stats_mask", "stats_len"] + ["stats_" + k for k in STAT_KEYS] if c["log_stats"] else []
    rec = {k: [] for k in names}
    vec = {"euclidean_distance": [], "mse": []}
    a_all, p_all = inputs(name)
    zeros = np.zeros(n, bool)
    for t in range(c["steps"]):
        obs, rew, term, trunc, info = env.step({"action": a_all[t], "prediction": p_all[t]})
        assert rew.dtype == np.float64 and obs["lidar"].dtype == np.float32
        for k in ("lidar", "odometry", "time_step"):
            rec[k].append(obs[k])
        rec["reward"].append(rew)
        rec["terminated"].append(term)
        rec["truncated"].append(trunc)
        mask = info.get("_base_reward", zeros)
        rec["info_mask"].append(mask)
        if mask.any():
            tgt = info["prediction"]["target"]
            if c["sparse"]:
                assert np.array_equal(tgt["_target"], mask) and np.array_equal(tgt["_weight"], mask)
                assert tgt["weight"].dtype == np.float64
                rec["weight"].append(tgt["weight"])
                tgt = tgt["target"]
            rec["base_reward"].append(info["base_reward"])
            rec["target"].append(tgt)
            rec["loss"].append(info["prediction"]["loss"])
        else:
            assert "base_reward" not in info and "prediction" not in info
            rec["base_reward"].append(np.zeros(n, np.float32))
            rec["target"].append(np.zeros((n, 2), np.float32))
            rec["loss"].append(np.zeros(n, np.float32))
            if c["sparse"]:
                rec["weight"].append(np.zeros(n, np.float64))
        rec["map_idx"].append(info.get("map_idx", np.zeros(n, np.int64)))
        rec["map_idx_mask"].append(info.get("_map_idx", zeros))
        if not c["static"]:
            rec["map"].append(np.packbits(obs["map"][..., 0] > 0, axis=-1))
        if c["log_stats"]:
            smask = info.get("_stats", zeros)
            rec["stats_mask"].append(smask)
            lens = np.zeros(n, np.int32)
            if smask.any():
                st = info["stats"]
                assert np.array_equal(st["_scalar"], smask) and np.array_equal(st["_vector"], smask)
                for k in STAT_KEYS:
                    assert st["scalar"][k].dtype == np.float64 and np.array_equal(st["scalar"]["_" + k], smask)
                    rec["stats_" + k].append(st["scalar"][k])
                for i in np.nonzero(smask)[0]:
                    lens[i] = len(st["vector"]["mse"][i])
                    for k in vec:
                        assert len(st["vector"][k][i]) == lens[i]
                        vec[k].extend(st["vector"][k][i])
            else:
                assert "stats" not in info
                for k in STAT_KEYS:
                    rec["stats_" + k].append(np.zeros(n, np.float64))
            rec["stats_len"].append(lens)
    env.close()
    out.update({k: np.stack(v) for k, v in rec.items()})
    if c["log_stats"]:
        for k, v in vec.items():
            out["stats_vector_" + k] = np.array(v, np.float32)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "active-perception-gym_amd"))
    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    res = {"envs_per_group": np.array(N.lib().apg_lidar_step_envs_per_group(N_ENVS))}
    for case in CASES:
        for key, v in run_case(ap, case).items():
            res[f"{case}/{key}"] = v
    np.savez(sys.argv[1], **res)
