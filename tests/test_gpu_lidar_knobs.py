"""GPU parity of k_lidar_step's instances that batch size alone selects only at 65536 envs and more, and of the
LIDAR tuning knobs (APG_STEP_EPB, APG_STEP_P4, APG_STEP_PRETEST, APG_MAZE_LANES: "the outputs do not depend on
it").

APG_STEP_EPB=256 runs the 256-envs-per-workgroup instance (1024 threads, the one bench.py times) at N = 300, so
every env of every slot of a full workgroup and of a partial one is compared with the oracle, over every generator
(fused rooms, pool, prefetched mazes, none), log_stats, sparse, packed rows, the unfused step after k_lidar_reset,
a 6-beam and a 72-beam instance and a range-8 scan.  The library reads each knob once per process, so each knob
set runs tests/lidar_knob_child.py in a fresh process; the comparison is against the oracle (bit for bit), not
against another child.  apg_lidar_step_envs_per_group proves the knob took effect.
"""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

from lidar_knob_child import CASES, N_ENVS, SEED, STAT_KEYS, case_params, inputs, make_pool

pytestmark = pytest.mark.gpu

KNOB_SETS = {
    "default": ({}, 64),
    "epb256": ({"APG_STEP_EPB": "256"}, 256),
    "epb256_p4_off": ({"APG_STEP_EPB": "256", "APG_STEP_P4": "0"}, 256),
    "pretest_off": ({"APG_STEP_PRETEST": "0"}, 64),
    "pretest_on_maze_lanes3": ({"APG_STEP_PRETEST": "1", "APG_MAZE_LANES": "3"}, 64),
}

_child_died = []  # a child ended by a signal or its time limit: no further GPU process is started


def oracle_trace(oracle_mod, name: str) -> dict:
    """What lidar_knob_child.run_case records, from the oracle env on the same inputs (and the
    ActiveRegressionLogWrapper stats restated from its targets like test_vector_env_matches_oracle does)."""
    c = case_params(name)
    n = N_ENVS
    ref = oracle_mod.OracleLidarVectorEnv(n, c["kind"], c["size"], c["static"], 0, c["beams"],
                                          lidar_range=c["lidar_range"], step_limit=c["step_limit"],
                                          sparse=c["sparse"], max_rooms=c["max_rooms"],
                                          pool=make_pool() if c["kind"] == "pool" else None)
    ref.reset(SEED)
    out = {"reset_lidar": ref.lidar.copy(), "reset_odometry": ref.odometry.copy(),
           "reset_time_step": ref.time_step.copy(), "reset_map_idx": ref.map_idx.astype(np.int64)}
    if not c["static"]:
        out["reset_map"] = np.packbits(ref.map > 0, axis=-1)
    rec = {}
    vec = {"euclidean_distance": [], "mse": []}
    hist = [[] for _ in range(n)]
    a_all, p_all = inputs(name)
    prev_done = np.zeros(n, bool)
    resets = np.zeros(n, int)

    def put(k, v):
        rec.setdefault(k, []).append(v)

    for t in range(c["steps"]):
        ref.step(a_all[t], p_all[t])
        mask = ref.info_mask.astype(bool)
        # NEXT_STEP autoreset: the envs that ended at the previous step reset now and report no step info
        assert np.array_equal(mask, ~prev_done), (name, t)
        resets += prev_done
        done = (ref.terminated | ref.truncated).astype(bool)
        for k in ("lidar", "odometry", "time_step"):
            put(k, getattr(ref, k).copy())
        put("reward", np.array(ref.reward, np.float64))
        put("terminated", ref.terminated.astype(bool))
        put("truncated", ref.truncated.astype(bool))
        put("info_mask", mask)
        put("base_reward", np.where(mask, ref.base_reward, np.float32(0)))
        put("target", np.where(mask[:, None], ref.target, np.float32(0)))
        put("loss", np.where(mask, ref.loss, np.float32(0)))
        put("map_idx", np.where(prev_done, ref.map_idx.astype(np.int64), 0))
        put("map_idx_mask", prev_done)
        if not c["static"]:
            put("map", np.packbits(ref.map > 0, axis=-1))
        if c["sparse"]:
            put("weight", np.array(ref.weight, np.float64))
        if c["log_stats"]:
            for i in np.nonzero(mask)[0]:
                d = ref.target[i] - p_all[t][i]
                with np.errstate(over="ignore"):
                    hist[i].append((np.linalg.norm(d), np.mean(d ** 2)))
            sc = {k: np.zeros(n, np.float64) for k in STAT_KEYS}
            lens = np.zeros(n, np.int32)
            for i in np.nonzero(done)[0]:
                ed = np.array([h[0] for h in hist[i]], np.float32)
                ms = np.array([h[1] for h in hist[i]], np.float32)
                sc["avg_euclidean_distance"][i], sc["avg_mse"][i] = float(np.mean(ed)), float(np.mean(ms))
                sc["final_euclidean_distance"][i], sc["final_mse"][i] = float(ed[-1]), float(ms[-1])
                lens[i] = len(ed)
                vec["euclidean_distance"].extend(ed)
                vec["mse"].extend(ms)
                hist[i] = []
            put("stats_mask", done)
            put("stats_len", lens)
            for k in STAT_KEYS:
                put("stats_" + k, sc[k])
        prev_done = done
    out.update({k: np.stack(v) for k, v in rec.items()})
    if c["log_stats"]:
        for k, v in vec.items():
            out["stats_vector_" + k] = np.array(v, np.float32)
    # the conditions under which a pass means something: every env went through an autoreset, every drawn map had a
    # free cell (the reference raises there)
    assert resets.min() >= 1, (name, int(resets.min()))
    assert not ref.no_free_cell(), name
    ref.close()
    return out


@pytest.fixture(scope="module")
def oracle_traces(oracle_mod):
    return {name: oracle_trace(oracle_mod, name) for name in CASES}


def _first_mismatch(got, want, env_axis):
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape/dtype {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    bad = (got != want) & ~((got != got) & (want != want)) if got.dtype.kind == "f" else got != want
    idx = np.argwhere(bad)
    envs = sorted(set(int(i[env_axis]) for i in idx)) if env_axis < got.ndim else []
    return f"{len(idx)} elements differ, first at {tuple(int(x) for x in idx[0])}, env slots {envs[:12]}"


@pytest.mark.parametrize("knob_set", list(KNOB_SETS))
def test_lidar_tuning_knobs_match_oracle(gpu, oracle_traces, tmp_path, knob_set):
    if _child_died:
        pytest.fail(f"not started: the child of knob set {_child_died[0]!r} was killed or faulted the GPU")
    knobs, want_epg = KNOB_SETS[knob_set]
    env = {k: v for k, v in os.environ.items() if not k.startswith("APG_")}
    env.update(knobs)
    out = tmp_path / "trace.npz"
    here = os.path.dirname(os.path.abspath(__file__))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.join(here, "lidar_knob_child.py"), str(out)], env=env,
                           check=False, timeout=300, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _child_died.append(knob_set)
        pytest.fail(f"{knob_set}: the child ran into its time limit")
    if r.returncode < 0 or (r.returncode and "memory access" in r.stderr.lower()):  # a signal, or a GPU fault
        _child_died.append(knob_set)
    assert r.returncode == 0, f"{knob_set}: child exit {r.returncode}\n{r.stderr[-3000:]}"
    got = np.load(out)
    epg = int(got["envs_per_group"])
    print(f"{knob_set}: envs_per_group={epg}, child {time.perf_counter() - t0:.1f} s")
    assert epg == want_epg, (knob_set, epg)
    want_keys = {"envs_per_group"} | {f"{c}/{k}" for c, tr in oracle_traces.items() for k in tr}
    assert set(got.files) == want_keys, set(got.files) ^ want_keys
    bad = []
    for case, tr in oracle_traces.items():
        for key, want in tr.items():
            g = got[f"{case}/{key}"]
            if not (g.dtype == want.dtype and np.array_equal(g, want, equal_nan=want.dtype.kind == "f")):
                # the env axis: 0 of the reset outputs, 1 of the per-step ones (the stats vectors have none)
                axis = 0 if key.startswith("reset_") else 9 if key.startswith("stats_vector_") else 1
                bad.append(f"{case}/{key}: {_first_mismatch(g, want, axis)}")
    assert not bad, f"{knob_set} (envs_per_group {epg}):\n" + "\n".join(bad)
