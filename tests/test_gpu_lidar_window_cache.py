"""GPU parity of k_lidar_step's resident window cache (each env's staged 32 x 32 occupancy window kept in HBM between
steps and re-centred only when the env drifts or resets), against the oracle, bit for bit.

1. tests/lidar_knob_child.py (8 cases, N = 300) in fresh processes with the cache on and off (APG_STEP_WINCACHE=0), at
   64 and 256 envs per workgroup.
2. tests/lidar_wincache_child.py: drift-heavy cases (a shared heading that turns every 15 steps, 7-step episodes, a
   two-word pool, a static map, the largest lidar_range with a cache and the first without), with the cache's origin
   words and the env positions read between the steps, which prove that the cached path ran: windows are re-centred
   ahead of need (no env ever starts a step outside the hard zone), most envs keep their window on an ordinary step,
   and every origin is valid after every step.

After a child dies on a signal or its time limit no further GPU process is started."""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

import lidar_wincache_child as wcc
from test_gpu_lidar_knobs import _first_mismatch, oracle_trace

pytestmark = pytest.mark.gpu

KNOB_SETS = {
    "default": ({}, 64),
    "wincache_off": ({"APG_STEP_WINCACHE": "0"}, 64),
    "epb256": ({"APG_STEP_EPB": "256"}, 256),
    "epb256_wincache_off": ({"APG_STEP_EPB": "256", "APG_STEP_WINCACHE": "0"}, 256),
}

_child_died = []  # a child ended by a signal or its time limit: no further GPU process is started


def run_child(script: str, knobs: dict, out, tag: str):
    if _child_died:
        pytest.fail(f"not started: the child of {_child_died[0]!r} was killed or faulted the GPU")
    env = {k: v for k, v in os.environ.items() if not k.startswith("APG_")}
    env.update(knobs)
    here = os.path.dirname(os.path.abspath(__file__))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.join(here, script), str(out)], env=env, check=False, timeout=300,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _child_died.append(tag)
        pytest.fail(f"{tag}: the child ran into its time limit")
    if r.returncode < 0 or (r.returncode and "memory access" in r.stderr.lower()):  # a signal, or a GPU fault
        _child_died.append(tag)
    assert r.returncode == 0, f"{tag}: child exit {r.returncode}\n{r.stderr[-3000:]}"
    got = np.load(out)
    print(f"{tag}: envs_per_group={int(got['envs_per_group'])}, child {time.perf_counter() - t0:.1f} s")
    return got


def compare(got, traces: dict, tag: str, extra_keys=()):
    bad = []
    for case, tr in traces.items():
        for key, want in tr.items():
            g = got[f"{case}/{key}"]
            if not (g.dtype == want.dtype and np.array_equal(g, want, equal_nan=want.dtype.kind == "f")):
                axis = 0 if key.startswith("reset_") else 9 if key.startswith("stats_vector_") else 1
                bad.append(f"{case}/{key}: {_first_mismatch(g, want, axis)}")
    assert not bad, f"{tag}:\n" + "\n".join(bad)


@pytest.fixture(scope="module")
def knob_traces(oracle_mod):
    from lidar_knob_child import CASES

    return {name: oracle_trace(oracle_mod, name) for name in CASES}


@pytest.mark.parametrize("knob_set", list(KNOB_SETS))
def test_knob_cases_match_oracle_with_and_without_cache(gpu, knob_traces, tmp_path, knob_set):
    knobs, want_epg = KNOB_SETS[knob_set]
    got = run_child("lidar_knob_child.py", knobs, tmp_path / "trace.npz", knob_set)
    assert int(got["envs_per_group"]) == want_epg, knob_set
    want_keys = {"envs_per_group"} | {f"{c}/{k}" for c, tr in knob_traces.items() for k in tr}
    assert set(got.files) == want_keys, set(got.files) ^ want_keys
    compare(got, knob_traces, knob_set)


def drift_oracle_trace(oracle_mod, name: str) -> dict:
    """What lidar_wincache_child.run_case records of the outputs, from the oracle env on the same inputs."""
    c = wcc.case_params(name)
    n = wcc.N_ENVS
    ref = oracle_mod.OracleLidarVectorEnv(n, c["kind"], c["size"], c["static"], 0, c["beams"],
                                          lidar_range=c["lidar_range"], step_limit=c["step_limit"],
                                          pool=wcc.make_pool() if c["kind"] == "pool" else None)
    ref.reset(wcc.SEED)
    out = {"reset_lidar": ref.lidar.copy()}
    rec = {}
    a_all, p_all = wcc.inputs(name)
    for t in range(wcc.STEPS):
        ref.step(a_all[t], p_all[t])
        mask = ref.info_mask.astype(bool)
        for k in ("lidar", "odometry", "time_step"):
            rec.setdefault(k, []).append(getattr(ref, k).copy())
        rec.setdefault("reward", []).append(np.array(ref.reward, np.float64))
        rec.setdefault("terminated", []).append(ref.terminated.astype(bool))
        rec.setdefault("truncated", []).append(ref.truncated.astype(bool))
        rec.setdefault("info_mask", []).append(mask)
        rec.setdefault("base_reward", []).append(np.where(mask, ref.base_reward, np.float32(0)))
        rec.setdefault("target", []).append(np.where(mask[:, None], ref.target, np.float32(0)))
        rec.setdefault("loss", []).append(np.where(mask, ref.loss, np.float32(0)))
        if not c["static"]:
            rec.setdefault("map", []).append(np.packbits(ref.map > 0, axis=-1))
    assert not ref.no_free_cell(), name
    ref.close()
    out.update({k: np.stack(v) for k, v in rec.items()})
    return out


@pytest.fixture(scope="module")
def drift_traces(oracle_mod):
    return {name: drift_oracle_trace(oracle_mod, name) for name in wcc.CASES}


@pytest.fixture(scope="module")
def drift_run(gpu, tmp_path_factory):
    return run_child("lidar_wincache_child.py", {}, tmp_path_factory.mktemp("wincache") / "trace.npz", "drift")


def test_drift_cases_match_oracle(drift_run, drift_traces):
    compare(drift_run, drift_traces, "drift")


def origin_xy(words):
    return (words & 0xFFF).astype(np.int64) - 64, ((words >> 12) & 0xFFF).astype(np.int64) - 64


@pytest.mark.parametrize("case", list(wcc.CASES))
def test_drift_cases_ran_the_cached_path(drift_run, case):
    got = drift_run
    n = wcc.N_ENVS
    if case in wcc.UNCACHED:
        assert int(got[f"{case}/cache_bytes"]) == 0 and f"{case}/origin" not in got.files
        return
    assert int(got[f"{case}/cache_bytes"]) == n * 33 * 4
    org, pos = got[f"{case}/origin"], got[f"{case}/pos"]  # [STEPS, n] / [STEPS, n, 2]: the state after each step
    done = got[f"{case}/terminated"] | got[f"{case}/truncated"]  # ended at step t: resets at step t + 1
    hard, inner = got[f"{case}/zone_hard"], got[f"{case}/zone_inner"]
    assert int(got[f"{case}/max_drift"]) == 2 and np.array_equal(inner, hard + np.array([2, -2, 2, -2]))
    assert ((org >> 31) == 1).all(), "an env without a valid origin after a step"
    x0, y0 = origin_xy(org)
    ox, oy = np.floor(pos[..., 0]).astype(np.int64) - x0, np.floor(pos[..., 1]).astype(np.int64) - y0
    in_hard = (ox >= hard[0]) & (ox <= hard[1]) & (oy >= hard[2]) & (oy <= hard[3])
    in_inner = (ox >= inner[0]) & (ox <= inner[1]) & (oy >= inner[2]) & (oy <= inner[3])
    # re-centring ahead: every env that does not reset at the next step starts it inside the hard zone
    assert (in_hard | done).all(), f"{case}: {int((~(in_hard | done)).sum())} step starts outside the hard zone"
    changed = org[1:] != org[:-1]  # by step t + 1
    quiet = ~done[:-1].any(axis=1)  # steps t + 1 at which no env resets
    # a window re-centred although its env did not reset and was still inside the hard zone: the refresh of the step
    # before moved it (it left the inner zone), not a fallback of its workgroup
    wg = np.arange(n) // int(got["envs_per_group"])
    refreshed = 0
    for t in np.nonzero(quiet)[0]:
        for g in np.unique(wg[changed[t]]):
            m = wg == g
            if in_hard[t][m].all():  # the workgroup took the cached path at step t + 1
                assert (~in_inner[t][m & changed[t]]).all(), f"{case}: step {t + 1}, a window moved inside the inner zone"
                refreshed += int((m & changed[t]).sum())
    hits = 1.0 - changed[quiet].mean() if quiet.any() else None
    print(f"{case}: {refreshed} windows re-centred ahead, hit rate on quiet steps {hits}")
    if case != "rooms64_b32_drift_limit7":
        assert refreshed > 0, f"{case}: no window was re-centred ahead"
        assert quiet.sum() >= wcc.STEPS // 2 and hits > 0.5, (case, hits)
