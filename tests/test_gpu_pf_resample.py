"""lidar_pf_resample, the kernel k_pf_resample (csrc/apg_pf_resample.hip), env.pf_update and LidarParticleFilter on the
GPU.

The kernel is compared with the numpy restatement of tests/test_pf_resample_host.py at the smallest shapes that cross
each boundary of its work split: bit for bit on every output where the exponential is exact (log-weights that take one
finite value and -inf), within two ulps of a float64 exponential on the weights of random sets, and bit for bit again on
everything after the exponential once the restatement is given the kernel's own weights.  pf_update is tied to
pose_scores + lidar_pf_resample, the filter to the env: a filter that holds the true position must reproduce it, and the
step kernel's target, bit for bit.
"""

import ctypes
import functools

import numpy as np
import pytest

from test_gpu_scan_poses import dev, host
from test_pf_resample_host import F, pf_resample_np

pytestmark = pytest.mark.gpu

OUTPUTS = ("weight", "estimate", "ess", "index", "poses_out", "logw_out", "resampled")
AFTER_EXP = ("ess", "index", "poses_out", "logw_out", "resampled")
SIDE = 32.0
ONE_LESS = np.nextafter(F(1), F(0))


def k_values():
    from ap_gym_amd import _native as N

    wk, tile = N.PF_RESAMPLE_WAVE_K, N.PF_RESAMPLE_TILE
    return [1, 2, wk - 1, wk, wk + 1, tile - 1, tile, tile + 1, 1000, N.PF_RESAMPLE_MAX_K]


def m_values():
    from ap_gym_amd import _native as N

    return [1, 2 * N.PF_RESAMPLE_SETS_PER_WG + 1]  # the second: a ragged last workgroup of one-wave sets


K_IDX = list(range(10))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def equal_nan(a, b):
    """array_equal with NaN equal to NaN, and 0.0 distinct from -0.0."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f") and (
        a.dtype.kind != "f" or np.array_equal(np.signbit(a), np.signbit(b)))


@functools.lru_cache(maxsize=None)
def random_case(k, m):
    """logw ~ N(0, 1), scores uniform in [0, 8] (score_scale 0.5), poses uniform in a 32 x 32 map (read-only)."""
    rng = np.random.default_rng(1000 * k + m)
    c = dict(logw=rng.standard_normal((m, k)).astype(F), scores=rng.uniform(0, 8, (m, k)).astype(F),
             poses=rng.uniform(0, SIDE, (m, k, 2)).astype(F), u=rng.random(m).astype(F))
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def exact_case(k):
    """Sets whose log-weights take one finite value and -inf (weights in {0, 1}: no exponential rounds), with the special
    inputs: 0 random alive mask, u = 0; 1 the same with u = nextafter(1, 0); 2 all -inf (restart); 3 a NaN log-weight;
    4 a +inf log-weight; 5 a pose with an infinite coordinate; 6 uniform; 7 one-hot by scores 1e4 * j (exp underflows
    to 0 in every precision); 8 every particle bad; 9 one-hot by -inf, u random; 10 a NaN u; 11 u = 7 (clamped)."""
    rng = np.random.default_rng(77 + k)
    m = 12
    alive = rng.random((m, k)) < 0.4
    alive[:, rng.integers(0, k)] = True
    logw = np.where(alive, F(-1.25), F(-np.inf)).astype(F)
    scores = np.full((m, k), 2.0, F)
    poses = rng.uniform(0, SIDE, (m, k, 2)).astype(F)
    u = rng.random(m).astype(F)
    u[0], u[1], u[10], u[11] = 0.0, ONE_LESS, np.nan, 7.0
    logw[2] = -np.inf
    logw[3, k // 2] = np.nan
    logw[4, k // 3] = np.inf
    poses[5, (2 * k) // 3, 1] = -np.inf
    logw[6] = 0.5
    logw[7] = 0.0
    scores[7] = 1e4 * np.arange(k)
    logw[8] = np.nan
    logw[9] = -np.inf
    logw[9, k - 1] = 3.0
    c = dict(logw=logw, scores=scores, poses=poses, u=u)
    for v in c.values():
        v.setflags(write=False)
    return c


def run_op(gpu, c, ess_frac, score_scale=0.5, in_place=False, use_err=True):
    """lidar_pf_resample on numpy inputs; returns (outputs named as the C struct's, error word)."""
    import torch

    import ap_gym_amd as ap

    err = torch.zeros(1, dtype=torch.int32, device=gpu) if use_err else None
    logw = dev(np.array(c["logw"]), gpu)
    res = ap.lidar_pf_resample(dev(np.array(c["poses"]), gpu), logw, dev(np.array(c["scores"]), gpu),
                               score_scale=score_scale, u=dev(np.array(c["u"]), gpu), ess_frac=ess_frac, err=err,
                               logw_out=logw if in_place else None)
    if in_place:
        assert res.logw is logw
    got = dict(weight=res.weight, estimate=res.estimate, ess=res.ess, index=res.index, poses_out=res.poses,
               logw_out=res.logw, resampled=res.resampled)
    return {name: v.cpu().numpy() for name, v in got.items()}, (int(err.item()) if use_err else None)


@pytest.mark.parametrize("ess_frac", [0.0, 0.5, 1.0, 1.5])
@pytest.mark.parametrize("ki", K_IDX)
def test_exact_sets_equal_the_restatement_bit_for_bit(gpu, ki, ess_frac):
    from ap_gym_amd import _native as N

    k = k_values()[ki]
    c = exact_case(k)
    want = pf_resample_np(c["poses"], c["logw"], c["scores"], 0.5, c["u"], ess_frac)
    assert set(np.unique(want["weight"])) <= {0.0, 1.0}
    got, err = run_op(gpu, c, ess_frac)
    for name in OUTPUTS:
        assert got[name].dtype == want[name].dtype and equal_nan(got[name], want[name]), (k, ess_frac, name)
    assert err == N.APG_ERR_BAD_POSE == want["err"]
    # the uniform set: the identity, ess == K, resampled only by ess_frac > 1
    assert np.array_equal(got["index"][6], np.arange(k)) and got["ess"][6] == k
    assert got["resampled"][6] == (ess_frac > 1) and same(got["poses_out"][6], c["poses"][6])
    assert got["ess"][7] == 1 and (not got["resampled"][7] or (got["index"][7] == 0).all())
    assert np.isnan(got["estimate"][8]).all() and got["ess"][8] == 0 and not got["resampled"][8]
    assert got["index"].min() >= 0 and got["index"].max() < k
    # flags: set exactly when a bad particle exists; -inf alone sets none
    clean = {name: v[[0, 1, 2, 6, 7, 9, 10, 11]] for name, v in c.items()}
    got2, err2 = run_op(gpu, clean, ess_frac)
    assert err2 == 0
    for name in OUTPUTS:
        assert equal_nan(got2[name], want[name][[0, 1, 2, 6, 7, 9, 10, 11]]), (k, ess_frac, name)
    for row in (3, 4, 5, 8):
        assert run_op(gpu, {name: v[[0, row]] for name, v in c.items()}, ess_frac)[1] == N.APG_ERR_BAD_POSE, row
    if ess_frac == 0.5:  # err=None is accepted
        got3, _ = run_op(gpu, c, ess_frac, use_err=False)
        assert all(equal_nan(got3[name], got[name]) for name in OUTPUTS)


@pytest.mark.parametrize("mi", [0, 1])
@pytest.mark.parametrize("ki", K_IDX)
def test_random_sets_weights_then_everything_after_them_exactly(gpu, ki, mi):
    k, m = k_values()[ki], m_values()[mi]
    c = random_case(k, m)
    worst = 0.0
    for ess_frac in (0.0, 0.5, 1.5):  # (0: no set is resampled, logw_out is l - l_max everywhere)
        ref = pf_resample_np(c["poses"], c["logw"], c["scores"], 0.5, c["u"], ess_frac)
        got, err = run_op(gpu, c, ess_frac)
        assert err == 0
        # weights: OCML's 1-ulp expf plus the rounding of the float64 reference to float32
        dev_ulps = np.abs(got["weight"].astype(np.float64) - ref["weight"]) / np.spacing(ref["weight"])
        worst = max(worst, float(dev_ulps.max()))
        print(f"K {k} M {m} ess_frac {ess_frac}: max weight deviation {dev_ulps.max():.3f} ulp, "
              f"{int(got['resampled'].sum())} of {m} sets resampled")
        assert (np.abs(got["weight"] - ref["weight"]) <= 2 * np.spacing(ref["weight"])).all(), (k, m, worst)
        assert (got["weight"].max(axis=1) == 1.0).all()
        assert (got["weight"][np.arange(m), ref["d"].argmax(axis=1)] == 1.0).all()
        keep = got["resampled"] == 0
        assert same(got["logw_out"][keep], ref["d"][keep])
        # everything after the exponential, from the kernel's own weights
        want = pf_resample_np(c["poses"], c["logw"], c["scores"], 0.5, c["u"], ess_frac, weight=got["weight"])
        for name in AFTER_EXP:
            assert got[name].dtype == want[name].dtype and equal_nan(got[name], want[name]), (k, m, ess_frac, name)
        bound = 2.0 ** -23 * np.abs(c["poses"]).max(axis=1)
        assert (np.abs(got["estimate"] - want["estimate"]) <= bound).all(), (k, m)
        if ess_frac == 1.5:
            assert got["resampled"].all() and (got["logw_out"] == 0).all()
            assert (np.diff(got["index"], axis=1) >= 0).all()
        # in place: logw_out is logw
        again, _ = run_op(gpu, c, ess_frac, in_place=True)
        for name in OUTPUTS:
            assert same(again[name], got[name]), (k, m, ess_frac, name)


@pytest.mark.parametrize("k", [5, 300])
def test_identical_poses_and_optional_inputs(gpu, k):
    import torch

    import ap_gym_amd as ap

    rng = np.random.default_rng(k)
    m = 3
    pose = rng.uniform(0, SIDE, (m, 1, 2)).astype(F)
    poses = dev(np.repeat(pose, k, axis=1), gpu)
    logw = dev(rng.standard_normal((m, k)).astype(F), gpu)
    res = ap.lidar_pf_resample(poses, logw, ess_frac=0.0)  # no scores, no u, no err
    assert same(res.estimate.cpu().numpy(), pose[:, 0])
    want = pf_resample_np(host(poses), host(logw), ess_frac=0.0)
    assert same(res.logw.cpu().numpy(), want["logw_out"]) and not res.resampled.any()
    assert res.resampled.dtype == torch.uint8 and res.index.dtype == torch.int32
    none = ap.lidar_pf_resample(poses, ess_frac=1.0, u=torch.zeros(m, device=gpu))  # no logw: uniform
    assert (none.weight == 1).all() and (none.ess == k).all() and not none.resampled.any()
    gen = torch.Generator(device=gpu).manual_seed(5)
    a = ap.lidar_pf_resample(poses, logw, ess_frac=1.5, generator=gen)
    gen.manual_seed(5)
    u = torch.rand(m, dtype=torch.float32, device=gpu, generator=gen)
    c = ap.lidar_pf_resample(poses, logw, ess_frac=1.5, u=u)
    assert a.resampled.all() and (a.logw == 0).all()
    assert torch.equal(a.index, c.index)  # u=None draws torch.rand(M) from the generator


@pytest.mark.parametrize("k", [7, 70])
def test_each_output_alone_through_the_c_abi(gpu, k):
    """Every output pointer may be NULL: each output alone equals the full call."""
    import torch

    from ap_gym_amd import _native as N

    c = random_case(k, 5)
    got, _ = run_op(gpu, c, 1.0)
    t = {name: dev(np.array(c[name]), gpu) for name in ("logw", "scores", "poses", "u")}
    fn = N.lib().apg_lidar_pf_resample
    with torch.cuda.device(gpu):
        for name in OUTPUTS:
            out = torch.zeros(got[name].shape, dtype=torch.from_numpy(got[name]).dtype, device=gpu)
            a = N.PfResampleArgs(logw=t["logw"].data_ptr(), score=t["scores"].data_ptr(), poses=t["poses"].data_ptr(),
                                 u=t["u"].data_ptr(), m=5, k=k, score_scale=0.5, ess_frac=1.0)
            setattr(a, name, out.data_ptr())
            assert fn(ctypes.byref(a), N.current_stream_ptr(gpu)) == N.APG_OK
            assert same(out.cpu().numpy(), got[name]), name
        a = N.PfResampleArgs(logw=t["logw"].data_ptr(), score=t["scores"].data_ptr(), poses=t["poses"].data_ptr(),
                             u=t["u"].data_ptr(), m=5, k=k, score_scale=0.5, ess_frac=1.0)
        assert fn(ctypes.byref(a), N.current_stream_ptr(gpu)) == N.APG_OK  # no output at all
        torch.cuda.synchronize(gpu)


def test_graph_capture_and_replay(gpu):
    import torch

    import ap_gym_amd as ap

    k, m = 70, 9
    first, second = random_case(k, m), random_case(k + 1, m)
    poses = dev(np.array(first["poses"]), gpu)
    logw, scores, u = (dev(np.array(first[name]), gpu) for name in ("logw", "scores", "u"))
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    kw = dict(score_scale=0.5, ess_frac=1.0, err=err)
    ap.lidar_pf_resample(poses, logw, scores, u=u, **kw)  # (loads the op before the capture)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        res = ap.lidar_pf_resample(poses, logw, scores, u=u, **kw)
    torch.cuda.current_stream(gpu).wait_stream(side)
    for name, x in (("logw", logw), ("scores", scores), ("u", u)):
        x.copy_(dev(np.array(second[name][:, :k] if name != "u" else second[name]), gpu))
    graph.replay()
    eager = ap.lidar_pf_resample(poses, logw, scores, u=u, **kw)
    for a, b in zip(res, eager):
        assert same(a.cpu().numpy(), b.cpu().numpy())
    assert int(err.item()) == 0


def _env(ap, env_id, gpu, backend, map_obs, n=5, **kw):
    return ap.make_vec(env_id, num_envs=n, device=gpu, array_backend=backend, map_obs=map_obs, lidar_beam_count=8, **kw)


@pytest.mark.parametrize("backend", ["torch", "numpy"])
@pytest.mark.parametrize("map_obs", ["dense", "bits"])
@pytest.mark.parametrize("env_id", ["LIDARLocRooms-v0", "LIDARLocMaze-v0"])
def test_pf_update_is_pose_scores_then_resample(gpu, env_id, map_obs, backend):
    import torch

    import ap_gym_amd as ap

    env = _env(ap, env_id, gpu, backend, map_obs)
    env.reset(seed=3)
    rng = np.random.default_rng(len(env_id))
    h, w = env.dataset.map_height, env.dataset.map_width
    k, sigma = 7, 0.3

    def give(a):
        return a if backend == "numpy" else dev(a, gpu)

    for step in range(2):
        for ids in (None, np.array([3, 0, 4, 1, 2]), np.array([2, 4, 2, 0])):
            m = 5 if ids is None else len(ids)
            particles = rng.uniform(0, [w, h], (m, k, 2)).astype(F)
            particles[:, 0] = host(env._t["pos"])[np.arange(5) if ids is None else ids]  # one that scores 0
            logw = rng.standard_normal((m, k)).astype(F)
            u = rng.random(m).astype(F)
            got = env.pf_update(give(particles), give(logw), sigma=sigma, env_ids=ids, ess_frac=0.9, u=give(u))
            assert type(got.poses) is (np.ndarray if backend == "numpy" else torch.Tensor)
            scores = env.pose_scores(give(particles), None, ids)
            want = ap.lidar_pf_resample(dev(particles, gpu), dev(logw, gpu), dev(host(scores), gpu),
                                        score_scale=F(1 / (2 * sigma * sigma)), u=dev(u, gpu), ess_frac=0.9)
            assert got._fields == want._fields + ("scores",)
            for name, b in zip(want._fields, want):
                assert same(host(getattr(got, name)), host(b)), (step, ids, name)
            assert same(host(got.scores), host(scores)) and (host(got.scores)[:, 0] == 0).all()
            auto = env.pf_update(give(particles), sigma=sigma, env_ids=ids, ess_frac=0.0)  # no logw, no u
            assert not host(auto.resampled).any() and same(host(auto.poses), particles)
        a = rng.uniform(-1, 1, (5, 2)).astype(F)
        env.step({"action": give(a), "prediction": give(np.zeros((5, 2), F))})
    env.check_errors()
    with pytest.raises(ValueError, match="sigma"):
        env.pf_update(give(particles), sigma=0.0, env_ids=ids)
    with pytest.raises(ValueError, match="one pose set per chosen sub-env"):
        env.pf_update(give(particles), sigma=sigma)
    if backend == "numpy":  # raised at once
        with pytest.raises(IndexError):
            env.pf_update(particles[:2], sigma=sigma, env_ids=[0, 5])
    else:
        env.pf_update(give(particles[:2]), sigma=sigma, env_ids=[0, 5])
        with pytest.raises(IndexError):
            env.check_errors()
        particles[1, 2, 0] = np.nan
        res = env.pf_update(give(particles[:2]), sigma=sigma, env_ids=[0, 1], ess_frac=1.5)  # (always resampled)
        assert float(res.weight[1, 2]) == 0 and res.resampled.all() and not (res.index[1] == 2).any()
        with pytest.raises(ValueError, match="pf_update"):
            env.check_errors()
    env.check_errors()
    env.close()


def _tracking_filter(ap, gpu, env, k=65):
    """A filter whose particle 0 of every set is the sub-env's position; the rest are uniform."""
    import torch

    n = env.num_envs
    pf = ap.LidarParticleFilter(env, k, sigma=1e-3, generator=torch.Generator(device=gpu).manual_seed(11))
    pf.reset()
    start = pf.particles.clone()
    start[:, 0] = env._t["pos"]
    pf.reset(start)
    assert pf.particles.shape == (n, k, 2) and (pf.logw == 0).all()
    return pf


@pytest.mark.parametrize("env_id", ["LIDARLocRooms-v0", "LIDARLocMaze-v0"])
def test_filter_that_holds_the_position_reproduces_it(gpu, env_id):
    import torch

    import ap_gym_amd as ap

    n, k = 4, 65
    env = _env(ap, env_id, gpu, "torch", "bits", n=n, max_episode_steps=100)
    env.reset(seed=9)
    pf = _tracking_filter(ap, gpu, env, k)
    with pytest.raises(RuntimeError, match="no estimate yet"):
        pf.estimate
    res = pf.update()
    assert res.resampled.all() and (res.index == 0).all()  # sigma = 1e-3: only the true position survives
    rng = np.random.default_rng(2)
    for step in range(6):
        pred = pf.prediction.clone()
        action = dev(rng.uniform(-1, 1, (n, 2)).astype(F), gpu)
        _, _, term, _, _ = env.step({"action": action, "prediction": pred})
        assert not term.any() and not env.device_outputs()["reset_mask"].any()
        pf.predict(action)
        res = pf.update()
        assert same(host(pf.estimate), host(env._t["pos"])), step
        assert same(host(pred), host(env.device_outputs()["target"])), step  # the step's target: the pose before it
        picked = torch.gather(res.scores, 1, res.index.long())
        assert (picked == 0).all(), step
    env.check_errors()
    env.close()


def test_filter_redraws_the_sets_of_sub_envs_that_autoreset(gpu):
    import torch

    import ap_gym_amd as ap

    n, k = 4, 65
    env = _env(ap, "LIDARLocRooms-v0", gpu, "torch", "dense", n=n, max_episode_steps=3)
    env.reset(seed=9)
    pf = _tracking_filter(ap, gpu, env, k)
    pf.update()
    rng = np.random.default_rng(3)
    w, h = env.dataset.map_width, env.dataset.map_height
    bits = env._t["occ"].view(n, h, -1)

    def step():
        action = dev(rng.uniform(-1, 1, (n, 2)).astype(F), gpu)
        env.step({"action": action, "prediction": pf.prediction})
        return action

    for i in range(3):  # the episode's three steps: the filter tracks
        pf.predict(step())
        pf.update()
        assert same(host(pf.estimate), host(env._t["pos"])), i
    # one sub-env alone marked in the env's reset_mask buffer: only its set is drawn anew
    mask = env.device_outputs()["reset_mask"]
    assert not mask.any()
    pf.logw = torch.full_like(pf.logw, -0.5)
    before = pf.particles.clone()
    mask[2] = True
    action = dev(rng.uniform(-1, 1, (n, 2)).astype(F), gpu)
    moved = ap.lidar_move_poses(bits, w, before, action[:, None, None, :].expand(n, k, 1, 2).contiguous(),
                                base_reward=False).pos.view(n, k, 2)
    after = pf.predict(action)
    others = [0, 1, 3]
    assert same(host(after[others]), host(moved[others])) and (pf.logw[others] == -0.5).all()
    assert (pf.logw[2] == 0).all() and not torch.equal(after[2], moved[2])
    assert len(torch.unique(after[2], dim=0)) == k and (after[2] >= 0).all() and (after[2] < w).all()
    mask[2] = False
    pf.reset(before)
    pf.update()
    # the real thing: every sub-env reached its step limit, the next step autoresets them all
    action = step()
    assert env.device_outputs()["reset_mask"].all()
    pf.predict(action)
    assert (pf.logw == 0).all() and not torch.equal(pf.particles, before)
    assert all(len(torch.unique(pf.particles[i], dim=0)) == k for i in range(n))
    assert (pf.particles >= 0).all() and (pf.particles[..., 0] < w).all() and (pf.particles[..., 1] < h).all()
    res = pf.update()
    assert torch.isfinite(res.ess).all()
    env.check_errors()
    env.close()
