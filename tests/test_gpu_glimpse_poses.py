"""Glimpses, fused match scores and moves of the image envs at caller-chosen positions (k_glimpse_scores,
k_image_move; ap_gym_amd.glimpse_poses and the env methods glimpses_at / glimpse_scores / lookahead) against the
numpy restatements of tests/test_glimpse_poses_host.py and against the env's own step outputs, bit for bit."""

import functools

import numpy as np
import pytest

from test_glimpse_poses_host import F, glimpse_scores_np, glimpses_np, move_positions_np

pytestmark = pytest.mark.gpu

POOL_LEN = 6
FORMATS = {  # name: (pool channels, observation channels, dtype, tiled)
    "u8_grey": (1, 1, np.uint8, False), "grey_rgb": (1, 3, np.uint8, False), "u8_rgb": (3, 3, np.uint8, False),
    "u8_tiled": (3, 3, np.uint8, True), "f32_grey": (1, 1, np.float32, False), "f32_rgb": (3, 3, np.float32, False)}


@functools.lru_cache(maxsize=None)
def host_pool(fmt, hw):
    pc, _, dtype, _ = FORMATS[fmt]
    rng = np.random.default_rng(hw[0] * 100 + hw[1] + pc)
    if dtype == np.uint8:
        pool = rng.integers(0, 256, (POOL_LEN, *hw, pc), dtype=np.uint8)
    else:  # values beyond [0, 1]: both clips of the glimpse
        pool = rng.uniform(-0.2, 1.2, (POOL_LEN, *hw, pc)).astype(np.float32)
    return pool


def dev_pool(fmt, hw, dev):
    import torch

    from ap_gym_amd import image_env as ie

    pool = host_pool(fmt, hw)
    if FORMATS[fmt][3]:
        return ie.device_pool_u8_tiled(pool, dev)
    if pool.dtype == np.uint8:
        return ie.device_pool_u8(pool, dev)
    return torch.from_numpy(pool.copy()).to(dev)


def geometry(fmt, hw, sensor, scale):
    return dict(image_size=hw, sensor_size=sensor, sensor_scale=scale, channels=FORMATS[fmt][1], tiled=FORMATS[fmt][3])


def positions_for(rng, m, k, dtype, hw, sensor, scale):
    """Random positions over the valid range with its four corners and the centre among them (as many as fit).  The
    range is [-1, 1]^2 for square sensors; the reference's position limit pairs x with sensor_size[0], so a non-square
    sensor leaves the image before |x| or |y| reaches 1, and the range is cut to what stays inside."""
    from oracle import image_oracle as io

    lim = io.sensor_pos_lim(hw, sensor, scale)  # (x, y)
    reach = np.array([(hw[1] - 1) / 2 - (sensor[1] - 1) / 2 * scale, (hw[0] - 1) / 2 - (sensor[0] - 1) / 2 * scale])
    ext = np.where(reach >= lim, 1.0, reach / np.maximum(lim, 1e-300) * (1 - 1e-12))
    pos = rng.uniform(-1, 1, (m, k, 2)) * ext
    special = np.array([(1, 1), (1, -1), (-1, 1), (-1, -1), (0, 0)], np.float64) * ext
    flat = pos.reshape(-1, 2)
    n = min(len(flat), len(special))
    flat[len(flat) - n:] = special[:n] if len(flat) >= 5 else special[[1]]
    out = pos.astype(dtype)
    over = np.abs(out.astype(np.float64)) > np.abs(pos)  # float32 rounding must not step over the range
    out[over] = np.nextafter(out[over], dtype(0))
    return out


def run_three_ways(ap, dev, fmt, hw, sensor, scale, index, pos, observed):
    """Scores only, glimpses only, both from one launch; returns (scores, glimpses, err bits) after checking that the
    three agree."""
    import torch

    pool = dev_pool(fmt, hw, dev)
    geo = geometry(fmt, hw, sensor, scale)
    idx_t, pos_t, obs_t = (torch.as_tensor(x, device=dev) for x in (index, pos, observed))
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    s_only = ap.image_glimpse_scores(pool, idx_t, pos_t, obs_t, err=err, **geo)
    g_only = ap.image_glimpses_at(pool, idx_t, pos_t, err=err, **geo)
    g_both = torch.full_like(g_only, -7.0)
    s_both = torch.full_like(s_only, -7.0)
    ret = ap.image_glimpse_scores(pool, idx_t, pos_t, obs_t, out=s_both, glimpse_out=g_both, err=err, **geo)
    assert ret is s_both
    s_only, g_only, s_both, g_both = (x.cpu().numpy() for x in (s_only, g_only, s_both, g_both))
    assert np.array_equal(g_only, g_both, equal_nan=True)  # (NaN only where the domain test puts it)
    assert np.array_equal(s_only, s_both, equal_nan=True)
    return s_only, g_only, int(err.item())


# (format, image (H, W), sensor, sensor_scale, (M, K), position dtype): every L boundary of the pairwise sum (< 8, one
# leaf with and without tail, 128 | 129, several leaves, 3072), partial tiles / odd pitch (13 x 17), every pool format,
# workgroups whose units straddle position sets with a ragged last one ((37, 65): 2405 units), both position dtypes
PARITY_CASES = [
    ("u8_grey", (28, 28), (1, 2), 1.0, (1, 1), np.float64),
    ("u8_grey", (28, 28), (1, 7), 0.5, (3, 7), np.float32),
    ("u8_grey", (13, 17), (3, 3), 1.0, (37, 65), np.float64),
    ("u8_grey", (64, 64), (5, 5), 1.0, (37, 65), np.float32),
    ("grey_rgb", (28, 28), (5, 5), 1.0, (37, 65), np.float64),
    ("u8_rgb", (13, 17), (5, 5), 2.0, (3, 7), np.float32),
    ("u8_tiled", (13, 17), (5, 5), 1.0, (37, 65), np.float64),
    ("f32_grey", (28, 28), (8, 16), 1.0, (3, 7), np.float64),
    ("f32_grey", (64, 64), (3, 43), 1.0, (37, 65), np.float32),
    ("u8_rgb", (13, 17), (10, 10), 1.0, (3, 7), np.float64),
    ("f32_rgb", (28, 28), (10, 10), 2.0, (3, 7), np.float32),
    ("u8_tiled", (64, 64), (12, 12), 1.0, (37, 65), np.float64),
    ("grey_rgb", (64, 64), (12, 12), 0.5, (3, 7), np.float32),
    ("u8_tiled", (64, 64), (32, 32), 1.0, (3, 7), np.float64),
    ("f32_rgb", (64, 64), (32, 32), 1.5, (1, 1), np.float64),
    ("u8_rgb", (64, 64), (32, 32), 0.5, (3, 7), np.float32),
]


@pytest.mark.parametrize("fmt,hw,sensor,scale,mk,pdtype", PARITY_CASES,
                         ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}-s{c[2][0]}x{c[2][1]}-x{c[3]}-{c[4][0]}x{c[4][1]}-"
                              f"{np.dtype(c[5]).name}" for c in PARITY_CASES])
def test_scores_and_glimpses_match_the_restatement(gpu, fmt, hw, sensor, scale, mk, pdtype):
    import ap_gym_amd as ap

    m, k = mk
    rng = np.random.default_rng(m * 1000 + k + sensor[0])
    index = rng.integers(0, POOL_LEN, m) if m > 1 else np.array([POOL_LEN - 1])  # duplicates, any order
    pos = positions_for(rng, m, k, pdtype, hw, sensor, scale)
    c = FORMATS[fmt][1]
    g_ref, bad = glimpses_np(host_pool(fmt, hw), c, index, pos, sensor, scale)
    assert not bad.any()
    # what a template search compares with: a glimpse of the same image elsewhere
    observed = glimpses_np(host_pool(fmt, hw), c, index, positions_for(rng, m, 6, np.float64, hw, sensor, scale)[:, :1],
                           sensor, scale)[0][:, 0]
    s_ref = glimpse_scores_np(g_ref, observed)
    assert g_ref.shape == (m, k, *sensor, c) and (s_ref > 0).all()
    s, g, err = run_three_ways(ap, gpu, fmt, hw, sensor, scale, index, pos, observed)
    assert err == 0
    assert g.dtype == F and np.array_equal(g, g_ref)
    assert s.dtype == F and np.array_equal(s, s_ref)


def test_exact_pixel_grid_positions(gpu):
    """13 x 17 with a 3 x 3 sensor: positions (i / 7, j / 5) put the sampling points on (or within an ulp of) pixel
    centres, where a bilinear weight is exactly 0 or the interval index is decided by the last bit."""
    import ap_gym_amd as ap

    hw, sensor = (13, 17), (3, 3)
    grid = np.array([(i / 7, j / 5) for i in range(-7, 8) for j in range(-5, 6)])  # 165 positions
    pos = grid.reshape(3, 55, 2)
    index = np.array([4, 0, 4])
    for fmt in ("u8_grey", "u8_tiled"):
        c = FORMATS[fmt][1]
        g_ref, bad = glimpses_np(host_pool(fmt, hw), c, index, pos, sensor, 1.0)
        assert not bad.any()
        observed = g_ref[:, 27].copy()
        s_ref = glimpse_scores_np(g_ref, observed)
        s, g, err = run_three_ways(ap, gpu, fmt, hw, sensor, 1.0, index, pos, observed)
        assert err == 0 and np.array_equal(g, g_ref) and np.array_equal(s, s_ref)
        assert (s[:, 27] == 0.0).all()


def test_exact_zero_and_nan_observed(gpu):
    import ap_gym_amd as ap

    fmt, hw, sensor = "u8_tiled", (64, 64), (12, 12)
    rng = np.random.default_rng(5)
    m, k = 3, 7
    index = np.array([2, 2, 5])
    pos = rng.uniform(-1, 1, (m, k, 2))
    g_ref, _ = glimpses_np(host_pool(fmt, hw), 3, index, pos, sensor, 1.0)
    own = np.array([6, 0, 3])
    observed = g_ref[np.arange(m), own].copy()  # candidate own[m]'s glimpse
    s, g, err = run_three_ways(ap, gpu, fmt, hw, sensor, 1.0, index, pos, observed)
    s_ref = glimpse_scores_np(g_ref, observed)
    assert err == 0 and np.array_equal(s, s_ref)
    assert (s[np.arange(m), own] == 0.0).all() and (np.delete(s[0], 6) > 0).all()
    observed[1, 4, 5, 1] = np.nan  # a NaN in observed[1]: row 1 is NaN, the others are untouched
    s2, g2, err = run_three_ways(ap, gpu, fmt, hw, sensor, 1.0, index, pos, observed)
    assert err == 0 and np.isnan(s2[1]).all() and np.array_equal(s2[[0, 2]], s_ref[[0, 2]])
    assert np.array_equal(g2, g_ref)


@pytest.mark.parametrize("fmt,hw,sensor", [("u8_grey", (13, 17), (3, 3)), ("u8_tiled", (64, 64), (12, 12)),
                                           ("f32_rgb", (28, 28), (5, 5))])
def test_domain_positions_and_indices(gpu, fmt, hw, sensor):
    """Positions outside the image, non-finite ones and indices outside the pool are specified behaviour: NaN units,
    the error bits, every other unit untouched (the addressing of such a unit never uses its own position or index)."""
    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    rng = np.random.default_rng(9)
    m, k = 4, 9
    c = FORMATS[fmt][1]
    pos = rng.uniform(-1, 1, (m, k, 2))
    pos[0, 1] = (1.5, 0)
    pos[0, 4] = (0, -2)
    pos[1, 0] = (np.nan, 0)
    pos[1, 8] = (np.inf, np.inf)
    pos[2, 3] = (0.25, 1e300)
    index = np.array([3, 1, 0, 5])
    observed = glimpses_np(host_pool(fmt, hw), c, index, np.zeros((m, 1, 2)), sensor, 1.0)[0][:, 0]

    def check(index, pos, want_bits):
        g_ref, bad = glimpses_np(host_pool(fmt, hw), c, index, pos, sensor, 1.0)
        s_ref = glimpse_scores_np(g_ref, observed)
        s, g, err = run_three_ways(ap, gpu, fmt, hw, sensor, 1.0, index, pos, observed)
        assert err == want_bits
        nan_units = bad.any(-1)
        assert np.array_equal(np.isnan(s), nan_units) and np.array_equal(np.isnan(g).all((-3, -2, -1)), nan_units)
        assert np.array_equal(np.isnan(g).any((-3, -2, -1)), nan_units)
        assert np.array_equal(s, s_ref, equal_nan=True) and np.array_equal(g, g_ref, equal_nan=True)
        return bad

    bad = check(index, pos, N.APG_ERR_OOB_X | N.APG_ERR_OOB_Y)
    assert bad[..., :2].any(-1).sum() == 5
    one = rng.uniform(-1, 1, (m, k, 2))
    one[3, 8] = (1.5, 0)
    check(index, one, N.APG_ERR_OOB_X)
    one[3, 8] = (0, -2)
    check(index, one, N.APG_ERR_OOB_Y)
    one[3, 8] = (0, 0)
    check(index, one, 0)
    bad = check(np.array([3, -1, POOL_LEN, 5]), one, N.APG_ERR_INDEX)
    assert bad[[1, 2], :, 2].all() and not bad[[0, 3]].any()
    check(np.array([-1, 1, 0, POOL_LEN]), pos, N.APG_ERR_INDEX | N.APG_ERR_OOB_X | N.APG_ERR_OOB_Y)


# ------------------------------------------------------------------------------------------------ tied to the product
STEP_LIMIT, N_ENVS, N_STEPS = 4, 64, 6
PRODUCT = {  # MNIST-shaped; TinyImageNetLoc-shaped (RGB u8 64 x 64: the tiled pool).  sensor_scale 3 keeps the
    # oracle's uniqueness ranking of the localization reset at 36 grid points.
    "cls": dict(shape=(28, 28), sensor=(5, 5), scale=1.0, k=10),
    "loc": dict(shape=(64, 64, 3), sensor=(10, 10), scale=3.0, k=10)}


def _product_inputs(kind):
    p = PRODUCT[kind]
    rng = np.random.default_rng(len(kind) + 40)
    pool = rng.integers(0, 256, (300, *p["shape"]), dtype=np.uint8)
    labels = rng.integers(0, p["k"], 300)
    arng = np.random.default_rng(3)
    acts = arng.uniform(-1.5, 1.5, (N_STEPS + 2, N_ENVS, 2)).astype(F)
    preds = (arng.standard_normal((N_STEPS, N_ENVS, p["k"])) if kind == "cls"
             else arng.uniform(-1, 1, (N_STEPS, N_ENVS, 2))).astype(F)
    return pool, labels, acts, preds


@functools.lru_cache(maxsize=None)
def oracle_trace(kind):
    """reset(seed) and N_STEPS steps of ImageVectorEnvOracle, computed once for both array backends."""
    from oracle import image_oracle as io

    p = PRODUCT[kind]
    pool, labels, acts, preds = _product_inputs(kind)
    c = 1 if len(p["shape"]) == 2 else 3
    ref = io.ImageVectorEnvOracle(kind, pool, labels, p["k"], c, N_ENVS, p["sensor"], p["scale"], STEP_LIMIT,
                                  log_stats=False)
    out = [ref.reset(11)]
    for t in range(N_STEPS):
        obs, reward, term, trunc, info = ref.step(acts[t], preds[t])
        out.append((dict(obs), reward, term, trunc, {"index": info["index"].copy(), "base_reward": info["base_reward"],
                                                      "prediction": dict(info["prediction"])}))
    return out


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


@pytest.mark.parametrize("backend", ["numpy", "torch"])
@pytest.mark.parametrize("kind", ["cls", "loc"])
def test_env_methods_equal_the_steps_they_predict(gpu, kind, backend):
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    p = PRODUCT[kind]
    pool, labels, acts, preds = _product_inputs(kind)
    c = 1 if len(p["shape"]) == 2 else 3
    ds = ap.ArrayImageClassificationDataset(pool, labels, p["k"], c)
    cfg = ap.ImagePerceptionConfig(dataset=ds, sensor_size=p["sensor"], sensor_scale=p["scale"], step_limit=STEP_LIMIT)
    env = (ap.ImageClassificationVectorEnv if kind == "cls" else ap.ImageLocalizationVectorEnv)(
        N_ENVS, cfg, array_backend=backend)
    assert env._cfg.pool_dtype == (N.APG_POOL_U8 if kind == "cls" else N.APG_POOL_U8_TILED)
    trace = oracle_trace(kind)
    n, gshape = N_ENVS, (*p["sensor"], c)

    def give(x):  # an argument in the backend's own form
        return x if backend == "numpy" else torch.as_tensor(x, device=gpu)

    def state():
        return ({k: v.clone() for k, v in env._t.items() if isinstance(v, torch.Tensor) and k != "pool"},
                (env._t_step, env._prev_done, env._ahead))

    def queries(obs, point):
        """Every new method at this point of the episode; returns the lookahead (candidate 1 = the next two real
        actions) after checking that nothing in the env changed."""
        before = state()
        assert np.array_equal(_np(env.glimpses_at()), _np(obs["glimpse"]))
        own = env._t["pos"].cpu().numpy()
        if kind == "loc":
            target = env._t["target"].cpu().numpy()
            assert target.dtype == F
            assert np.array_equal(_np(env.glimpses_at(give(target))), _np(obs["target_glimpse"]))
            sc = _np(env.glimpse_scores(give(target[:, None])))
        else:
            sc = _np(env.glimpse_scores(give(own[:, None])))
        assert sc.shape == (n, 1) and sc.dtype == F and (sc == 0.0).all()
        ids = np.array([5, 63, 5, 0])
        sub = _np(env.glimpses_at(give(own[ids][:, None].repeat(2, 1)), env_ids=ids))
        assert sub.shape == (4, 2, *gshape) and np.array_equal(sub[:, 1], _np(obs["glimpse"])[ids])
        cand = np.random.default_rng(point).uniform(-1.5, 1.5, (n, 3, 2, 2)).astype(F)
        cand[:, 1, 0], cand[:, 1, 1] = acts[point], acts[point + 1]
        la = {k: _np(v) for k, v in env.lookahead(give(cand), glimpses="all").items()}
        last = _np(env.lookahead(give(cand))["glimpse"])
        assert np.array_equal(last, la["glimpse"][:, :, -1])
        assert "glimpse" not in env.lookahead(give(cand), glimpses=None)
        after = state()
        assert before[1] == after[1]
        for k, v in before[0].items():
            assert torch.equal(v, after[0][k]), (point, k)
        # steps / terminated across the step limit; what is not applied repeats the pose with base reward 0
        pending = env._prev_done
        left = STEP_LIMIT - env._t_step
        steps = 2 if pending else min(2, left)
        assert la["pending_reset"].shape == (n,) and (la["pending_reset"] == pending).all()
        assert la["steps"].dtype == np.int32 and (la["steps"] == steps).all()
        assert la["terminated"].dtype == np.bool_ and (la["terminated"] == ((not pending) and steps >= left)).all()
        assert la["pos"].dtype == np.float64 and la["pos"].shape == (n, 3, 2, 2)
        assert la["glimpse"].shape == (n, 3, 2, *gshape)
        want = move_positions_np(own, cand, np.ones(2) * 0.2, max_steps=steps)
        for key, w in zip(("pos", "glimpse_pos", "base_reward"), want):
            assert np.array_equal(la[key], w), (point, key)
        if steps == 1:
            assert np.array_equal(la["pos"][:, :, 1], la["pos"][:, :, 0]) and (la["base_reward"][:, :, 1] == 0).all()
            assert np.array_equal(la["glimpse"][:, :, 1], la["glimpse"][:, :, 0])
        la["applied"] = 0 if pending else steps
        return la

    def same_as_oracle(got, want, t):
        for key in want[0]:
            assert np.array_equal(_np(got[0][key]), want[0][key]), (t, key)
        if len(want) == 2:
            assert np.array_equal(_np(got[1]["index"]), want[1]["index"])
            return
        for i in (1, 2, 3):
            assert np.array_equal(_np(got[i]), want[i]), (t, i)
        gi, wi = got[4], want[4]
        assert np.array_equal(_np(gi["index"]), wi["index"])
        assert np.array_equal(_np(gi["base_reward"]), wi["base_reward"]), t
        for key in ("target", "loss"):
            assert np.array_equal(_np(gi["prediction"][key]), wi["prediction"][key]), (t, key)

    got = env.reset(seed=11)
    same_as_oracle(got, trace[0], 0)
    looks = [queries(got[0], 0)]
    compared = 0
    for t in range(N_STEPS):
        got = env.step({"action": give(acts[t]), "prediction": give(preds[t])})
        same_as_oracle(got, trace[t + 1], t + 1)  # the queries between the steps perturbed nothing
        obs, info = got[0], got[4]
        for back in (1, 2):  # the lookahead taken `back` steps ago predicted this step as its action back - 1
            if t + 1 - back < 0:
                continue
            la, j = looks[t + 1 - back], back - 1
            if j >= la["applied"]:
                continue
            assert np.array_equal(la["pos"][:, 1, j], env._t["pos"].cpu().numpy()), (t, back)
            assert np.array_equal(la["glimpse_pos"][:, 1, j], _np(obs["glimpse_pos"])), (t, back)
            assert np.array_equal(la["base_reward"][:, 1, j], _np(info["base_reward"])), (t, back)
            assert np.array_equal(la["glimpse"][:, 1, j], _np(obs["glimpse"])), (t, back)
            compared += 1
        looks.append(queries(obs, t + 1))
    # steps 1-4 of the first episode are predicted by one or two lookaheads each, step 5 is the autoreset, step 6
    # by the lookahead after it
    assert compared == 4 + 3 + 1
    assert [la["applied"] for la in looks] == [2, 2, 2, 1, 0, 2, 2]
    env.check_errors()
    env.close()


@pytest.mark.parametrize("backend", ["numpy", "torch"])
def test_env_methods_raise_through_check_errors(gpu, backend):
    import torch

    import ap_gym_amd as ap

    pool, labels, _, _ = _product_inputs("cls")
    ds = ap.ArrayImageClassificationDataset(pool, labels, 10, 1)
    env = ap.ImageClassificationVectorEnv(8, ap.ImagePerceptionConfig(dataset=ds, step_limit=STEP_LIMIT),
                                          array_backend=backend)
    obs, _ = env.reset(seed=1)
    first = _np(obs["glimpse"]).copy()

    def raises(exc, match, call):
        with pytest.raises(exc, match=match):
            call()
            env.check_errors()  # torch backend: lazily
        env.check_errors()  # (the bits are cleared by the raise)

    pos = np.zeros((8, 2, 2))
    pos[3, 1] = (1.5, 0)
    raises(ValueError, "out of bounds in dimension 1", lambda: env.glimpses_at(pos))
    pos[3, 1] = (0, np.nan)
    raises(ValueError, "out of bounds in dimension 0", lambda: env.glimpse_scores(pos))
    raises(IndexError, "env id", lambda: env.glimpses_at(env_ids=[0, 8]))
    raises(IndexError, "env id", lambda: env.glimpse_scores(pos[:2, :1] * 0, env_ids=[-1, 2]))
    raises(IndexError, "env id", lambda: env.lookahead(np.zeros((1, 2, 2), F), env_ids=[9], glimpses=None))
    act = np.zeros((8, 2, 3, 2), F)
    act[2, 1, 1, 0] = np.nan
    raises(ValueError, "NaN values detected in action", lambda: env.lookahead(act, glimpses=None))
    with pytest.raises(ValueError, match="one set per chosen sub-env"):
        env.glimpses_at(pos[:3])
    with pytest.raises(ValueError, match="glimpses must be"):
        env.lookahead(act, glimpses="first")
    # the env still steps as before
    got = env.step({"action": np.zeros((8, 2), F), "prediction": np.zeros((8, 10), F)})
    assert np.array_equal(_np(got[0]["glimpse"]), first)  # (a zero action: the same glimpse)
    env.check_errors()
    env.close()


# ------------------------------------------------------------------------------------------------------------ move
@pytest.mark.parametrize("t", [1, 2, 17])
def test_move_matches_the_restatement(gpu, t):
    import torch

    import ap_gym_amd as ap

    rng = np.random.default_rng(t)
    m, k = 5, 6
    pos = rng.uniform(-1, 1, (m, 2))
    pos[0] = (0.95, -0.99)  # drives into the clip
    pos[1] = (-1.0, 1.0)
    act = rng.uniform(-1, 1, (m, k, t, 2)).astype(F)
    act[:, 0] *= F(0.3)                      # norm < 1
    act[:, 1] = rng.uniform(1.0, 1.5, (m, t, 2)).astype(F) * np.where(rng.random((m, t, 2)) < 0.5, -1, 1)  # > 1
    act[:, 2, :, 0], act[:, 2, :, 1] = 1.0, 0.0   # == 1
    act[:, 3] = 0.0                          # zero actions
    act[0, 4, :, 0], act[0, 4, :, 1] = 1.2, -1.2  # into the corner
    msl = (0.2, 0.35)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    for max_steps in sorted({0, 1, t, None}, key=lambda v: -1 if v is None else v):
        res = ap.image_move_positions(torch.as_tensor(pos, device=gpu), torch.as_tensor(act, device=gpu),
                                      max_step_length=msl, max_steps=max_steps, err=err)
        want = move_positions_np(pos, act, msl, max_steps)
        for got, w, dt in zip(res, want, (np.float64, F, F)):
            got = got.cpu().numpy()
            assert got.dtype == dt and np.array_equal(got, w), max_steps
        if max_steps == 0:
            assert np.array_equal(res.pos.cpu().numpy(), np.broadcast_to(pos[:, None, None], (m, k, t, 2)))
    assert (np.abs(want[0]) == 1.0).any() and int(err.item()) == 0
    # one scalar max_step_length is broadcast like the config's
    res = ap.image_move_positions(torch.as_tensor(pos, device=gpu), torch.as_tensor(act, device=gpu),
                                  max_step_length=0.2)
    assert np.array_equal(res.pos.cpu().numpy(), move_positions_np(pos, act, 0.2)[0])


def test_move_nan_action(gpu):
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    rng = np.random.default_rng(0)
    pos = rng.uniform(-1, 1, (3, 2))
    act = rng.uniform(-1, 1, (3, 4, 3, 2)).astype(F)
    act[1, 2, 1, 1] = np.nan  # step 1 of T = 3
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    res = ap.image_move_positions(torch.as_tensor(pos, device=gpu), torch.as_tensor(act, device=gpu),
                                  max_step_length=0.2, err=err)
    want = move_positions_np(pos, act, 0.2)
    for got, w in zip(res, want):
        assert np.array_equal(got.cpu().numpy(), w, equal_nan=True)
    got = res.pos.cpu().numpy()
    assert np.isnan(got[1, 2, 1:]).all() and not np.isnan(got[1, 2, 0]).any() and np.isnan(got).sum() == 4
    assert np.isnan(res.base_reward.cpu().numpy()).sum() == 2
    assert int(err.item()) == N.APG_ERR_NAN_ACTION
