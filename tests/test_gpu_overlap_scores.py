"""k_overlap_scores (ap_gym_amd.image_overlap_scores, env.target_overlap, ImageTargetBelief) against the numpy
restatement of tests/test_overlap_scores_host.py: sse, count and the fused log-weights bit for bit."""

import numpy as np
import pytest

from test_overlap_scores_host import F, check_noise_sweep, noise_case, overlap_scores_np

pytestmark = pytest.mark.gpu

# (sensor s0, s1, C) -> image (H, W) with lim_x = (W - s0) / 2 and lim_y = (H - s1) / 2 powers of two, so the shifts of
# positions on a dyadic grid are exact (integers, +-(s - 1), halves); 3 x 7 sits on a non-square image and pins the
# x <-> sensor_size[0] pairing
SHAPES = {(1, 1, 1): (9, 17), (5, 5, 1): (21, 37), (3, 7, 1): (23, 35), (12, 12, 3): (76, 44), (64, 64, 1): (80, 96)}


def lims(shape):
    h, w = SHAPES[shape]
    return np.array([(w - shape[0]) / 2, (h - shape[1]) / 2])  # (x, y)


def make_case(shape, m, k, pdtype, seed, bad_q=False):
    """g, G, q, h with every kind of shift mixed into every set (by hypothesis index modulo 16), set 0 on a dyadic grid
    so that its constructed shifts are exact."""
    rng = np.random.default_rng(seed)
    s0, s1, c = shape
    lim = lims(shape)
    g = rng.random((m, s0, s1, c), dtype=F)
    G = rng.random((m, s0, s1, c), dtype=F)
    q = rng.uniform(-1, 1, (m, 2))
    q[0] = rng.integers(-8, 9, 2) / 16
    if bad_q:
        q[m - 1, 0] = np.nan
        if m > 2:
            q[m - 2, 1] = -np.inf
    h = rng.uniform(-1, 1, (m, k, 2))
    size = np.array([s1, s0], np.float64)  # the sensor's length along (x, y)
    for j in range(k):
        kind = j % 16
        if kind == 0:
            d = np.zeros((m, 2))
        elif kind == 1:
            d = np.stack([rng.integers(-(s1 - 1), s1, m), rng.integers(-(s0 - 1), s0, m)], -1).astype(np.float64)
        elif kind in (2, 3, 4):  # fractional shifts of both signs (the floor of a negative)
            d = rng.uniform(-1, 1, (m, 2)) * (size - 0.5) * (0.3 if kind == 2 else 1.0)
        elif kind == 5:
            d = (size - 1) * rng.choice([-1.0, 1.0], (m, 2))  # exactly +-(s - 1): one row / column, f = 0, a clamp
        elif kind == 6:
            d = (size - 1) * np.array([1.0, 0.0]) * rng.choice([-1.0, 1.0], (m, 1)) + np.array([0.0, 0.5])
        elif kind == 7:
            d = (size - 1 + 2.0 ** -10) * rng.choice([-1.0, 1.0], (m, 2))  # just beyond: |d| < s, but no sample
        elif kind == 8:
            d = size * rng.choice([-1.0, 1.0], (m, 2)) * np.array([1.0, 0.0])  # |d| == s
        elif kind == 9:
            d = np.array([0.25, -0.5]) * np.ones((m, 1))
        elif kind == 10:
            d = np.full((m, 2), 1e30)
        else:
            continue  # uniform over the whole range: mostly no overlap
        h[:, j] = q - d / lim
    if k >= 16:  # non-finite hypotheses, a few
        h[:, 11, 0] = np.nan
        h[m - 1, 12, 1] = np.inf
    return g, G, q.astype(pdtype), h.astype(pdtype)


def run(dev, shape, g, G, q, h, logw=None, gain=0.0, tau=0.0, logw_out=None):
    import torch

    import ap_gym_amd as ap

    t = lambda x: None if x is None else torch.as_tensor(x, device=dev)  # noqa: E731
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    res = ap.image_overlap_scores(t(g), t(q), t(G), t(h), image_size=SHAPES[shape], sensor_size=shape[:2], logw=t(logw),
                                  gain=gain, tau=tau, logw_out=logw_out, err=err)
    return res, int(err.item())


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want) if want.dtype.kind == "f" else np.zeros(want.shape, bool)
    assert np.array_equal(np.isnan(got) if want.dtype.kind == "f" else nan, nan), what
    view = np.uint32 if want.dtype.itemsize == 4 else np.uint64
    bad = (got.view(view) != want.view(view)) & ~nan
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


def chunk_ks(m):
    from ap_gym_amd import _native as N

    ks = {1, 1000, 4096}
    for k in (8, 64):  # the chunk the launch of (m, k) resolves to, and its neighbours
        c = N.overlap_scores_chunk(m, k)
        ks |= {c - 1, c, c + 1}
    return sorted(ks)


PARITY = [(shape, m, pd) for shape in SHAPES for m, pd in ((1, np.float64), (3, np.float32))]


@pytest.mark.parametrize("shape,m,pdtype", PARITY,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_scores_match_the_restatement(gpu, shape, m, pdtype):
    from ap_gym_amd import _native as N

    image, L = SHAPES[shape], shape[0] * shape[1] * shape[2]
    ks = chunk_ks(m)
    if L == 4096:  # (the restatement's temporaries are [K, L] arrays)
        ks = [k for k in ks if k != 4096 or m == 1]
    seen = set()
    for k in ks:
        g, G, q, h = make_case(shape, m, k, pdtype, seed=k + 7 * m, bad_q=(m > 1 and k == 1000))
        rng = np.random.default_rng(k)
        logw = rng.standard_normal((m, k)).astype(F)
        gain, tau = F(0.5 / 0.3 ** 2), F(0.02)
        sse, count, lw, bad = overlap_scores_np(g, q, G, h, image, shape[:2], logw=logw, gain=gain, tau=tau)
        res, err = run(gpu, shape, g, G, q, h, logw=logw, gain=float(gain), tau=float(tau))
        same_bits(res.count.cpu().numpy(), count, ("count", k))
        same_bits(res.sse.cpu().numpy(), sse, ("sse", k))
        same_bits(res.logw.cpu().numpy(), lw, ("logw", k))
        assert err == (N.APG_ERR_BAD_POSE if bad.any() else 0), k
        assert np.isnan(sse[bad]).all() and not count[bad].any()
        plain, _ = run(gpu, shape, g, G, q, h)  # without the belief update: the same sse / count, no logw
        assert plain.logw is None
        same_bits(plain.sse.cpu().numpy(), sse, ("sse alone", k))
        same_bits(plain.count.cpu().numpy(), count, ("count alone", k))
        # what the mixture is there for: full, partial, single-row and empty overlaps all occur
        seen |= set(np.unique(count).tolist())
        if k >= 16:
            d = ((q[0].astype(np.float64) - h[0].astype(np.float64)) * lims(shape))
            assert d[0, 0] == 0 and d[0, 1] == 0 and count[0, 0] == L
            assert abs(d[5, 0]) == shape[1] - 1 and abs(d[5, 1]) == shape[0] - 1 and count[0, 5] == shape[2]
            assert count[0, 7] == 0 and count[0, 8] == 0 and count[0, 10] == 0 and sse[0, 7] == 0
            assert bad[:, 11].all() and np.isnan(lw[:, 11]).all()
    assert {0, L, shape[2]} <= seen


def test_shared_hypotheses_and_ragged_chunks_of_64(gpu):
    """[K, 2] hypotheses shared by every set; enough sets that the launch keeps chunks of 64 hypotheses."""
    from ap_gym_amd import _native as N

    shape, m = (5, 5, 1), 1100
    for k in (63, 64, 65):
        assert N.overlap_scores_chunk(m, k) == 64
        g, G, q, h = make_case(shape, m, k, np.float32, seed=k)
        h = h[0] + np.float32(0.001)
        logw = np.zeros((m, k), F)
        sse, count, lw, bad = overlap_scores_np(g, q, G, h, SHAPES[shape], shape[:2], logw=logw, gain=F(3), tau=F(0.1))
        res, err = run(gpu, shape, g, G, q, h, logw=logw, gain=3.0, tau=float(F(0.1)))
        same_bits(res.sse.cpu().numpy(), sse, k)
        same_bits(res.count.cpu().numpy(), count, k)
        same_bits(res.logw.cpu().numpy(), lw, k)
        assert err == (N.APG_ERR_BAD_POSE if bad.any() else 0)
        assert (count > 0).any()


def test_nan_in_glimpse_in_place_update_and_repeatability(gpu):
    import torch

    shape, m, k = (12, 12, 3), 2, 200
    g, G, q, h = make_case(shape, m, k, np.float64, seed=5)
    g[0, 3, 4, 1] = np.nan
    g[1, 11, 0, 2] = np.nan
    logw = np.random.default_rng(0).standard_normal((m, k)).astype(F)
    sse, count, lw, _ = overlap_scores_np(g, q, G, h, SHAPES[shape], shape[:2], logw=logw, gain=F(2), tau=F(0.05))
    # the NaN reaches exactly the hypotheses whose overlap holds that sample
    d = (q[:, None, :] - h) * lims(shape)
    for i, (a, b) in enumerate(((3, 4), (11, 0))):
        inside = (0 <= a + d[i, :, 1]) & (a + d[i, :, 1] <= 11) & (0 <= b + d[i, :, 0]) & (b + d[i, :, 0] <= 11)
        inside &= np.isfinite(h[i]).all(-1) & (np.abs(d[i]) < 12).all(-1)
        finite_h = np.isfinite(h[i]).all(-1)
        assert np.array_equal(np.isnan(sse[i])[finite_h], inside[finite_h]) and inside.any() and not inside.all()
    first, _ = run(gpu, shape, g, G, q, h, logw=logw, gain=2.0, tau=float(F(0.05)))
    again, _ = run(gpu, shape, g, G, q, h, logw=logw, gain=2.0, tau=float(F(0.05)))
    for a, b, w in zip(first, again, (sse, count, lw)):
        same_bits(a.cpu().numpy(), w, "first")
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # two launches: equal bits
    own = torch.as_tensor(logw, device=gpu)
    inplace, _ = run(gpu, shape, g, G, q, h, logw=own, gain=2.0, tau=float(F(0.05)), logw_out=own)
    assert inplace.logw is own
    same_bits(own.cpu().numpy(), lw, "in place")


@pytest.mark.parametrize("seed", range(3))
def test_exact_construction_on_the_device(gpu, seed):
    """The noise-image construction of the host test with g and G taken by image_glimpses_at from a uint8 pool."""
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd import image_env as ie

    pool, hyp, target, pos, _ = noise_case(seed)
    geo = dict(image_size=(40, 40), sensor_size=(8, 8))
    dpool = ie.device_pool_u8(pool, gpu)
    index = torch.zeros(1, dtype=torch.int64, device=gpu)
    at = torch.as_tensor(np.concatenate([pos, hyp[target][None]])[None], device=gpu)
    glimpses = ap.image_glimpses_at(dpool, index, at, channels=1, **geo)[0]
    g, G = glimpses[:-1].contiguous(), glimpses[-1:].expand(len(pos), 8, 8, 1).contiguous()
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    logw = torch.zeros((len(pos), len(hyp)), dtype=torch.float32, device=gpu)
    res = ap.image_overlap_scores(g, torch.as_tensor(pos, device=gpu), G, torch.as_tensor(hyp, device=gpu), logw=logw,
                                  gain=1.0, tau=float(F(0.01)), err=err, **geo)
    sse, count = res.sse.cpu().numpy(), res.count.cpu().numpy()
    assert int(err.item()) == 0
    check_noise_sweep(sse, count, target)
    want = overlap_scores_np(g.cpu().numpy(), pos, G.cpu().numpy(), hyp, (40, 40), (8, 8), logw=np.zeros(sse.shape, F),
                             gain=F(1), tau=F(0.01))
    same_bits(sse, want[0], "sse")
    same_bits(count, want[1], "count")
    same_bits(res.logw.cpu().numpy(), want[2], "logw")


# ------------------------------------------------------------------ env method and belief
N_ENVS, STEP_LIMIT, SENSOR, IMAGE = 8, 4, (4, 4), (16, 16)


def small_env(backend, kind="loc", channels=1):
    import ap_gym_amd as ap

    rng = np.random.default_rng(21)
    pool = rng.integers(0, 256, (5, *IMAGE, channels), dtype=np.uint8)
    ds = ap.ArrayImageClassificationDataset(pool if channels == 3 else pool[..., 0], rng.integers(0, 3, 5), 3, channels)
    cfg = ap.ImagePerceptionConfig(dataset=ds, sensor_size=SENSOR, step_limit=STEP_LIMIT)
    cls = ap.ImageLocalizationVectorEnv if kind == "loc" else ap.ImageClassificationVectorEnv
    return cls(N_ENVS, cfg, array_backend=backend)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


@pytest.mark.parametrize("backend", ["numpy", "torch"])
def test_env_target_overlap_equals_the_function_on_the_observation(gpu, backend):
    import torch

    import ap_gym_amd as ap

    env = small_env(backend, channels=3 if backend == "torch" else 1)
    give = (lambda x: x) if backend == "numpy" else (lambda x: torch.as_tensor(x, device=gpu))
    rng = np.random.default_rng(4)
    obs, _ = env.reset(seed=3)
    geo = dict(image_size=IMAGE, sensor_size=SENSOR)
    for t in range(STEP_LIMIT + 2):
        hyp = rng.uniform(-1, 1, (N_ENVS, 40, 2))
        hyp[:, 0] = _np(obs["glimpse_pos"])  # full overlap ...
        hyp[:, 1] = _np(env._t["target"])    # ... and the truth
        logw = rng.standard_normal((N_ENVS, 40)).astype(F)
        res = env.target_overlap(give(hyp), logw=give(logw), gain=1.5, tau=0.01)
        assert type(res.sse) is (np.ndarray if backend == "numpy" else torch.Tensor)
        dev = lambda x: torch.as_tensor(_np(x), device=gpu)  # noqa: E731
        want = ap.image_overlap_scores(dev(obs["glimpse"]), dev(obs["glimpse_pos"]), dev(obs["target_glimpse"]),
                                       dev(hyp), logw=dev(logw), gain=1.5, tau=0.01, **geo)
        for a, b in zip(res, want):
            same_bits(_np(a), _np(b), t)
        assert (_np(res.count)[:, 0] == SENSOR[0] * SENSOR[1] * _np(obs["glimpse"]).shape[-1]).all()
        # a subset of the sub-envs, shared hypotheses, no belief update
        ids = np.array([5, 0, 5])
        sub = env.target_overlap(give(hyp[0]), env_ids=ids)
        assert sub.logw is None and _np(sub.sse).shape == (3, 40)
        want = ap.image_overlap_scores(dev(obs["glimpse"])[ids].contiguous(), dev(obs["glimpse_pos"])[ids].contiguous(),
                                       dev(obs["target_glimpse"])[ids].contiguous(), dev(hyp[0]), **geo)
        same_bits(_np(sub.sse), _np(want.sse), t)
        same_bits(_np(sub.count), _np(want.count), t)
        act = rng.uniform(-1, 1, (N_ENVS, 2)).astype(F)
        obs = env.step({"action": give(act), "prediction": give(np.zeros((N_ENVS, 2), F))})[0]
    # errors: at once on the numpy backend, through check_errors() on the torch backend
    hyp[2, 3, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        env.target_overlap(give(hyp))
        env.check_errors()
    env.check_errors()
    with pytest.raises(ValueError, match="hypotheses must have shape"):
        env.target_overlap(give(hyp[:3]))
    env.close()


def test_classification_env_raises(gpu):
    env = small_env("torch", kind="cls")
    env.reset(seed=0)
    with pytest.raises(TypeError, match="localization env"):
        env.target_overlap(np.zeros((4, 2)))
    import ap_gym_amd as ap

    with pytest.raises(ValueError, match="localization env"):
        ap.ImageTargetBelief(env, sigma=0.1, tau=0.01)
    env.close()


def test_belief_update_reset_and_policy(gpu):
    import torch

    import ap_gym_amd as ap

    env, twin = small_env("torch"), small_env("torch")
    sigma, tau = 0.2, 0.01
    belief = ap.ImageTargetBelief(env, grid=(9, 7), sigma=sigma, tau=tau)
    k = belief.num_hypotheses
    assert k == 63 and tuple(belief.hypotheses.shape) == (N_ENVS, k, 2)
    hyp = belief.hypotheses[0].cpu().numpy()
    assert np.array_equal(hyp[:9, 0], np.linspace(-1, 1, 9, dtype=F)) and np.array_equal(hyp[::9, 1],
                                                                                         np.linspace(-1, 1, 7, dtype=F))
    gain = float(F(1.0 / (2.0 * sigma * sigma)))
    geo = dict(image_size=IMAGE, sensor_size=SENSOR)
    obs, _ = env.reset(seed=9)
    tobs, _ = twin.reset(seed=9)
    belief.reset()
    assert torch.equal(belief.logw, torch.zeros((N_ENVS, k), device=gpu))
    carried = torch.zeros((N_ENVS, k), dtype=torch.float32, device=gpu)
    for t in range(2 * STEP_LIMIT + 3):
        res = belief.update()
        # by hand: the function on the observation, then lidar_pf_resample without resampling
        fresh = t > 0 and (t % (STEP_LIMIT + 1)) == 0  # the step before this update was the batch autoreset
        if fresh:
            carried = torch.zeros_like(carried)
        want = ap.image_overlap_scores(obs["glimpse"].contiguous(), obs["glimpse_pos"].contiguous(),
                                       obs["target_glimpse"].contiguous(), belief.hypotheses[0].contiguous(),
                                       logw=carried, gain=gain, tau=tau, **geo)
        pf = ap.lidar_pf_resample(belief.hypotheses, want.logw, ess_frac=0.0)
        for name, a, b in (("sse", res.sse, want.sse), ("count", res.count, want.count), ("logw", res.logw, want.logw),
                           ("weight", res.weight, pf.weight), ("estimate", res.estimate, pf.estimate),
                           ("ess", res.ess, pf.ess)):
            same_bits(a.cpu().numpy(), b.cpu().numpy(), (t, name))
        if fresh:  # the log-weights started from 0 again: they are this update's increment alone
            zero = ap.image_overlap_scores(obs["glimpse"].contiguous(), obs["glimpse_pos"].contiguous(),
                                           obs["target_glimpse"].contiguous(), belief.hypotheses[0].contiguous(),
                                           logw=torch.zeros_like(carried), gain=gain, tau=tau, **geo)
            assert torch.equal(belief.logw, zero.logw)
        carried = want.logw
        assert torch.equal(belief.prediction, res.estimate)
        lw = belief.logw.cpu().numpy()
        best = hyp[np.argmax(lw, axis=1)]  # (numpy: the first of equals)
        assert np.array_equal(belief.best.cpu().numpy(), best)
        act = belief.choose_action()
        raw = (best - obs["glimpse_pos"].cpu().numpy()) / F(0.2)
        norm = np.maximum(F(1), np.sqrt((raw.astype(np.float64) ** 2).sum(-1)))[:, None]
        assert act.dtype == torch.float32 and tuple(act.shape) == (N_ENVS, 2)
        np.testing.assert_allclose(act.cpu().numpy(), raw / norm, rtol=1e-6, atol=1e-7)
        # stepping with the belief's action equals stepping a twin env with the same numbers passed in by hand
        pred = belief.prediction.clone()
        out = env.step({"action": act, "prediction": pred})
        tout = twin.step({"action": act.clone(), "prediction": pred.clone()})
        for key in out[0]:
            assert torch.equal(out[0][key], tout[0][key]), (t, key)
        for i in (1, 2, 3):
            assert torch.equal(out[i], tout[i]), (t, i)
        assert torch.equal(out[4]["prediction"]["loss"], tout[4]["prediction"]["loss"])
        assert torch.equal(out[4]["prediction"]["target"], tout[4]["prediction"]["target"])
        obs = out[0]
    env.check_errors()
    env.close()
    twin.close()
