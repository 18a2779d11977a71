"""Host-side pieces of the image envs' glimpses / match scores / moves at chosen positions (ap_gym_amd.glimpse_poses):
the numpy restatements the GPU tests compare against, built only from oracle/image_oracle.py, and the argument checks
of the three public functions (raised on CPU tensors, before anything touches a device)."""

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from oracle import image_oracle as io

F = np.float32
# every L = s0 * s1 * C the GPU tests use, as (s0, s1, C)
L_SHAPES = [(1, 2, 1), (1, 7, 1), (3, 3, 1), (5, 5, 3), (8, 16, 1), (3, 43, 1), (10, 10, 3), (12, 12, 3), (32, 32, 3),
            (5, 5, 1)]


def glimpses_np(pool, channels, index, positions, sensor, scale):
    """Glimpses f32 [M, K, s0, s1, C] of image_oracle.glimpse at positions [M, K, 2], and the error bits per unit
    (bool [M, K, 3]: out of bounds in dimension 0, in dimension 1, index outside the pool).  A unit outside the domain
    is NaN; the oracle raises for it like the reference (bounds_error=True), so it is evaluated unit by unit only
    where the batch raises."""
    images = io.images_f32(pool, channels)
    index = np.asarray(index)
    positions = np.asarray(positions)
    m, k = positions.shape[:2]
    ok_idx = (index >= 0) & (index < len(images))
    imgs = images[np.where(ok_idx, index, 0)]
    bad = np.zeros((m, k, 3), bool)
    bad[..., 2] = ~ok_idx[:, None]
    try:
        g = io.glimpse(imgs, positions, sensor, scale)
    except ValueError:
        g = np.full((m, k, sensor[0], sensor[1], imgs.shape[-1]), np.nan, F)
        for i in range(m):
            for j in range(k):
                try:
                    g[i, j] = io.glimpse(imgs[i:i + 1], positions[i:i + 1, j], sensor, scale)[0]
                except ValueError:
                    # which dimension: the oracle reports the first; probe each with the other coordinate centred
                    for d, probe in ((0, (0.0, positions[i, j, 1])), (1, (positions[i, j, 0], 0.0))):
                        try:
                            io.glimpse(imgs[i:i + 1], np.array([probe]), sensor, scale)
                        except ValueError:
                            bad[i, j, d] = True
    g[bad[..., 2]] = np.nan
    return g, bad


def glimpse_scores_np(g, observed):
    """np.mean((g - observed[:, None]) ** 2, axis=(-3, -2, -1)) in float32 as numpy evaluates it on a contiguous
    block: g f32 [M, K, s0, s1, C], observed f32 [M, s0, s1, C] -> f32 [M, K] (image_oracle.uniqueness's
    expression)."""
    g = np.asarray(g, F)
    o = np.asarray(observed, F)
    m, k = g.shape[:2]
    l = int(np.prod(g.shape[2:]))
    with np.errstate(invalid="ignore"):
        d = (g.reshape(m, k, l) - o.reshape(m, 1, l)) ** 2
        return (F(0) + io.pairwise_sum_f32(d)) / F(l)


def move_positions_np(pos, actions, msl, max_steps=None):
    """ImagePerceptionModule.step's move applied open-loop: pos f64 [M, 2], actions f32 [M, K, T, 2] -> pos f64
    [M, K, T, 2], glimpse_pos f32, base_reward f32 [M, K, T].  After max_steps actions the position repeats and the
    base reward is 0; a NaN action gives NaN from that action on."""
    actions = np.asarray(actions, F)
    m, k, t = actions.shape[:3]
    msl = np.ones(2) * np.asarray(msl, np.float64)
    max_steps = t if max_steps is None else max_steps
    p = np.broadcast_to(np.asarray(pos, np.float64)[:, None, :], (m, k, 2)).copy()
    out = np.empty((m, k, t, 2), np.float64)
    base = np.zeros((m, k, t), F)
    nan = np.zeros((m, k), bool)
    for s in range(t):
        if s < max_steps:
            a = actions[:, :, s]
            nan |= np.isnan(a).any(-1)
            with np.errstate(invalid="ignore"):
                p = np.clip(p + msl * io.project_sphere(a), -1, 1)
                base[:, :, s] = -np.linalg.norm(a, axis=-1) * 1e-3
        p[nan] = np.nan
        base[nan, s] = np.nan
        out[:, :, s] = p
    return out, out.astype(F), base


@pytest.mark.parametrize("shape", L_SHAPES)
def test_glimpse_scores_np_is_numpys_own_mean(shape):
    """The restatement equals numpy's own evaluation on contiguous float32 blocks for every L the GPU tests use."""
    rng = np.random.default_rng(sum(shape))
    m, k = 5, 9
    g = rng.uniform(0, 1, (m, k, *shape)).astype(F)
    o = rng.uniform(0, 1, (m, *shape)).astype(F)
    g[2, 3] = o[2]
    want = np.empty((m, k), F)
    for i in range(m):
        block = np.ascontiguousarray(g[i])
        want[i] = np.mean((block - o[i]) ** 2, axis=(-3, -2, -1))
        assert want[i].dtype == F
    got = glimpse_scores_np(g, o)
    assert got.dtype == F and np.array_equal(got, want)
    assert got[2, 3] == 0.0
    o[1, 0, 0, 0] = np.nan
    got = glimpse_scores_np(g, o)
    assert np.isnan(got[1]).all() and np.array_equal(np.delete(got, 1, 0), np.delete(want, 1, 0))


def test_glimpses_np_marks_the_domain():
    rng = np.random.default_rng(0)
    pool = rng.integers(0, 256, (4, 13, 17, 1), dtype=np.uint8)
    pos = np.array([[[0.0, 0.0], [1.5, 0.0], [0.0, -2.0], [np.nan, 0.0]], [[1.0, 1.0], [np.inf, np.inf], [1e300, 0], [-1, 1]]])
    g, bad = glimpses_np(pool, 1, [3, 7], pos, (3, 3), 1.0)
    assert np.array_equal(bad[0], [[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0]])
    assert bad[1, :, 2].all() and np.isnan(g[1]).all()
    assert np.isnan(g[0, 1:]).all() and not np.isnan(g[0, 0]).any()
    assert np.array_equal(g[0, 0], io.glimpse(io.images_f32(pool, 1)[3:4], pos[0:1, 0], (3, 3), 1.0)[0])


def test_move_positions_np_matches_the_oracle_env_step():
    rng = np.random.default_rng(1)
    pos = rng.uniform(-1, 1, (6, 2))
    a = rng.uniform(-1.5, 1.5, (6, 1, 3, 2)).astype(F)
    out, gp, base = move_positions_np(pos, a, 0.2, max_steps=2)
    p = pos
    for s in range(2):
        p = np.clip(p + np.ones(2) * 0.2 * io.project_sphere(a[:, 0, s]), -1, 1)
        assert np.array_equal(out[:, 0, s], p) and np.array_equal(gp[:, 0, s], p.astype(F))
        assert np.array_equal(base[:, 0, s], (-np.linalg.norm(a[:, 0, s], axis=-1) * 1e-3).astype(F))
    assert np.array_equal(out[:, 0, 2], p) and (base[:, 0, 2] == 0).all()


# ---------------------------------------------------------------------------------------------- argument checks
def _args(m=2, k=3, h=13, w=17, pc=1, dtype="u8"):
    import torch

    pool = (torch.zeros((4, h, w, pc), dtype=torch.uint8) if dtype == "u8"
            else torch.zeros((4, h, w, pc), dtype=torch.float32))
    return pool, torch.zeros(m, dtype=torch.int64), torch.zeros((m, k, 2), dtype=torch.float64)


GEO = dict(image_size=(13, 17), sensor_size=(3, 3), channels=1)


def test_glimpses_at_argument_checks():
    import torch

    import ap_gym_amd as ap

    pool, index, pos = _args()
    with pytest.raises(ValueError, match="no CPU fallback"):
        ap.image_glimpses_at(pool, index, pos, **GEO)
    with pytest.raises(TypeError, match="pool must be a uint8 or float32"):
        ap.image_glimpses_at(pool.double(), index, pos, **GEO)
    with pytest.raises(TypeError, match="index must be"):
        ap.image_glimpses_at(pool, index.int(), pos, **GEO)
    with pytest.raises(TypeError, match="positions must be"):
        ap.image_glimpses_at(pool, index, pos.half(), **GEO)
    with pytest.raises(ValueError, match=r"positions must have shape \[M, K, 2\]"):
        ap.image_glimpses_at(pool, index, pos[:, 0], **GEO)
    with pytest.raises(ValueError, match="one pool image per position set"):
        ap.image_glimpses_at(pool, index[:1], pos, **GEO)
    with pytest.raises(ValueError, match="pool must have shape"):
        ap.image_glimpses_at(pool, index, pos, **{**GEO, "image_size": (17, 13)})
    with pytest.raises(ValueError, match="Target channels must be either 1 or 3"):
        ap.image_glimpses_at(pool, index, pos, **{**GEO, "channels": 2})
    with pytest.raises(ValueError, match="Expected 1 channels but got 3"):
        ap.image_glimpses_at(_args(pc=3)[0], index, pos, **GEO)
    with pytest.raises(ValueError, match="sensor sides must be in 1..256"):
        ap.image_glimpses_at(pool, index, pos, **{**GEO, "sensor_size": (257, 1)})
    with pytest.raises(ValueError, match="at most 16384 values"):
        ap.image_glimpses_at(pool, index, pos, **{**GEO, "sensor_size": (128, 129)})
    with pytest.raises(ValueError, match="too many pixels"):
        ap.image_glimpses_at(pool, torch.zeros(2**20, dtype=torch.int64).expand(2**20),
                             torch.zeros(1, dtype=torch.float64).expand(2**20, 2**8, 2), **GEO)
    with pytest.raises(ValueError, match="sensor_scale must be positive"):
        ap.image_glimpses_at(pool, index, pos, sensor_scale=0.0, **GEO)
    with pytest.raises(ValueError, match="a tiled pool is the flat uint8"):
        ap.image_glimpses_at(pool, index, pos, tiled=True, **{**GEO, "channels": 3})
    with pytest.raises(ValueError, match="a multiple of 1536 bytes"):
        ap.image_glimpses_at(torch.zeros(1000, dtype=torch.uint8), index, pos, tiled=True, **{**GEO, "channels": 3})
    with pytest.raises(TypeError, match="out must be a float32"):
        ap.image_glimpses_at(pool, index, pos, out=torch.zeros((2, 3, 3, 3, 1), dtype=torch.float64), **GEO)
    with pytest.raises(ValueError, match="out must have shape"):
        ap.image_glimpses_at(pool, index, pos, out=torch.zeros((2, 3, 3, 3, 3)), **GEO)


def test_glimpse_scores_argument_checks():
    import torch

    import ap_gym_amd as ap

    pool, index, pos = _args()
    obs = torch.zeros((2, 3, 3, 1))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ap.image_glimpse_scores(pool, index, pos, obs, **GEO)
    with pytest.raises(TypeError, match="observed must be a float32"):
        ap.image_glimpse_scores(pool, index, pos, obs.double(), **GEO)
    with pytest.raises(ValueError, match="observed must have shape"):
        ap.image_glimpse_scores(pool, index, pos, obs[:1], **GEO)
    with pytest.raises(ValueError, match="out must have shape"):
        ap.image_glimpse_scores(pool, index, pos, obs, out=torch.zeros((2, 4)), **GEO)
    with pytest.raises(ValueError, match="glimpse_out must have shape"):
        ap.image_glimpse_scores(pool, index, pos, obs, glimpse_out=torch.zeros((2, 3, 3, 3, 3)), **GEO)
    # the fused score's bound on the glimpse size: 32 x 32 x 3 = 3072 passes it, 37 x 37 x 3 = 4107 does not
    big = dict(image_size=(64, 64), channels=3)
    pool3 = torch.zeros((2, 64, 64, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="image_glimpses_at"):
        ap.image_glimpse_scores(pool3, index, pos, torch.zeros((2, 37, 37, 3)), sensor_size=(37, 37), **big)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ap.image_glimpse_scores(pool3, index, pos, torch.zeros((2, 32, 32, 3)), sensor_size=(32, 32), **big)
    assert ap.glimpse_poses.GLIMPSE_SCORES_MAX_L >= 3072


def test_move_positions_argument_checks():
    import torch

    import ap_gym_amd as ap

    pos, act = torch.zeros((2, 2), dtype=torch.float64), torch.zeros((2, 3, 4, 2))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ap.image_move_positions(pos, act, max_step_length=0.2)
    with pytest.raises(TypeError, match="pos must be a float64"):
        ap.image_move_positions(pos.float(), act, max_step_length=0.2)
    with pytest.raises(TypeError, match="actions must be a float32"):
        ap.image_move_positions(pos, act.double(), max_step_length=0.2)
    with pytest.raises(ValueError, match="pos must have shape"):
        ap.image_move_positions(pos[0], act, max_step_length=0.2)
    with pytest.raises(ValueError, match="actions must have shape"):
        ap.image_move_positions(pos, act[:1], max_step_length=0.2)
    with pytest.raises(ValueError, match="actions must have shape"):
        ap.image_move_positions(pos, act[:, :, 0], max_step_length=0.2)
    with pytest.raises(ValueError, match="T must be in 1..4096"):
        ap.image_move_positions(pos, torch.zeros(1).expand(2, 1, 4097, 2), max_step_length=0.2)
    with pytest.raises(ValueError, match="max_step_length"):
        ap.image_move_positions(pos, act, max_step_length=(0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match="max_steps"):
        ap.image_move_positions(pos, act, max_step_length=0.2, max_steps=-1)
    with pytest.raises(ValueError, match="max_steps"):
        ap.image_move_positions(pos, act, max_step_length=0.2, max_steps=1.5)
