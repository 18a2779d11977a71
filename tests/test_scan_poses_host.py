"""lidar_scan_poses / lidar_pose_scores: what needs no GPU -- the numpy restatements over the oracle's segment scan
that tests/test_gpu_scan_poses.py compares the kernel with (themselves checked against the oracle env's own lidar
observation), the argument checks of both public functions and the C ABI's host-side validation (it returns before
any HIP call)."""

import ctypes

import numpy as np
import pytest


def normalize_np(dist, lidar_range):
    """The divide-and-clip of write_obs (oracle/apg_oracle_lidar.c) in float32: distances in cells to the
    observation's values."""
    return np.clip(np.asarray(dist, np.float32) / np.float32(lidar_range), np.float32(-1), np.float32(1))


def scan_poses_np(oracle, maps, poses, dirs, lidar_range, map_ids=None, normalize=True):
    """numpy restatement of apg_lidar_scan_poses' scan output.  maps: bool / uint8 [n_src, H, W]; poses float32
    [M, K, 2]; dirs float32 [B, 2].  Beam b of pose p is p -> (p + dirs[b]).astype(float32), scanned by the oracle's
    restatement of __lidar_scan; normalize: the divide-and-clip of write_obs (oracle/apg_oracle_lidar.c) in float32.
    A pose with a non-finite coordinate gives NaN; a map id outside [0, n_src) an all-zero map."""
    maps = np.asarray(maps).astype(np.uint8)
    poses = np.asarray(poses, dtype=np.float32)
    dirs = np.asarray(dirs, dtype=np.float32)
    n_src, h, w = maps.shape
    m, k, _ = poses.shape
    ids = (np.zeros(m, np.int64) if n_src == 1 else np.arange(m)) if map_ids is None else np.asarray(map_ids)
    empty = np.zeros((h, w), np.uint8)
    out = np.zeros((m, k, len(dirs)), np.float32)
    for i in range(m):
        occ = maps[ids[i]] if 0 <= ids[i] < n_src else empty
        for j in range(k):
            p = poses[i, j]
            if not np.isfinite(p).all():
                out[i, j] = np.nan
                continue
            for b, d in enumerate(dirs):
                q = (p + d).astype(np.float32)
                dist = oracle.lidar_scan(occ, p, q)[0]
                out[i, j, b] = normalize_np(dist, lidar_range) if normalize else dist
    return out


def pose_scores_np(scans, observed):
    """numpy restatement of the score output: scans float32 [M, K, B] (normalised), observed float32 [M, B];
    acc = acc + (s_b - o_b) * (s_b - o_b) in float32, beam order from 0, every operation rounded on its own."""
    scans = np.asarray(scans, dtype=np.float32)
    observed = np.asarray(observed, dtype=np.float32)
    acc = np.zeros(scans.shape[:2], np.float32)
    with np.errstate(invalid="ignore"):
        for b in range(scans.shape[2]):
            e = (scans[:, :, b] - observed[:, None, b]).astype(np.float32)
            acc = (acc + (e * e).astype(np.float32)).astype(np.float32)
    return acc


@pytest.mark.parametrize("kind,size,beams", [("rooms", 32, 8), ("maze", 21, 7)])
def test_restated_scan_equals_the_oracle_envs_observation(oracle_mod, kind, size, beams):
    """The restatement at the oracle env's own positions is its lidar output, after a reset and five steps."""
    n = 6
    env = oracle_mod.OracleLidarVectorEnv(n, map_kind=kind, size=size, beams=beams, lidar_range=5, step_limit=3)
    rng = np.random.default_rng(5)

    def check(where):
        maps = env.map != 0  # the dense observation: 1/255 at walls
        pos = env.state()["pos"]
        got = scan_poses_np(oracle_mod, maps, pos[:, None, :], env.dirs, 5)
        assert np.array_equal(got[:, 0, :].view(np.int32), env.lidar.view(np.int32)), where
        # the true position among three poses: score exactly 0 there, the plain formula elsewhere
        poses = np.stack([pos, pos + np.float32(0.37), pos[::-1]], axis=1).astype(np.float32)
        scans = scan_poses_np(oracle_mod, maps, poses, env.dirs, 5)
        scores = pose_scores_np(scans, env.lidar)
        assert scores.dtype == np.float32 and np.all(scores[:, 0] == 0.0), where
        b0 = (scans[:, 1, 0] - env.lidar[:, 0]) ** 2
        assert np.array_equal(pose_scores_np(scans[:, 1:2, :1], env.lidar[:, :1])[:, 0], b0.astype(np.float32))

    env.reset(11)
    check("reset")
    for t in range(5):
        env.step(rng.uniform(-1, 1, (n, 2)).astype(np.float32), rng.uniform(-1, 1, (n, 2)).astype(np.float32))
        check(f"step {t}")
    env.close()


def test_restatement_conventions(oracle_mod):
    """Non-finite poses are NaN, ids outside the batch an empty map, one map serves every set, raw distances."""
    maps = np.zeros((1, 5, 7), bool)
    maps[0, 2, 4] = True
    dirs = oracle_mod.beam_directions(4, 3)
    poses = np.array([[[1.5, 2.5], [np.nan, 1.0]], [[1.5, 2.5], [np.inf, 0.0]]], np.float32)
    got = scan_poses_np(oracle_mod, maps, poses, dirs, 3, normalize=False)
    assert got.shape == (2, 2, 4) and np.isnan(got[:, 1]).all() and np.array_equal(got[0, 0], got[1, 0])
    assert got[0, 0, 2] < 2.5 and abs(got[0, 0, 0] - 3) < 1e-5  # beam 2 looks along +x into the wall at x = 4
    off = scan_poses_np(oracle_mod, maps, poses[:, :1], dirs, 3, map_ids=[0, 1], normalize=False)
    assert np.array_equal(off[0], got[0, :1]) and np.allclose(off[1], 3, atol=1e-5)
    s = pose_scores_np(np.zeros((1, 2, 3), np.float32), np.array([[0, np.nan, 0]], np.float32))
    assert np.isnan(s).all()


def test_scan_poses_argument_checks():
    """Dtype, rank and shape errors come first, on tensors of any device; the device is refused last."""
    import torch

    import ap_gym_amd as ap

    bits = torch.zeros((3, 4, 2), dtype=torch.int64)
    poses = torch.zeros((3, 5, 2))
    obs = torch.zeros((3, 8))
    kw = dict(beams=8, lidar_range=5)

    def both(exc, match, b=bits, w=70, p=poses, o=obs, ids=None, **over):
        with pytest.raises(exc, match=match):
            ap.lidar_scan_poses(b, w, p, ids, **{**kw, **over})
        with pytest.raises(exc, match=match):
            ap.lidar_pose_scores(b, w, p, o, ids, **{**kw, **over})

    both(TypeError, "int64", b=bits.to(torch.int32))
    both(TypeError, "int64", b=bits[0])
    both(TypeError, "int64", b=bits.numpy())
    both(TypeError, "float32", p=poses.double())
    both(TypeError, "float32", p=poses.numpy())
    both(ValueError, r"\[M, K, 2\]", p=poses[0])
    both(ValueError, r"\[M, K, 2\]", p=torch.zeros((3, 5, 3)))
    both(ValueError, "words per row", w=64)
    both(ValueError, "1..511", b=torch.zeros((3, 4, 8), dtype=torch.int64), w=512)
    both(ValueError, "1..511", b=torch.zeros((3, 0, 2), dtype=torch.int64))
    both(ValueError, "lidar_range", lidar_range=0)
    both(ValueError, "lidar_range", lidar_range=60.5)
    both(ValueError, "beams", beams=0)
    both(ValueError, "beams", beams=4097)
    both(TypeError, "map_ids", ids=torch.zeros(3, dtype=torch.int32))
    both(TypeError, "map_ids", ids=[0, 1, 2])
    both(ValueError, "map_ids", ids=torch.zeros(2, dtype=torch.int64))
    both(ValueError, "without map_ids", p=torch.zeros((2, 5, 2)), o=torch.zeros((2, 8)))
    with pytest.raises(TypeError, match="observed"):
        ap.lidar_pose_scores(bits, 70, poses, obs.double(), **kw)
    for bad in (torch.zeros((3, 7)), torch.zeros((2, 8)), torch.zeros(24)):
        with pytest.raises(ValueError, match="observed"):
            ap.lidar_pose_scores(bits, 70, poses, bad, **kw)
    with pytest.raises(ValueError, match="shape"):
        ap.lidar_scan_poses(bits, 70, poses, out=torch.zeros((3, 5, 7)), **kw)
    with pytest.raises(TypeError, match="float32"):
        ap.lidar_scan_poses(bits, 70, poses, out=torch.zeros((3, 5, 8), dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match="shape"):
        ap.lidar_pose_scores(bits, 70, poses, obs, out=torch.zeros((3, 5, 1)), **kw)
    with pytest.raises(ValueError, match="scan_out must have shape"):
        ap.lidar_pose_scores(bits, 70, poses, obs, scan_out=torch.zeros((3, 5)), **kw)
    # every check above came first: there is no CPU fallback
    both(ValueError, "GPU")
    both(ValueError, "GPU", b=bits[:1])  # one map for every pose set
    with pytest.raises(ValueError, match="GPU"):
        ap.lidar_scan_poses(bits, 70, poses, torch.tensor([2, 0, 2]), out=torch.zeros((3, 5, 8)), normalize=False, **kw)


def test_beam_directions_are_the_envs():
    from ap_gym_amd.lidar_env import lidar_beam_directions
    from oracle import oracle

    for beams, rng in ((1, 5), (7, 5), (32, 60)):
        assert np.array_equal(lidar_beam_directions(beams, rng), oracle.beam_directions(beams, rng))


def test_scan_poses_c_abi_validates_on_the_host():
    from ap_gym_amd import _native as N

    fn = N.lib().apg_lidar_scan_poses
    buf = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(buf)

    def call(**over):
        a = N.ScanPosesArgs(occ=p, map_ids=None, poses=p, beam_dirs=p, observed=p, scan=p, score=p, err=None,
                            n_src=1, m=1, height=4, width=70, k=1, beams=8, normalize=1, lidar_range=5.0)
        for name, v in over.items():
            setattr(a, name, v)
        return fn(ctypes.byref(a), None)

    for kw in (dict(height=0), dict(height=512), dict(width=0), dict(width=512), dict(beams=0), dict(beams=4097),
               dict(lidar_range=0.0), dict(lidar_range=60.5), dict(lidar_range=float("nan")), dict(m=-1), dict(k=-1),
               dict(n_src=-1), dict(poses=None), dict(beam_dirs=None), dict(occ=None), dict(scan=None, score=None),
               dict(observed=None), dict(n_src=2, m=3)):
        assert call(**kw) == N.APG_E_INVALID, kw
        assert N.lib().apg_last_error()
    assert fn(None, None) == N.APG_E_INVALID
    assert call(m=0) == N.APG_OK and call(k=0) == N.APG_OK  # launches nothing
    assert N.APG_ERR_BAD_POSE == 256 and N.APG_ERR_INDEX == 128
    assert ctypes.sizeof(N.ScanPosesArgs) == 8 * 8 + 2 * 8 + 6 * 4
    assert (N.SCAN_POSES_TILE, N.SCAN_POSES_MAX_MPW, N.SCAN_POSES_MAX_GRID) == (256, 32, 8192)
