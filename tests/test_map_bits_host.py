"""map_obs="bits" and unpack_map_bits: what needs no GPU -- the spaces of both modes, the constructor's argument
checks, the numpy restatement of the unpack kernel that tests/test_gpu_map_bits.py compares against, the functional's
argument checks and the C ABI's host-side validation (it returns before any HIP call)."""

import ctypes

import numpy as np
import pytest


def pack_bits_np(maps: np.ndarray) -> np.ndarray:
    """Occupancy rows uint64 [n, H, ceil(W / 64)] of bool maps [n, H, W] (bit x & 63 of word x >> 6; padding 0)."""
    n, h, w = maps.shape
    wpr = (w + 63) // 64
    padded = np.zeros((n, h, wpr * 64), dtype=np.uint8)
    padded[..., :w] = maps
    return np.packbits(padded, axis=-1, bitorder="little").view(np.uint64).reshape(n, h, wpr)


def unpack_bits_np(rows: np.ndarray, width: int, env_ids=None, dtype=np.float32, wall=None) -> np.ndarray:
    """numpy restatement of apg_lidar_unpack_maps: rows uint64 (or int64) [n_src, H, wpr] -> [M, H, W, 1] of `dtype`,
    `wall` (converted once to `dtype`, numpy's astype rounds to nearest even) where the bit is set, 0 elsewhere.
    An id outside [0, n_src) gives an all-zero map.  The padding bits at x >= width are ignored."""
    rows = np.ascontiguousarray(rows).view(np.uint64)
    n_src, h, wpr = rows.shape
    assert wpr == (width + 63) // 64
    dtype = np.dtype(dtype)
    if wall is None:
        wall = 1 if dtype == np.uint8 else np.float32(1) / np.float32(255)
    wall = np.float32(wall).astype(dtype)
    ids = np.arange(n_src) if env_ids is None else np.asarray(env_ids, dtype=np.int64)
    out = np.zeros((len(ids), h, width, 1), dtype=dtype)
    for m, i in enumerate(ids):
        if not 0 <= i < n_src:
            continue
        for y in range(h):
            for x in range(width):
                if (int(rows[i, y, x >> 6]) >> (x & 63)) & 1:
                    out[m, y, x, 0] = wall
    return out


@pytest.mark.parametrize("w", [1, 63, 64, 65, 130])
def test_unpack_bits_np_is_little_endian_unpackbits(w):
    rng = np.random.default_rng(w)
    h, n = 3, 4
    rows = rng.integers(0, 2**64, (n, h, (w + 63) // 64), dtype=np.uint64)  # garbage in the padding bits too
    want = np.unpackbits(rows.view(np.uint8).reshape(n, h, -1), axis=-1, bitorder="little")[..., :w]
    assert np.array_equal(unpack_bits_np(rows, w, dtype=np.uint8)[..., 0], want)
    got = unpack_bits_np(rows, w, env_ids=[2, 0, 2, 7, -1])
    assert got.dtype == np.float32 and got.shape == (5, h, w, 1)
    assert np.array_equal(got[:3, ..., 0], want[[2, 0, 2]] * (np.float32(1) / np.float32(255)))
    assert not got[3:].any()
    assert np.array_equal(pack_bits_np(want.astype(bool)),
                          rows & pack_bits_np(np.ones((n, h, w), bool)))  # pack is its inverse up to the padding


def test_spaces_of_both_map_obs_modes():
    from ap_gym_amd.lidar_env import lidar_spaces
    from ap_gym_amd.spaces import ImageSpace

    dense = lidar_spaces(5, 9, 70, 8, False, False)
    assert isinstance(dense["single_observation_space"]["map"], ImageSpace)
    assert dense["single_observation_space"]["map"].shape == (9, 70, 1)
    assert dense["observation_space"]["map"].shape == (5, 9, 70, 1)
    assert dense["observation_space"]["map"].dtype == np.float32
    same = lidar_spaces(5, 9, 70, 8, False, False, "dense")
    assert same["observation_space"]["map"].shape == (5, 9, 70, 1)
    bits = lidar_spaces(5, 9, 70, 8, False, False, "bits")
    single, batch = bits["single_observation_space"]["map"], bits["observation_space"]["map"]
    assert single.shape == (9, 2) and single.dtype == np.uint64
    assert batch.shape == (5, 9, 2) and batch.dtype == np.uint64
    assert int(single.low.max()) == 0 and int(single.high.min()) == 2**64 - 1
    assert lidar_spaces(5, 64, 64, 8, False, False, "bits")["single_observation_space"]["map"].shape == (64, 1)
    for k in ("lidar", "odometry", "time_step"):
        assert bits["observation_space"][k].shape == dense["observation_space"][k].shape
    assert "map" not in lidar_spaces(5, 9, 70, 8, True, False, "bits")["single_observation_space"].spaces


def test_map_obs_argument_errors():
    """Both raise before any device work (no GPU needed)."""
    import ap_gym_amd as ap

    with pytest.raises(ValueError, match="map_obs"):
        ap.LIDARLocalization2DVectorEnv(num_envs=2, map_obs="packed")
    with pytest.raises(ValueError, match="static"):
        ap.LIDARLocalization2DVectorEnv(num_envs=2, map_obs="bits", static_map=True)
    with pytest.raises(ValueError, match="map_obs"):
        ap.make_vec("LIDARLocRooms-v0", num_envs=2, map_obs="sparse")
    with pytest.raises(ValueError, match="static"):
        ap.make_vec("LIDARLocMazeStatic-v0", num_envs=2, map_obs="bits")


def test_unpack_map_bits_argument_checks():
    import torch

    import ap_gym_amd as ap

    bits = torch.zeros((3, 4, 2), dtype=torch.int64)
    with pytest.raises(TypeError, match="int64"):
        ap.unpack_map_bits(bits.to(torch.int32), 70)
    with pytest.raises(TypeError, match="int64"):
        ap.unpack_map_bits(bits[0], 70)
    with pytest.raises(TypeError, match="int64"):
        ap.unpack_map_bits(bits.numpy(), 70)
    with pytest.raises(ValueError, match="words per row"):
        ap.unpack_map_bits(bits, 64)
    with pytest.raises(ValueError, match="1..511"):
        ap.unpack_map_bits(torch.zeros((3, 4, 8), dtype=torch.int64), 512)
    with pytest.raises(ValueError, match="1..511"):
        ap.unpack_map_bits(torch.zeros((3, 0, 2), dtype=torch.int64), 70)
    with pytest.raises(TypeError, match="dtype"):
        ap.unpack_map_bits(bits, 70, dtype=torch.float64)
    with pytest.raises(TypeError, match="asked for"):
        ap.unpack_map_bits(bits, 70, dtype=torch.float16, out=torch.zeros((3, 4, 70, 1)))
    for wall in (256, -1, 0.5):
        with pytest.raises(ValueError, match="0..255"):
            ap.unpack_map_bits(bits, 70, dtype=torch.uint8, wall=wall)
    with pytest.raises(ValueError, match="GPU"):  # every check above came first: there is no CPU fallback
        ap.unpack_map_bits(bits, 70)


def test_unpack_maps_c_abi_validates_on_the_host():
    from ap_gym_amd import _native as N

    fn = N.lib().apg_lidar_unpack_maps
    buf = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(buf)

    def call(h=4, w=70, count=1, dtype=N.APG_UNPACK_F32, wall=1.0, n_src=1):
        return fn(p, n_src, h, w, None, count, dtype, wall, p, None, None)

    for kw in (dict(h=0), dict(h=512), dict(w=0), dict(w=512), dict(count=-1), dict(dtype=4), dict(dtype=-1),
               dict(dtype=N.APG_UNPACK_U8, wall=256.0), dict(dtype=N.APG_UNPACK_U8, wall=-1.0),
               dict(dtype=N.APG_UNPACK_U8, wall=1.5), dict(dtype=N.APG_UNPACK_U8, wall=float("nan"))):
        assert call(**kw) == N.APG_E_INVALID, kw
        assert N.lib().apg_last_error()
    for dt in (N.APG_UNPACK_F32, N.APG_UNPACK_F16, N.APG_UNPACK_BF16, N.APG_UNPACK_U8):
        assert call(count=0, dtype=dt) == N.APG_OK  # count == 0 launches nothing
    assert N.APG_ERR_INDEX == 128


def test_host_words_np_slices_refer_to_the_array_handed_out():
    """The numpy backend hands a host block out again once nothing refers to the array it returned
    (sys.getrefcount).  numpy collapses chains of views, so that array's base must not be another ndarray: every
    slice or view a caller keeps then has the returned array as its base and is counted."""
    import sys

    import torch

    from ap_gym_amd.map_bits import host_words_np

    t = torch.arange(24, dtype=torch.int64).reshape(2, 3, 4)
    t[0, 0, 0] = -1
    a = host_words_np(t)
    assert a.dtype == np.uint64 and a.shape == (2, 3, 4) and int(a[0, 0, 0]) == 2**64 - 1
    assert not isinstance(a.base, np.ndarray)
    a[1, 2, 3] = 7  # the same memory, writable
    assert int(t[1, 2, 3]) == 7
    alone = sys.getrefcount(a)
    row, plane, as_bytes = a[0], a[..., 0], a.view(np.uint8)
    assert row.base is a and plane.base is a and as_bytes.base is a
    assert sys.getrefcount(a) == alone + 3
    del row, plane, as_bytes
    assert sys.getrefcount(a) == alone


def test_unpack_map_bits_checks_the_shape_of_out_and_env_ids():
    """Checked before the device, so without a GPU too."""
    import torch

    import ap_gym_amd as ap

    bits = torch.zeros((3, 4, 2), dtype=torch.int64)
    ids = torch.tensor([2, 0], dtype=torch.int64)
    for shape in ((3, 4, 69, 1), (2, 4, 70, 1), (3, 4, 70, 2), (3 * 4 * 70,), (3, 70, 4)):
        with pytest.raises(ValueError, match="shape"):
            ap.unpack_map_bits(bits, 70, out=torch.zeros(shape))
    with pytest.raises(ValueError, match="shape"):  # two ids: two maps
        ap.unpack_map_bits(bits, 70, ids, out=torch.zeros((3, 4, 70, 1)))
    for bad in (ids.to(torch.int32), ids.reshape(1, 2), [2, 0], np.array([2, 0])):
        with pytest.raises(TypeError, match="env_ids"):
            ap.unpack_map_bits(bits, 70, bad)
    for ok_shape in ((2, 4, 70, 1), (2, 4, 70)):  # right shapes reach the device check
        with pytest.raises(ValueError, match="GPU"):
            ap.unpack_map_bits(bits, 70, ids, out=torch.zeros(ok_shape))
