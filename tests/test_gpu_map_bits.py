"""map_obs="bits" and the device unpack kernel (k_unpack_maps, csrc/apg_unpack.hip) on the GPU.

The op is compared with the numpy restatement of tests/test_map_bits_host.py (itself checked against
np.unpackbits(bitorder="little")) at the smallest shapes that cross each of the kernel's boundaries: one cell, rows
shorter than / equal to / one past a word, two words, W % 64 == 0 (rows copied) and not (rows re-laid), map sizes
that leave every map's start at another offset of its 16-byte chunk, one and several maps per workgroup, more batches
than the grid holds.  The env in bits mode is compared step for step with the same env in dense mode, which the
oracle and the goldens already pin.
"""

import numpy as np
import pytest

from test_gpu_lidar_pool import random_pool
from test_map_bits_host import pack_bits_np, unpack_bits_np

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (7, 63), (5, 64), (4, 65), (9, 127), (2, 128), (3, 130), (33, 31), (6, 511)]
IDS = [None, [3, 0, 3, 5, 1]]
# the second wall of every dtype is inexact in it, so the conversion's rounding (to nearest even) shows
WALLS = {"float32": (None, 0.3), "float16": (None, 0.3), "bfloat16": (None, 0.3), "uint8": (None, 255)}
SENTINEL = {"float32": -7.0, "float16": -7.0, "bfloat16": -7.0, "uint8": 0x5A}


def random_rows(n, h, w, seed):
    """uint64 [n, h, wpr] with random garbage in the padding bits too."""
    return np.random.default_rng(seed).integers(0, 2**64, (n, h, (w + 63) // 64), dtype=np.uint64)


def to_device(rows, gpu):
    import torch

    return torch.as_tensor(rows.view(np.int64), device=gpu)


def expected(rows, w, ids, dtype_name, wall):
    """The numpy restatement's result as raw element bits (bfloat16: torch's CPU conversion of the wall value, which
    rounds to nearest even; numpy has no such dtype)."""
    import torch

    if dtype_name == "bfloat16":
        wall16 = torch.tensor(np.float32(1) / np.float32(255) if wall is None else wall,
                              dtype=torch.float32).to(torch.bfloat16).view(torch.int16).item()
        mask = unpack_bits_np(rows, w, ids, dtype=np.uint8)
        return (mask.astype(np.int16) * np.int16(wall16)).astype(np.int16)
    want = unpack_bits_np(rows, w, ids, dtype=np.dtype(dtype_name), wall=wall)
    return want.view({4: np.int32, 2: np.int16, 1: np.uint8}[want.itemsize])


def raw(t):
    """A tensor's elements as raw bits on the host."""
    import torch

    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]).cpu().numpy()


def carved_out(count, h, w, dtype, gpu, offset=1, slack=37):
    """`out` [count, h, w, 1] carved from a larger sentinel-filled buffer at an element offset, so it is not 16-byte
    aligned; returns (buffer, out)."""
    import torch

    numel = count * h * w
    buf = torch.full((numel + offset + slack,), SENTINEL[str(dtype).split(".")[1]], dtype=dtype, device=gpu)
    return buf, buf[offset:offset + numel].view(count, h, w, 1)


@pytest.mark.parametrize("dtype_name", list(WALLS))
@pytest.mark.parametrize("h,w", SHAPES)
def test_unpack_op_matches_numpy(gpu, h, w, dtype_name):
    import torch

    import ap_gym_amd as ap

    dtype = getattr(torch, dtype_name)
    rows = random_rows(6, h, w, seed=1000 * h + w)
    bits = to_device(rows, gpu)
    for ids in IDS:
        ids_t = None if ids is None else torch.tensor(ids, dtype=torch.int64, device=gpu)
        count = 6 if ids is None else len(ids)
        for wall in WALLS[dtype_name]:
            for offset in (1, 0, 3):
                buf, out = carved_out(count, h, w, dtype, gpu, offset)
                before = raw(buf).copy()
                got = ap.unpack_map_bits(bits, w, ids_t, wall=wall, out=out)
                assert got is out
                after = raw(buf)
                body = slice(offset, offset + count * h * w)
                assert np.array_equal(after[body].reshape(count, h, w, 1), expected(rows, w, ids, dtype_name, wall)), \
                    (ids, wall, offset)
                assert np.array_equal(after[:offset], before[:offset]), "sentinels before out"
                assert np.array_equal(after[body.stop:], before[body.stop:]), "sentinels after out"
        fresh = ap.unpack_map_bits(bits, w, ids_t, dtype=dtype)
        assert fresh.shape == (count, h, w, 1) and fresh.dtype == dtype
        assert np.array_equal(raw(fresh), expected(rows, w, ids, dtype_name, None))


def test_unpack_default_is_float32_dense_value(gpu):
    import ap_gym_amd as ap

    rows = random_rows(3, 4, 70, seed=5)
    got = ap.unpack_map_bits(to_device(rows, gpu), 70)
    want = np.unpackbits(rows.view(np.uint8).reshape(3, 4, -1), axis=-1, bitorder="little")[..., :70]
    assert got.dtype.is_floating_point and got.element_size() == 4
    assert np.array_equal(got.cpu().numpy()[..., 0], want.astype(np.float32) * (np.float32(1) / np.float32(255)))


def test_unpack_count_zero_is_a_no_op(gpu):
    import torch

    import ap_gym_amd as ap

    bits = to_device(random_rows(6, 3, 5, seed=1), gpu)
    none = torch.zeros(0, dtype=torch.int64, device=gpu)
    got = ap.unpack_map_bits(bits, 5, none)
    assert got.shape == (0, 3, 5, 1)
    buf, out = carved_out(0, 3, 5, torch.float32, gpu)
    ap.unpack_map_bits(bits, 5, none, out=out)
    assert (buf == SENTINEL["float32"]).all()
    assert ap.unpack_map_bits(bits[:0], 5).shape == (0, 3, 5, 1)


@pytest.mark.parametrize("dtype_name", ["float32", "uint8"])
def test_unpack_many_maps_grid_stride(gpu, dtype_name):
    """64 x 64, n_src = 300: one (float32) and several (uint8) maps per workgroup iteration, a ragged last batch;
    300 000 gathered 3 x 5 maps: more batches (32 maps each) than the grid's 8 192 workgroups, so they stride."""
    import torch

    import ap_gym_amd as ap

    dtype = getattr(torch, dtype_name)
    rows = random_rows(300, 64, 64, seed=64)
    buf, out = carved_out(300, 64, 64, dtype, gpu)
    ap.unpack_map_bits(to_device(rows, gpu), 64, out=out)
    want = np.unpackbits(rows.view(np.uint8).reshape(300, 64, -1), axis=-1, bitorder="little")
    assert np.array_equal(out.cpu().numpy()[..., 0] != 0, want.astype(bool))
    assert np.array_equal(raw(out)[:7], expected(rows[:7], 64, None, dtype_name, None))
    assert (buf[0] == SENTINEL[dtype_name]) and (buf[1 + out.numel():] == SENTINEL[dtype_name]).all()

    small = random_rows(6, 3, 5, seed=35)
    ids = np.random.default_rng(2).integers(0, 6, 300_000)
    buf, out = carved_out(len(ids), 3, 5, dtype, gpu)
    ap.unpack_map_bits(to_device(small, gpu), 5, torch.as_tensor(ids, device=gpu), out=out)
    per_map = expected(small, 5, None, dtype_name, None)
    assert np.array_equal(raw(out), per_map[ids])
    assert (buf[0] == SENTINEL[dtype_name]) and (buf[1 + out.numel():] == SENTINEL[dtype_name]).all()


def test_unpack_bad_id_is_flagged_not_read(gpu):
    """Ids outside [0, n_src) are never read: all-zero maps and APG_ERR_INDEX, the good row still right; the env
    method raises IndexError through check_errors()."""
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    n_src, h, w = 6, 4, 65
    rows = random_rows(n_src, h, w, seed=9)
    ids = [0, n_src, -1]
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    got = ap.unpack_map_bits(to_device(rows, gpu), w, torch.tensor(ids, device=gpu), err=err)
    assert int(err.item()) == N.APG_ERR_INDEX
    assert np.array_equal(got.cpu().numpy(), unpack_bits_np(rows, w, ids))
    assert got[0].any() and not got[1:].any()
    err.zero_()
    ap.unpack_map_bits(to_device(rows, gpu), w, torch.tensor([5, 0], device=gpu), err=err)
    assert int(err.item()) == 0
    ap.unpack_map_bits(to_device(rows, gpu), w, torch.tensor(ids, device=gpu))  # no error word: zeros, nothing else

    env = ap.LIDARLocalization2DVectorEnv(num_envs=n_src, dataset=ap.FloorMapDatasetRooms(32, 32), device=gpu,
                                          array_backend="torch", map_obs="bits")
    obs, _ = env.reset(seed=3)
    env.check_errors()
    maps = env.unpack_maps(ids)
    assert maps.shape == (3, 32, 32, 1) and maps[0].any() and not maps[1:].any()
    with pytest.raises(IndexError):
        env.check_errors()
    env.check_errors()  # raised once, then clear
    assert torch.equal(env.unpack_maps([0])[0], maps[0])
    env.close()
    npenv = ap.LIDARLocalization2DVectorEnv(num_envs=n_src, dataset=ap.FloorMapDatasetRooms(32, 32), device=gpu,
                                            map_obs="bits")
    npenv.reset(seed=3)
    with pytest.raises(IndexError):
        npenv.unpack_maps(np.array(ids))
    assert np.array_equal(npenv.unpack_maps(np.array([0]))[0], maps[0].cpu().numpy())
    with pytest.raises(RuntimeError, match="bits"):
        ap.LIDARLocalization2DVectorEnv(num_envs=2, dataset=ap.FloorMapDatasetRooms(32, 32),
                                        device=gpu).unpack_maps()
    npenv.close()


# ------------------------------------------------------------------ the env, bits mode against dense mode
def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def assert_same(a, b, where):
    """array_equal over nested dicts of outputs (torch or numpy; object arrays of lists: the numpy stats)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for k in a:
            assert_same(a[k], b[k], f"{where}/{k}")
        return
    x, y = host(a), host(b)
    assert x.dtype == y.dtype and x.shape == y.shape, where
    if x.dtype == object:
        assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(x, y)), where
    else:
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), where


def _source(ap, source):
    if source == "rooms":
        return ap.FloorMapDatasetRooms(32, 32), {}
    if source.startswith("maze"):
        return ap.FloorMapDatasetMaze(21, 21), dict(prefetch=source == "maze_prefetch")
    maps = random_pool(11, 9, 70, seed=4)  # two words per row
    return ap.ArrayFloorMapDataset(maps), dict(frozen_maps=source == "pool_frozen")


@pytest.mark.parametrize("backend,copy", [("torch", False), ("torch", True), ("numpy", True), ("numpy", False)])
@pytest.mark.parametrize("source", ["rooms", "maze_prefetch", "maze_sync", "pool_frozen", "pool_streamed"])
def test_env_bits_mode_matches_dense_mode(gpu, source, backend, copy):
    import ap_gym_amd as ap

    n, steps = 70, 13
    ds, extra = _source(ap, source)
    h, w = ds.map_height, ds.map_width
    kw = dict(num_envs=n, dataset=ds, device=gpu, array_backend=backend, copy=copy, max_episode_steps=5,
              lidar_beam_count=8, log_stats=True, render_envs=[0, 69], **extra)
    dense = ap.LIDARLocalization2DVectorEnv(**kw)
    bits = ap.LIDARLocalization2DVectorEnv(map_obs="bits", **kw)
    assert bits._t["map_obs"] is None and bits._out.map_obs is None  # no dense buffer, NULL in the C ABI
    assert bits.observation_space["map"].shape == (n, h, (w + 63) // 64)
    valid = pack_bits_np(np.ones((1, h, w), bool))

    def check(ob, od, where):
        for k in ("lidar", "odometry", "time_step"):
            assert_same(ob[k], od[k], f"{where}/{k}")
        m = host(ob["map"])
        if backend == "numpy":
            assert m.dtype == np.uint64 and (m.flags.writeable or not copy)
        else:
            assert str(ob["map"].dtype) == "torch.int64"
            assert (ob["map"].data_ptr() == bits._t["occ"].data_ptr()) == (not copy)  # the state's own rows, or a clone
            assert (bits.device_outputs()["map"].data_ptr() == bits._t["occ"].data_ptr())
        assert m.shape == (n, h, (w + 63) // 64), where
        d = host(od["map"])
        assert np.array_equal(m.view(np.uint64) & valid, pack_bits_np(d[..., 0] != 0)), where
        assert_same(bits.unpack_maps(), od["map"], f"{where}/unpack_maps")
        return ob["map"]  # (the returned object itself: what a caller would keep)

    ob, ib = bits.reset(seed=21)
    od, idn = dense.reset(seed=21)
    assert_same(ib, idn, "reset/info")
    held = check(ob, od, "reset")
    held_copy = first = host(held).view(np.uint64).copy()
    rng = np.random.default_rng(8)
    changed = False
    for t in range(steps):
        a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        p = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        ob, rb, tb, ub, ib = bits.step({"action": a, "prediction": p})
        od, rd, td, ud, idn = dense.step({"action": a, "prediction": p})
        for name, x, y in (("reward", rb, rd), ("terminated", tb, td), ("truncated", ub, ud), ("info", ib, idn)):
            assert_same(x, y, f"step {t}/{name}")
        now = check(ob, od, f"step {t}")
        changed |= not np.array_equal(host(now).view(np.uint64) & valid, first & valid)
        if copy:  # the array handed out earlier is the caller's own: this step (a reset step included) left it alone
            assert np.array_equal(host(held).view(np.uint64), held_copy), t
            held, held_copy = now, host(now).view(np.uint64).copy()
    assert changed  # two autoresets happened: the maps did change
    ids = np.array([69, 0, 33, 69])
    assert_same(bits.unpack_maps(ids), host(od["map"])[ids], "unpack_maps(ids)")
    if backend == "torch":
        import torch

        half = bits.unpack_maps(torch.as_tensor(ids, device=gpu), dtype=torch.float16)
        assert half.dtype == torch.float16
        assert np.array_equal(half.cpu().numpy(), host(od["map"])[ids].astype(np.float16))
    else:
        u8 = bits.unpack_maps(ids, dtype=np.uint8)
        assert u8.dtype == np.uint8 and np.array_equal(u8, (host(od["map"])[ids] != 0).astype(np.uint8))
    for fb, fd in zip(bits.render(), dense.render(), strict=True):
        assert np.array_equal(fb, fd)
    bits.check_errors()
    dense.check_errors()
    bits.close()
    dense.close()


def test_captured_step_graph_in_bits_mode(gpu):
    """capture_step_graph in bits mode: three replays (an autoreset among them) equal three eager steps of a twin,
    the bit rows included."""
    import torch

    import ap_gym_amd as ap

    n = 70
    kw = dict(num_envs=n, dataset=ap.FloorMapDatasetRooms(32, 32), device=gpu, array_backend="torch",
              max_episode_steps=2, map_obs="bits")
    eager = ap.LIDARLocalization2DVectorEnv(**kw)
    graphed = ap.LIDARLocalization2DVectorEnv(**kw)
    eager.reset(seed=11)
    graphed.reset(seed=11)
    a_buf = torch.zeros((n, 2), dtype=torch.float32, device=gpu)
    p_buf = torch.zeros((n, 2), dtype=torch.float32, device=gpu)
    graph = graphed.capture_step_graph(a_buf, p_buf)
    out_g, out_e = graphed.device_outputs(), eager.device_outputs()
    assert out_g["map"].dtype == torch.int64 and out_g["map"].shape == (n, 32, 1)
    before = out_g["map"].clone()
    g = torch.Generator(device=gpu).manual_seed(3)
    for t in range(3):
        a = torch.rand((n, 2), device=gpu, generator=g) * 2 - 1
        p = torch.rand((n, 2), device=gpu, generator=g) * 2 - 1
        eager.step({"action": a, "prediction": p})
        a_buf.copy_(a)
        p_buf.copy_(p)
        graph.replay()
        for k in out_e:
            assert torch.equal(out_g[k], out_e[k]), (t, k)
        assert torch.equal(graphed.unpack_maps(), eager.unpack_maps()), t
    assert not torch.equal(out_g["map"], before)  # the third step reset every env: new maps
    eager.check_errors()
    graphed.check_errors()
    eager.close()
    graphed.close()


@pytest.mark.parametrize("snapshot", ["copy", "shared"])
def test_numpy_bits_kept_slices_stay_the_callers_own(gpu, snapshot):
    """numpy backend, copy=True: a caller who keeps only a slice or a view of a returned obs["map"] (and drops the
    dict) keeps its values over more steps than the env has host blocks, resets among them -- as in dense mode."""
    import ap_gym_amd as ap
    from ap_gym_amd.lidar_env import LIDARLocalization2DVectorEnv as Env

    n = 6
    env = Env(num_envs=n, dataset=ap.FloorMapDatasetRooms(32, 32), device=gpu, copy=True, obs_snapshot=snapshot,
              max_episode_steps=2, map_obs="bits")
    zero = {"action": np.zeros((n, 2), np.float32), "prediction": np.zeros((n, 2), np.float32)}
    obs, _ = env.reset(seed=5)
    kept = [(obs["map"][0], obs["map"][0].copy())]
    del obs
    for t in range(3 * Env.MAP_COPIES + 3):  # every third step resets every env: new maps
        obs = env.step(zero)[0]
        piece = (obs["map"][t % n], obs["map"].view(np.uint8), obs["map"][..., 0])[t % 3]
        del obs
        if snapshot == "copy" and t % 2:  # the caller's own: writable, and what it wrote stays
            piece[...] = 0xA5
        kept.append((piece, piece.copy()))
        for i, (k, c) in enumerate(kept):
            assert np.array_equal(k, c), (t, i)
    rows = [c for k, c in kept if c.shape == (32, 1)]
    assert any(not np.array_equal(rows[0], r) for r in rows[1:])  # the maps did change in between
    fresh, want = env.step(zero)[0]["map"], env._t["occ"].view(n, 32, 1).cpu().numpy().view(np.uint64)
    assert np.array_equal(fresh, want)  # and what the caller wrote reached no later hand-out
    env.close()


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_env_unpack_maps_accepts_any_integer_ids(gpu, backend):
    import torch

    import ap_gym_amd as ap

    env = ap.LIDARLocalization2DVectorEnv(num_envs=5, dataset=ap.FloorMapDatasetRooms(32, 32), device=gpu,
                                          array_backend=backend, map_obs="bits")
    env.reset(seed=2)
    want = host(env.unpack_maps())[[4, 0, 4]]
    for ids in ([4, 0, 4], (4, 0, 4), np.array([4, 0, 4], np.int32), np.array([[4, 0, 4]], np.uint8),
                torch.tensor([4, 0, 4], dtype=torch.int32), torch.tensor([4, 0, 4]),
                torch.tensor([4, 0, 4], dtype=torch.int16, device=gpu), torch.tensor([4, 0, 4], device=gpu)):
        assert np.array_equal(host(env.unpack_maps(ids)), want), type(ids)
    assert host(env.unpack_maps([])).shape == (0, 32, 32, 1)
    assert np.array_equal(host(env.unpack_maps(3)), host(env.unpack_maps())[[3]])
    for bad in ([0.0, 1.0], np.array([True, False]), torch.tensor([0.5]), torch.tensor([True])):
        with pytest.raises(TypeError, match="integers"):
            env.unpack_maps(bad)
    env.check_errors()
    env.close()
