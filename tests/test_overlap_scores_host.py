"""Host-side pieces of the target-overlap scores (ap_gym_amd.overlap_scores): the numpy restatement of the definition
in include/apgym_capi.h (apg_image_overlap_scores) that the GPU tests compare against bit for bit, the properties of
that definition that need no device, and the argument checks of the public function (raised on CPU tensors, before
anything touches a device).  The glimpses come from oracle/image_oracle.py."""

import ctypes

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from oracle import image_oracle as io

F = np.float32


def overlap_scores_np(g, q, G, h, image_size, sensor, scale=1.0, logw=None, gain=0.0, tau=0.0):
    """The definition, step by step: g, G f32 [M, s0, s1, C]; q [M, 2]; h [M, K, 2] or [K, 2] (f32 or f64) ->
    (sse f32 [M, K], count i32 [M, K], logw_out f32 [M, K] or None, bad bool [M, K]: the error bit)."""
    g, G = np.asarray(g, F), np.asarray(G, F)
    q, h = np.asarray(q), np.asarray(h)
    m, s0, s1, c = g.shape
    assert (s0, s1) == tuple(sensor)
    h = np.broadcast_to(h, (m,) + h.shape[-2:])
    k = h.shape[1]
    lim = io.sensor_pos_lim(image_size, sensor, scale)  # f64 (x, y): x pairs with sensor[0], like the reference
    q64, h64 = q.astype(np.float64)[:, None, :], h.astype(np.float64)
    sse = np.zeros((m, k), F)
    count = np.zeros((m, k), np.int32)
    with np.errstate(all="ignore"):
        d = ((q64 - h64) * lim) / np.float64(scale)  # 1
        bad = ~(np.isfinite(q64).all(-1) & np.isfinite(h64).all(-1))  # 2
        dy, dx = d[..., 1], d[..., 0]
        none = bad | ~(np.abs(dy) < s0) | ~(np.abs(dx) < s1)
        dy, dx = np.where(none, 0.0, dy), np.where(none, 0.0, dx)
        iy, ix = np.floor(dy), np.floor(dx)  # 3
        fy, fx = (dy - iy).astype(F)[..., None, None, None], (dx - ix).astype(F)[..., None, None, None]
        ay = np.arange(s0, dtype=np.float64) + dy[..., None]
        bx = np.arange(s1, dtype=np.float64) + dx[..., None]
        in_a = (0 <= ay) & (ay <= s0 - 1) & ~none[..., None]
        in_b = (0 <= bx) & (bx <= s1 - 1) & ~none[..., None]
        # 4 (the clips never act on a sample in the overlap)
        r0 = np.clip(np.arange(s0) + iy.astype(np.int64)[..., None], 0, s0 - 1)
        c0 = np.clip(np.arange(s1) + ix.astype(np.int64)[..., None], 0, s1 - 1)
        r1, c1 = np.minimum(r0 + 1, s0 - 1), np.minimum(c0 + 1, s1 - 1)
        one = F(1)
        for i in range(m):  # (set by set: [K, s0, s1, C] temporaries)
            R0, R1, C0, C1 = r0[i][:, :, None], r1[i][:, :, None], c0[i][:, None, :], c1[i][:, None, :]
            Gi = G[i]
            top = Gi[R0, C0] * (one - fx[i]) + Gi[R0, C1] * fx[i]
            bot = Gi[R1, C0] * (one - fx[i]) + Gi[R1, C1] * fx[i]
            pred = top * (one - fy[i]) + bot * fy[i]
            assert pred.dtype == F
            e = (g[i] - pred) * (g[i] - pred)
            mask = in_a[i][:, :, None, None] & in_b[i][:, None, :, None]
            e = np.where(mask, e, F(0))
            sse[i] = io.pairwise_sum_f32(e.reshape(k, s0 * s1 * c))  # 5
        count[:] = c * in_a.sum(-1) * in_b.sum(-1)
        sse[bad] = np.nan
        out = None
        if logw is not None:  # 6
            out = np.asarray(logw, F) + F(gain) * (F(tau) * count.astype(F) - sse)
            assert out.dtype == F
            out[~np.isfinite(sse)] = np.nan
    return sse, count, out, bad


def noise_case(seed, image_hw=(40, 40), sensor=(8, 8), step=6):
    """The exact construction: a single-channel uint8 noise image, the hypotheses at every integer pixel position
    (lim = 16 for 40 x 40 / 8 x 8 / scale 1, so every multiple of 1/16 is one), the target one of them, the sensor on
    every `step`-th integer position per axis.  Returns (pool u8 [1, H, W, 1], hypotheses f64 [K, 2], target index,
    sensor positions f64 [P, 2], lim)."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (1, image_hw[0], image_hw[1], 1), dtype=np.uint8)
    lim = io.sensor_pos_lim(image_hw, sensor, 1.0)
    assert lim[0] == lim[1] == int(lim[0])
    n = int(lim[0])
    ticks = np.arange(-n, n + 1) / n
    hyp = np.stack(np.meshgrid(ticks, ticks, indexing="xy"), -1).reshape(-1, 2)
    target = int(rng.integers(len(hyp)))
    pos = np.stack(np.meshgrid(ticks[::step], ticks[::step], indexing="xy"), -1).reshape(-1, 2)
    return pool, hyp, target, pos, lim


def check_noise_sweep(sse, count, target, tau=F(0.01)):
    """The three required properties of the exact construction, from sse / count [P, K] of a sweep over the sensor
    positions: the true hypothesis has sse == 0.0 exactly wherever it overlaps, every other hypothesis with
    count >= 4 has sse > 0, and the log-weights summed over the sweep (gain 1) peak at the target."""
    assert (count[:, target] > 0).any()
    assert np.all(sse[:, target][count[:, target] > 0] == 0.0)
    others = np.ones(sse.shape[1], bool)
    others[target] = False
    wrong = sse[:, others][count[:, others] >= 4]
    assert wrong.size and np.all(wrong > 0), wrong.min()
    logw = np.zeros(sse.shape[1], F)
    for p in range(len(sse)):
        logw = logw + F(1) * (tau * count[p].astype(F) - sse[p])
    assert int(np.argmax(logw)) == target
    return float(wrong.min())


# ------------------------------------------------------------------ the definition's own properties
def _glimpses(pool, positions, sensor, scale=1.0, channels=1):
    imgs = io.images_f32(pool, channels)
    return io.glimpse(np.broadcast_to(imgs, (len(positions),) + imgs.shape[1:]), positions, sensor, scale)


def test_restatement_sums_like_numpy():
    rng = np.random.default_rng(3)
    for sensor, c in (((5, 5), 1), ((12, 12), 3), ((3, 43), 1)):
        g, G = rng.random((2, 2, *sensor, c), dtype=F)
        q = rng.uniform(-1, 1, (2, 2))
        h = q[:, None, :] + rng.uniform(-0.2, 0.2, (2, 7, 2))
        sse, count, _, _ = overlap_scores_np(g, q, G, h, (64, 64), sensor)
        lim = io.sensor_pos_lim((64, 64), sensor, 1.0)
        for i in range(2):
            for j in range(7):  # the same block summed by numpy itself
                one = overlap_scores_np(g[i:i + 1], q[i:i + 1], G[i:i + 1], h[i:i + 1, j:j + 1], (64, 64), sensor)
                assert one[0][0, 0] == sse[i, j] and one[1][0, 0] == count[i, j]
                d = (q[i] - h[i, j]) * lim
                assert count[i, j] == c * max(0, int(np.sum((0 <= np.arange(sensor[0]) + d[1])
                                                            & (np.arange(sensor[0]) + d[1] <= sensor[0] - 1)))) * max(
                    0, int(np.sum((0 <= np.arange(sensor[1]) + d[0]) & (np.arange(sensor[1]) + d[0] <= sensor[1] - 1))))
    # pairwise_sum_f32 is np.sum on a contiguous float32 block
    e = rng.random((5, 432), dtype=F)
    assert np.array_equal(io.pairwise_sum_f32(e), np.array([np.sum(r, dtype=F) for r in e]))


def test_zero_shift_is_exact():
    rng = np.random.default_rng(0)
    for sensor, c in (((1, 1), 1), ((5, 5), 1), ((3, 7), 1), ((12, 12), 3)):
        g = rng.random((3, *sensor, c), dtype=F)
        q = rng.uniform(-1, 1, (3, 2)).astype(F)
        sse, count, logw, bad = overlap_scores_np(g, q, g, q[:, None, :], (31, 47), sensor, logw=np.zeros((3, 1), F),
                                                  gain=2.0, tau=0.5)
        l = sensor[0] * sensor[1] * c
        assert np.all(sse == 0.0) and not np.signbit(sse).any() and np.all(count == l) and not bad.any()
        assert np.array_equal(logw, np.full((3, 1), F(2.0) * (F(0.5) * F(l)), F))


def test_integer_shifts_count_the_overlap():
    rng = np.random.default_rng(1)
    image, sensor, c = (40, 52), (6, 8), 3  # lim = (52 - 6) / 2, (40 - 8) / 2 = (23, 16): integers
    lim = io.sensor_pos_lim(image, sensor, 1.0)
    assert tuple(lim) == (23.0, 16.0)
    g, G = rng.random((2, 1, *sensor, c), dtype=F)
    q = np.array([[3 / 23, -2 / 16]])
    shifts = [(iy, ix) for iy in range(-7, 8) for ix in range(-9, 10)]
    h = np.array([[q[0, 0] - ix / 23, q[0, 1] - iy / 16] for iy, ix in shifts])[None]
    d = (q[:, None, :] - h) * lim
    sse, count, _, _ = overlap_scores_np(g, q, G, h, image, sensor)
    for j, (iy, ix) in enumerate(shifts):
        dy, dx = d[0, j, 1], d[0, j, 0]  # what the shift really is in f64 (an integer up to rounding)
        rows = int(np.sum((0 <= np.arange(6) + dy) & (np.arange(6) + dy <= 5))) if abs(dy) < 6 else 0
        cols = int(np.sum((0 <= np.arange(8) + dx) & (np.arange(8) + dx <= 7))) if abs(dx) < 8 else 0
        assert count[0, j] == c * rows * cols
        if dy == iy and dx == ix:
            assert count[0, j] == c * max(0, 6 - abs(iy)) * max(0, 8 - abs(ix))
    exact = [(d[0, j, 1] == iy and d[0, j, 0] == ix) for j, (iy, ix) in enumerate(shifts)]
    assert sum(exact) > len(shifts) // 2  # (most of the constructed shifts are exact integers)


def test_domain():
    rng = np.random.default_rng(2)
    sensor = (5, 5)
    g, G = rng.random((2, 1, *sensor, 1), dtype=F)
    g[0, 0, 0, 0] = np.nan  # reaches only the hypotheses whose overlap contains sample (0, 0)
    lim = io.sensor_pos_lim((28, 28), sensor, 1.0)
    q = np.zeros((1, 2))
    dyx = [(0, 0), (1, 1), (-1, 0), (0, -1), (4, 4), (-4, -4), (3.5, 0), (5, 0), (0, -5), (1e30, 0)]
    h = np.array([[-dx / lim[0], -dy / lim[1]] for dy, dx in dyx] + [[np.nan, 0], [0, np.inf]])[None]
    sse, count, logw, bad = overlap_scores_np(g, q, G, h, (28, 28), sensor, logw=np.full((1, 12), 3, F), gain=1, tau=1)
    # sample (0, 0) lies in the overlap iff dy >= 0 and dx >= 0
    assert [bool(np.isnan(s)) for s in sse[0]] == [True, True, False, False, True, False, True, False, False, False,
                                                   True, True]
    assert list(count[0]) == [25, 16, 20, 20, 1, 1, 5, 0, 0, 0, 0, 0]  # 3.5: row 0 alone, with f = 0.5
    assert list(bad[0]) == [False] * 10 + [True, True]
    assert np.all(sse[0, 7:10] == 0) and np.all(logw[0, 7:10] == 3) and np.isnan(logw[0, 10:]).all()
    qbad = overlap_scores_np(g, np.array([[np.nan, 0.0]]), G, h, (28, 28), sensor)
    assert np.isnan(qbad[0]).all() and not qbad[1].any() and qbad[3].all()


@pytest.mark.parametrize("seed", range(10))
def test_exact_construction_finds_the_target(seed):
    pool, hyp, target, pos, _ = noise_case(seed)
    assert len(hyp) == 33 * 33 and len(pos) == 36
    G = _glimpses(pool, hyp[target][None], (8, 8))
    g = _glimpses(pool, pos, (8, 8))
    assert np.array_equal(np.unique(np.round(g * 255)), np.unique(g * F(255)))  # integer pixel positions: exact pixels
    sse, count, _, bad = overlap_scores_np(g, pos, np.broadcast_to(G, g.shape), hyp, (40, 40), (8, 8))
    assert not bad.any()
    check_noise_sweep(sse, count, target)


# ------------------------------------------------------------------ the library's host side
def test_chunk_restatement_matches_the_library():
    from ap_gym_amd import _native as N

    lib = N.lib()
    for m in (0, 1, 2, 3, 7, 15, 16, 17, 100, 1023, 1024, 1025, 65536, 2**31):
        for k in (0, 1, 7, 8, 9, 31, 63, 64, 65, 255, 256, 1000, 4096, 100000):
            assert lib.apg_image_overlap_chunk(m, k) == N.overlap_scores_chunk(m, k), (m, k)
    assert N.overlap_scores_chunk(1, 4096) == 8 and N.overlap_scores_chunk(65536, 256) == 64


def test_args_struct_matches_the_c_header(tmp_path):
    import os
    import shutil
    import subprocess

    from ap_gym_amd import _native as N

    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    py, cname = N.OverlapScoresArgs, "apg_overlap_scores_args"
    lines = ["#include <stdio.h>", "#include \"apgym_capi.h\"", "int main(void) {",
             f'  printf("size %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(conftest.ROOT, "include"), str(tmp_path / "layout.c"), "-o",
                    str(tmp_path / "layout")], check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(py)
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f


def test_c_entry_refuses_bad_arguments_without_a_device():
    from ap_gym_amd import _native as N

    lib = N.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def args(**kw):
        a = N.OverlapScoresArgs(glimpse=p, target_glimpse=p, glimpse_pos=p, hypotheses=p, sse=p, count=p, m=1, k=1,
                                height=28, width=28, sensor_h=5, sensor_w=5, channels=1, sensor_scale=1.0)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    for kw, text in ((dict(sensor_h=65, sensor_w=64), "at most 4096"), (dict(channels=0), "positive"),
                     (dict(sensor_scale=0.0), "sensor_scale"), (dict(m=-1), "m and k"), (dict(height=1), "2 x 2"),
                     (dict(logw=p), "go together"), (dict(logw_out=p), "go together"),
                     (dict(sse=None), "null"), (dict(m=2**31, k=65), "too many workgroups")):
        assert lib.apg_image_overlap_scores(ctypes.byref(args(**kw)), None) == N.APG_E_INVALID, kw
        assert text in lib.apg_last_error().decode(), (kw, lib.apg_last_error())
    assert lib.apg_image_overlap_scores(None, None) == N.APG_E_INVALID
    assert lib.apg_image_overlap_scores(ctypes.byref(args(m=0)), None) == N.APG_OK  # nothing to launch


# ------------------------------------------------------------------ argument checks of the Python entry (CPU tensors)
def test_python_entry_checks_arguments_before_the_device():
    import torch

    import ap_gym_amd as ap

    m, k, sensor = 3, 5, (4, 6)
    g = torch.zeros((m, *sensor, 1))
    q = torch.zeros((m, 2))
    h = torch.zeros((m, k, 2), dtype=torch.float64)
    lw = torch.zeros((m, k))
    geo = dict(image_size=(20, 30), sensor_size=sensor)

    def call(*a, **kw):
        return ap.image_overlap_scores(*a, **{**geo, **kw})

    with pytest.raises(TypeError, match="glimpse must be a float32"):
        call(g.double(), q, g, h)
    with pytest.raises(TypeError, match="target_glimpse must be a float32"):
        call(g, q, g.numpy(), h)
    with pytest.raises(TypeError, match="glimpse_pos must be a float64 or float32"):
        call(g, q.half(), g, h)
    with pytest.raises(TypeError, match="hypotheses must be a float64 or float32"):
        call(g, q, g, h.long())
    with pytest.raises(ValueError, match="glimpse must have shape"):
        call(g[:, :3], q, g[:, :3], h)
    with pytest.raises(ValueError, match="target_glimpse must have the glimpse's shape"):
        call(g, q, g[:2], h)
    with pytest.raises(ValueError, match="glimpse_pos must have shape"):
        call(g, q[:2], g, h)
    with pytest.raises(ValueError, match="hypotheses must have shape"):
        call(g, q, g, h[:2])
    with pytest.raises(ValueError, match="hypotheses must have shape"):
        call(g, q, g, h[..., :1])
    with pytest.raises(ValueError, match="at most 4096 values"):
        ap.image_overlap_scores(torch.zeros((1, 37, 37, 3)), q[:1], torch.zeros((1, 37, 37, 3)), h[:1],
                                image_size=(64, 64), sensor_size=(37, 37))
    with pytest.raises(ValueError, match="sensor_scale"):
        call(g, q, g, h, sensor_scale=0.0)
    with pytest.raises(ValueError, match="at least 2 x 2"):
        ap.image_overlap_scores(g, q, g, h, image_size=(1, 30), sensor_size=sensor)
    with pytest.raises(ValueError, match="logw_out needs logw"):
        call(g, q, g, h, logw_out=lw)
    with pytest.raises(TypeError, match="logw must be a float32"):
        call(g, q, g, h, logw=lw.double())
    with pytest.raises(ValueError, match="logw must have shape"):
        call(g, q, g, h, logw=lw[:, :4])
    with pytest.raises(ValueError, match="logw_out must have shape"):
        call(g, q, g, h, logw=lw, logw_out=lw[:2])
    # aliasing: logw_out may be logw itself, nothing else
    flat = torch.zeros(m * k + 1)
    with pytest.raises(ValueError, match="overlaps logw partially"):
        call(g, q, g, h, logw=flat[:-1].view(m, k), logw_out=flat[1:].view(m, k))
    hf = torch.zeros((m, k, 2))
    with pytest.raises(ValueError, match="logw_out overlaps hypotheses"):
        call(g, q, g, hf, logw=lw, logw_out=hf.view(-1)[:m * k].view(m, k))
    # everything else is fine: only now the device is looked at, and there is no CPU fallback
    for kw in (dict(), dict(logw=lw), dict(logw=lw, logw_out=lw), dict(logw=lw, logw_out=torch.zeros((m, k)))):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call(g, q, g, h, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):
        call(g, q.double(), g, h[0].float())  # [K, 2] shared hypotheses
