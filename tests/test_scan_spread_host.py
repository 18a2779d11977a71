"""lidar_scan_spread without a GPU: the restatement of steps 1 and 3-7 of the definition in include/apgym_capi.h
(`scan_spread_np`, which tests/test_gpu_scan_spread.py applies to lidar_scan_poses' scans and compares the kernel
with), the restatement's own properties, the Python argument checks, the C ABI's host-side validation and the struct
layout.
"""

import ctypes
from fractions import Fraction

import numpy as np
import pytest

F = np.float32
TWO24 = 1 << 24


def scan_spread_np(scans, weight=None):
    """Steps 1 and 3-7 of apg_lidar_scan_spread on numpy arrays: scans float32 [M, A, K, B], the normalised scans of
    the hypotheses (a NaN anywhere in a hypothesis' scan: its pose was not scanned, weight 0 for that (m, a) only);
    weight float32 [M, K] or None.  The sums and N are Python ints, the conversion of N is float(int) (round to
    nearest even), the rest numpy float64.  Returns a dict: spread float32 [M, A], mean float32 [M, A, B], err, and the
    integers S0 [M][A], S1, S2 [M][A][B] and N [M][A] as nested lists."""
    scans = np.asarray(scans, F)
    m, a, k, b = scans.shape
    err = 0
    if weight is None:
        q = np.full((m, k), TWO24, np.int64)
    else:
        w = np.asarray(weight, F)
        with np.errstate(invalid="ignore"):
            ok = (w >= 0) & (w <= 1)  # (false for a NaN)
        q = np.where(ok, np.rint(np.where(ok, w, 0) * F(TWO24)), 0).astype(np.int64)  # round half to even
        err |= 0 if ok.all() else 256
    dead = np.isnan(scans).any(axis=-1)  # [M, A, K]
    err |= 256 if dead.any() else 0
    v = np.rint(np.where(dead[..., None], 0, scans) * F(4096)).astype(np.int64)  # exact product, half to even
    assert np.abs(v).max(initial=0) <= 4096
    spread, mean = np.zeros((m, a), F), np.zeros((m, a, b), F)
    S0s, S1s, S2s, Ns = [], [], [], []
    for i in range(m):
        S0s.append([]), S1s.append([]), S2s.append([]), Ns.append([])
        for c in range(a):
            qc = [0 if dead[i, c, j] else int(q[i, j]) for j in range(k)]
            vc = v[i, c].tolist()
            S0 = sum(qc)
            S1 = [sum(qc[j] * vc[j][bb] for j in range(k)) for bb in range(b)]
            S2 = [sum(qc[j] * vc[j][bb] * vc[j][bb] for j in range(k)) for bb in range(b)]
            n = sum(S0 * S2[bb] - S1[bb] * S1[bb] for bb in range(b))
            assert n >= 0 and S0 <= 1 << 36 and max(S2) <= 1 << 60 and max(map(abs, S1)) <= 1 << 48
            S0s[i].append(S0), S1s[i].append(S1), S2s[i].append(S2), Ns[i].append(n)
            if S0 == 0:
                spread[i, c], mean[i, c] = np.nan, np.nan
                continue
            s0 = np.float64(S0)
            spread[i, c] = F((np.float64(float(n)) / (s0 * s0)) * np.float64(2.0 ** -24))
            mean[i, c] = ((np.array([float(x) for x in S1], np.float64) / s0) * np.float64(2.0 ** -12)).astype(F)
    return dict(spread=spread, mean=mean, err=err, S0=S0s, S1=S1s, S2=S2s, N=Ns)


def grid_weights(rng, shape):
    """Random float32 weights in [0, 1] that are multiples of 2^-24 (so q / 2^24 is the weight itself)."""
    return (rng.integers(0, TWO24 + 1, shape).astype(np.float64) / TWO24).astype(F)


SELF_SHAPES = [(1, 1, 1, 1), (2, 3, 2, 3), (1, 2, 7, 5), (2, 1, 33, 4), (1, 1, 300, 2)]


@pytest.mark.parametrize("shape", SELF_SHAPES)
def test_restatement_equals_the_exact_variance_of_the_quantised_values(shape):
    """Self-check 1: N / S0^2 / 2^24 is the weighted variance of v / 4096, summed over the beams, as a Fraction; the
    restatement rounds it as the definition says (u128 -> f64, one multiply, one divide, the exact scale)."""
    rng = np.random.default_rng(sum(shape))
    m, a, k, b = shape
    scans = rng.uniform(-1, 1, shape).astype(F)
    w = grid_weights(rng, (m, k))
    w[:, 0] = 1.0
    r = scan_spread_np(scans, w)
    v = np.rint(scans * F(4096)).astype(np.int64)
    q = np.rint(w * F(TWO24)).astype(np.int64)
    for i in range(m):
        for c in range(a):
            W = sum(Fraction(int(x)) for x in q[i])
            var = Fraction(0)
            for bb in range(b):
                z = [Fraction(int(x), 4096) for x in v[i, c, :, bb]]
                mu = sum(Fraction(int(qq)) * zz for qq, zz in zip(q[i], z)) / W
                var += sum(Fraction(int(qq)) * (zz - mu) ** 2 for qq, zz in zip(q[i], z)) / W
                assert F(float(mu)) == r["mean"][i, c, bb]
            S0, n = r["S0"][i][c], r["N"][i][c]
            assert Fraction(n, S0 * S0) == var * (1 << 24)  # the integers hold the variance exactly
            want = F((np.float64(float(n)) / (np.float64(S0) * np.float64(S0))) * np.float64(2.0 ** -24))
            assert r["spread"][i, c] == want
            assert abs(float(r["spread"][i, c]) - float(var)) <= float(var) * 2.0 ** -22 + 1e-300


@pytest.mark.parametrize("shape", SELF_SHAPES)
def test_restatement_agrees_with_the_unquantised_variance(shape):
    """Self-check 2: each reading moves by delta <= 2^-13 inside [-1, 1] when it is quantised, so a weighted variance
    (of values and a mean in [-1, 1]) moves by at most 4 delta + delta^2 < 2^-10, and the sum over beams by B 2^-10.
    The weights are multiples of 2^-24: they are not rounded."""
    rng = np.random.default_rng(7 + sum(shape))
    m, a, k, b = shape
    scans = rng.uniform(-1, 1, shape).astype(F)
    w = grid_weights(rng, (m, k))
    w[:, -1] = 0.5
    r = scan_spread_np(scans, w)
    z, wn = scans.astype(np.float64), (w.astype(np.float64) / w.astype(np.float64).sum(1, keepdims=True))[:, None, :, None]
    mu = (wn * z).sum(2, keepdims=True)
    var = (wn * (z - mu) ** 2).sum(2).sum(-1)
    assert np.abs(r["spread"].astype(np.float64) - var).max() <= b * 2.0 ** -10
    assert np.abs(r["mean"].astype(np.float64) - mu[:, :, 0]).max() <= 2.0 ** -13 + 2.0 ** -23


def test_restatement_is_invariant_under_permutation_and_weight_splitting():
    """Self-checks 3 and 4: bit-identical under a permutation of the hypotheses (with their weights), and when a
    hypothesis of weight 1 is replaced by two of weight 0.5 at the same scan."""
    rng = np.random.default_rng(3)
    m, a, k, b = 2, 3, 9, 5
    scans = rng.uniform(-1, 1, (m, a, k, b)).astype(F)
    w = rng.random((m, k)).astype(F)
    w[:, 4] = 1.0
    r = scan_spread_np(scans, w)
    perm = rng.permutation(k)
    rp = scan_spread_np(scans[:, :, perm], w[:, perm])
    assert np.array_equal(r["spread"].view(np.uint32), rp["spread"].view(np.uint32))
    assert np.array_equal(r["mean"].view(np.uint32), rp["mean"].view(np.uint32))
    assert r["N"] == rp["N"] and r["S1"] == rp["S1"]
    split_scans = np.concatenate([scans, scans[:, :, 4:5]], axis=2)
    split_w = np.concatenate([w, np.full((m, 1), 0.5, F)], axis=1)
    split_w[:, 4] = 0.5
    rs = scan_spread_np(split_scans, split_w)
    assert np.array_equal(r["spread"].view(np.uint32), rs["spread"].view(np.uint32))
    assert np.array_equal(r["mean"].view(np.uint32), rs["mean"].view(np.uint32))
    assert r["N"] == rs["N"] and r["S0"] == rs["S0"]


def test_restatement_zero_nan_and_the_bound():
    """Self-checks 5 and 6, and the domain: equal scans give exactly 0 (also when they differ by less than the
    quantum); K = 4096 at weight 1 with every reading 1.0 reaches S2_b == 2^60 and spread 0; dead hypotheses."""
    rng = np.random.default_rng(5)
    row = rng.uniform(-1, 1, 6).astype(F)
    scans = np.broadcast_to(row, (1, 2, 11, 6)).copy()
    r = scan_spread_np(scans, rng.random((1, 11)).astype(F))
    assert (r["spread"] == 0).all() and r["err"] == 0
    assert np.array_equal(r["mean"][0, 0], (np.rint(row * F(4096)) / 4096).astype(F))
    scans[0, 1, 3, 2] = np.nextafter(scans[0, 1, 3, 2], F(2))  # below the quantum (unless it sits on a tie)
    scans[0, 0, 5, 0] = -row[0] if abs(row[0]) > 0.01 else F(0.5)
    r = scan_spread_np(scans)
    assert r["spread"][0, 0] > 0 and r["spread"][0, 1] == 0
    big = scan_spread_np(np.ones((1, 1, 4096, 2), F))
    assert big["S2"][0][0] == [1 << 60, 1 << 60] and big["S0"][0][0] == 1 << 36 and big["S1"][0][0][0] == 1 << 48
    assert big["spread"][0, 0] == 0 and big["mean"][0, 0, 0] == 1
    # the domain: a NaN scan drops the hypothesis from its own (m, a) only; bad weights count as 0; both flag
    scans = rng.uniform(-1, 1, (1, 2, 3, 2)).astype(F)
    scans[0, 0, 1] = np.nan
    r = scan_spread_np(scans, np.array([[1, 0.5, 0.25]], F))
    assert r["err"] == 256 and r["S0"][0] == [TWO24 + TWO24 // 4, TWO24 + TWO24 // 2 + TWO24 // 4]
    keep = scan_spread_np(scans[:, :1, [0, 2]], np.array([[1, 0.25]], F))
    assert keep["err"] == 0 and r["spread"][0, 0] == keep["spread"][0, 0]
    r = scan_spread_np(scans[:, 1:], np.array([[np.nan, -0.5, 1.5]], F))
    assert r["err"] == 256 and np.isnan(r["spread"]).all() and np.isnan(r["mean"]).all() and r["S0"][0] == [0]
    r = scan_spread_np(scans[:, 1:], np.array([[0, 0, 2.0 ** -26]], F))
    assert r["err"] == 0 and np.isnan(r["spread"]).all()  # weights that round to q = 0: no error, no belief


def test_scan_spread_argument_checks():
    """Dtype, rank and shape errors come first, on tensors of any device; the device is refused last."""
    import torch

    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    bits = torch.zeros((3, 8, 1), dtype=torch.int64)
    poses = torch.zeros((3, 2, 5, 2))

    def bad(exc, match, b=bits, width=8, p=poses, weight=None, map_ids=None, beams=4, lidar_range=2.0, **kw):
        with pytest.raises(exc, match=match):
            ap.lidar_scan_spread(b, width, p, weight, map_ids, beams=beams, lidar_range=lidar_range, **kw)

    bad(TypeError, "poses must be a float32", p=poses.double())
    bad(TypeError, "poses must be a float32", p=poses.numpy())
    bad(ValueError, r"\[M, A, K, 2\]", p=poses[0])
    bad(ValueError, r"\[M, A, K, 2\]", p=torch.zeros((3, 2, 5, 3)))
    bad(ValueError, "A must be >= 1", p=torch.zeros((3, 0, 5, 2)))
    bad(ValueError, "K must be in 1..4096", p=torch.zeros((3, 2, 0, 2)))
    bad(ValueError, "K must be in 1..4096", p=torch.zeros((3, 1, N.SCAN_SPREAD_MAX_K + 1, 2)))
    bad(TypeError, "bits must be an int64", b=bits.to(torch.int32))
    bad(ValueError, "words per row", width=65)
    bad(ValueError, "beams must be in", beams=0)
    bad(ValueError, "beams must be in 1..1024", beams=N.SCAN_SPREAD_MAX_BEAMS + 1)
    bad(ValueError, "lidar_range must be in", lidar_range=0.0)
    bad(ValueError, "lidar_range must be in", lidar_range=61.0)
    bad(TypeError, "weight must be a float32", weight=torch.zeros((3, 5), dtype=torch.float64))
    bad(TypeError, "weight must be a float32", weight=np.zeros((3, 5), F))
    bad(ValueError, "weight must have shape", weight=torch.zeros((3, 2, 5)))
    bad(ValueError, "weight must have shape", weight=torch.zeros((3, 4)))
    bad(TypeError, "map_ids must be a 1-d int64", map_ids=torch.zeros(3, dtype=torch.int32))
    bad(ValueError, "one id per pose set", map_ids=torch.zeros(2, dtype=torch.int64))
    bad(ValueError, "one map or one per pose set", b=bits[:2])
    bad(TypeError, "out must be a float32", out=torch.zeros((3, 2), dtype=torch.float64))
    bad(ValueError, "out must have shape", out=torch.zeros((3, 2, 1)))
    # every check above came first: there is no CPU fallback
    bad(ValueError, "GPU.*no CPU fallback")
    bad(ValueError, "GPU", weight=torch.zeros((3, 5)), map_ids=torch.zeros(3, dtype=torch.int64), mean=True,
        out=torch.zeros((3, 2)))
    assert (N.SCAN_SPREAD_TILE, N.SCAN_SPREAD_MAX_K, N.SCAN_SPREAD_MAX_BEAMS, N.SCAN_SPREAD_MAX_GRID) == (
        256, 4096, 1024, 8192)
    assert ap.ScanSpreadResult._fields == ("spread", "mean")


def test_scan_spread_c_abi_validates_on_the_host():
    from ap_gym_amd import _native as N

    fn = N.lib().apg_lidar_scan_spread
    bufs = [(ctypes.c_float * 64)() for _ in range(8)]
    p = [ctypes.addressof(b) for b in bufs]

    def call(**over):
        a = N.ScanSpreadArgs(occ=p[0], map_ids=None, poses=p[1], beam_dirs=p[2], weight=p[3], spread=p[4], mean=p[5],
                             err=None, n_src=1, m=2, height=8, width=8, a=2, k=4, beams=4, lidar_range=2.0)
        for name, v in over.items():
            setattr(a, name, v)
        return fn(ctypes.byref(a), None)

    def last():
        return N.lib().apg_last_error().decode()

    for kw, text in ((dict(k=0), "k must be in 1..4096"), (dict(k=4097), "k must be in 1..4096"),
                     (dict(k=-1), "k must be in 1..4096"), (dict(a=0), "a must be >= 1"), (dict(a=-3), "a must be >= 1"),
                     (dict(beams=0), "beams must be in 1..1024"), (dict(beams=1025), "beams must be in 1..1024"),
                     (dict(height=0), "height and width must be in 1..511"),
                     (dict(width=512), "height and width must be in 1..511"),
                     (dict(lidar_range=0.0), "lidar_range must be in (0, 60]"),
                     (dict(lidar_range=60.5), "lidar_range must be in (0, 60]"),
                     (dict(lidar_range=float("nan")), "lidar_range must be in (0, 60]"),
                     (dict(m=-1), "m and n_src must be >= 0"), (dict(n_src=-1), "m and n_src must be >= 0"),
                     (dict(spread=None, mean=None), "neither spread nor mean"),
                     (dict(poses=None), "null occ / poses / beam_dirs"),
                     (dict(beam_dirs=None), "null occ / poses / beam_dirs"),
                     (dict(occ=None), "null occ / poses / beam_dirs"),
                     (dict(n_src=3, m=4), "one map or a map per set")):
        assert call(**kw) == N.APG_E_INVALID, kw
        assert text in last() and last().startswith("scan_spread:"), (kw, last())
    assert fn(None, None) == N.APG_E_INVALID and "null arguments" in last()
    # m == 0 launches nothing, whatever the pointers hold -- but the scalars are validated first
    assert call(m=0) == N.APG_OK
    assert call(m=0, poses=None, beam_dirs=None, occ=None, weight=None, mean=None) == N.APG_OK
    assert call(m=0, k=0) == N.APG_E_INVALID and call(m=0, spread=None, mean=None) == N.APG_E_INVALID
    assert ctypes.sizeof(N.ScanSpreadArgs) == 8 * 8 + 2 * 8 + 5 * 4 + 4


def test_scan_spread_struct_layout_matches_the_c_header(tmp_path):
    """The ctypes mirror of apg_scan_spread_args has the size and field offsets gcc gives include/apgym_capi.h."""
    import os
    import subprocess

    from ap_gym_amd import _native as N

    cname, py = "apg_scan_spread_args", N.ScanSpreadArgs
    lines = ["#include <stdio.h>", "#include \"apgym_capi.h\"", "int main(void) {",
             f'  printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                              text=True).stdout.splitlines())
    assert int(got[cname]) == ctypes.sizeof(py)
    for fname, _ in py._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, fname


def test_scan_spread_op_is_registered():
    import torch

    from ap_gym_amd import _native as N

    ops = N.torch_ops()
    assert callable(ops.lidar_scan_spread)
    schema = str(torch.ops.apgym.lidar_scan_spread.default._schema)
    for name in ("bits", "width", "poses", "weight", "map_ids", "beam_dirs", "lidar_range", "spread", "mean", "err"):
        assert f" {name}" in schema, (name, schema)
    with pytest.raises(RuntimeError, match="GPU"):  # the op itself refuses a CPU tensor: no fallback
        ops.lidar_scan_spread(torch.zeros((1, 8, 1), dtype=torch.int64), 8, torch.zeros((1, 1, 2, 2)), None, None,
                              torch.zeros((4, 2)), 2.0, torch.zeros((1, 1)), None, None)


def test_action_spread_is_on_the_env_and_the_filter():
    import ap_gym_amd as ap

    assert callable(ap.LIDARLocalization2DVectorEnv.action_spread)
    assert callable(ap.LidarParticleFilter.action_spread) and callable(ap.LidarParticleFilter.choose_action)
