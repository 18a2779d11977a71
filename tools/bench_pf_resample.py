#!/usr/bin/env python
"""Measure k_pf_resample (lidar_pf_resample) on one GPU against the chain of torch ops a user had to write for the
same result.

    python tools/bench_pf_resample.py [--runs 3] [--launches 10] [--out profiles/pf_resample.json]

Prints one JSON line.  The driver itself never touches the GPU: every shape runs in a child process of its own under
`timeout -k 10 <seconds>`, and the first one that fails (or times out) ends the run.

  new     lidar_pf_resample: the seven output tensors allocated, then one launch of k_pf_resample: weight, estimate,
          ess, index, poses, logw and resampled of M sets of K particles
  kernel  the same launch through the C ABI into outputs allocated once: at small shapes `new` is bound by the host
          (seven torch.empty and the op's dispatch), this is the kernel itself
  parent  the same definition in torch, on the same integers: l = logw - scale * scores, max, exp, rint to int64, the
          sums, cumsum, the ESS and the weighted mean in float64, the thresholds T in int64, torch.searchsorted, two
          gathers and the where()s of the decision.  torch.exp is not required to round as the kernel's expf does, so
          the weights that differ in their last bit are counted, and the indices are compared twice: as timed, and
          (untimed) with the parent chain given the kernel's weights, where they must be equal.

Shapes: (a) M = 65 536, K = 64; (b) M = 65 536, K = 16; (c) M = 4 096, K = 1 024; (d) M = 16, K = 4 096.  logw ~ N(0, 1),
scores uniform in [0, 8], score_scale 0.5, poses uniform in a 64 x 64 map, ess_frac 0.5.  For (a), env.pose_scores at 32
beams on 64 x 64 rooms is timed in the same run: the resample's share of a filter step.

Every timing is the median of `--launches` launches between device events, taken `--runs` times with the two sides
alternating inside a run; the runs' medians are all reported with their spread (max - min) / median.  Clocks as found.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "active-perception-gym_amd"))

SHAPES = {"a": (65536, 64), "b": (65536, 16), "c": (4096, 1024), "d": (16, 4096)}
QUICK = {"a": (512, 64), "b": (512, 16), "c": (32, 1024), "d": (2, 4096)}
CHILD_SECONDS = 300
SCALE, ESS_FRAC, SIDE, SCAN_BEAMS = 0.5, 0.5, 64, 32
TWO24 = 1 << 24


def summary(per_run: list[float]) -> dict:
    med = statistics.median(per_run)
    return {"median": med, "runs": per_run, "spread": (max(per_run) - min(per_run)) / med if med else 0.0}


def time_launches(fn, launches: int) -> float:
    """Median device time (us) of `launches` calls of fn, each between its own pair of events."""
    import torch

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for b, e in ev:
        b.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(b.elapsed_time(e) * 1e3 for b, e in ev)


def child(args) -> int:
    import torch

    if not torch.cuda.is_available():
        print("bench_pf_resample: needs a GPU (nothing is measured without one)", file=sys.stderr)
        return 2
    import ctypes

    import ap_gym_amd as ap
    from ap_gym_amd import _native as N

    m, k = QUICK[args.shape] if args.quick else SHAPES[args.shape]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    logw = torch.randn((m, k), device=dev, generator=g)
    scores = torch.rand((m, k), device=dev, generator=g) * 8.0
    poses = torch.rand((m, k, 2), device=dev, generator=g) * SIDE
    u = torch.rand(m, device=dev, generator=g)
    slots = torch.arange(k, dtype=torch.int64, device=dev)[None]
    out = {}

    def new():
        out["new"] = ap.lidar_pf_resample(poses, logw, scores, score_scale=SCALE, u=u, ess_frac=ESS_FRAC)

    keep = ap.lidar_pf_resample(poses, logw, scores, score_scale=SCALE, u=u, ess_frac=ESS_FRAC)  # the outputs' storage
    c_args = N.PfResampleArgs(logw=logw.data_ptr(), score=scores.data_ptr(), poses=poses.data_ptr(), u=u.data_ptr(),
                              weight=keep.weight.data_ptr(), estimate=keep.estimate.data_ptr(),
                              ess=keep.ess.data_ptr(), index=keep.index.data_ptr(), poses_out=keep.poses.data_ptr(),
                              logw_out=keep.logw.data_ptr(), resampled=keep.resampled.data_ptr(), m=m, k=k,
                              score_scale=SCALE, ess_frac=ESS_FRAC)
    c_fn, c_stream = N.lib().apg_lidar_pf_resample, N.current_stream_ptr(dev)

    def kernel():
        N.check(c_fn(ctypes.byref(c_args), c_stream), "apg_lidar_pf_resample")

    def chain(weight=None):
        l = logw - SCALE * scores
        d = l - l.max(dim=1, keepdim=True).values
        w = torch.exp(d) if weight is None else weight
        q = torch.round(w * float(TWO24)).to(torch.int64)  # (round half to even)
        big, s2 = q.sum(dim=1), (q * q).sum(dim=1)
        ess64 = big.double() * big.double() / s2.double()
        est = ((q.double()[:, :, None] * poses.double()).sum(dim=1) / big.double()[:, None]).float()
        res = ess64 < ESS_FRAC * k
        cum = q.cumsum(dim=1)
        uu = torch.floor(u * float(TWO24)).clamp(0, TWO24 - 1).to(torch.int64)
        thr = slots * big[:, None] // k + (uu * big // (k * TWO24))[:, None]
        idx = torch.where(res[:, None], torch.searchsorted(cum, thr, right=True), slots)
        pos = torch.gather(poses, 1, idx[:, :, None].expand(m, k, 2))
        lw = torch.where(res[:, None], torch.zeros_like(d), d)
        return w, est, ess64.float(), idx, pos, lw, res

    def parent():
        out["parent"] = chain()

    for fn in (new, parent):  # warm up both sides at the timed shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    r, q = out["new"], out["parent"]
    res = {"M": m, "K": k, "particles": m * k}
    # results first, at the timed size
    res["weight_not_bit_equal"] = int((r.weight.view(torch.int32) != q[0].view(torch.int32)).sum())
    l = logw - SCALE * scores
    ref = torch.exp((l - l.max(dim=1, keepdim=True).values).double())  # float64 exp of the float32 d
    ulp = torch.exp2(torch.floor(torch.log2(ref)) - 23)
    res["weight_max_ulp_vs_f64_exp"] = float(((r.weight.double() - ref).abs() / ulp).max())
    del l, ref, ulp
    res["sets_resampled"] = int(r.resampled.sum())
    res["resampled_differ"] = int((r.resampled.bool() != q[6]).sum())
    res["index_differ_as_timed"] = int((r.index.long() != q[3]).sum())
    given = chain(r.weight)  # the same integers: must be equal
    res["index_differ_given_the_kernels_weights"] = int((r.index.long() != given[3]).sum())
    res["poses_differ_given_the_kernels_weights"] = int((r.poses != given[4]).sum())
    res["ess_not_bit_equal_given_the_kernels_weights"] = int((r.ess.view(torch.int32) != given[2].view(torch.int32)).sum())
    res["estimate_max_abs_diff_given_the_kernels_weights"] = float((r.estimate - given[1]).abs().max())
    del given
    out.clear()
    runs = {"new": [], "parent": [], "kernel": []}
    scan = None
    if args.shape == "a":
        env = ap.LIDARLocalization2DVectorEnv(num_envs=m, dataset=ap.FloorMapDatasetRooms(SIDE, SIDE), device=dev,
                                              array_backend="torch", map_obs="bits", lidar_beam_count=SCAN_BEAMS)
        env.reset(seed=0)
        score_out = torch.empty((m, k), dtype=torch.float32, device=dev)

        def scan():
            env.pose_scores(poses, out=score_out)

        scan()
        runs["scan"] = []
    for run in range(args.runs):  # alternate inside a run, either side first in turn
        for name, fn in (("new", new), ("parent", parent))[::-1 if run % 2 else 1]:
            runs[name].append(time_launches(fn, args.launches))
            out.clear()
        runs["kernel"].append(time_launches(kernel, args.launches))
        if scan is not None:
            runs["scan"].append(time_launches(scan, args.launches))
    res["new_us"], res["parent_us"] = summary(runs["new"]), summary(runs["parent"])
    res["kernel_us"] = summary(runs["kernel"])
    res["parent_over_new"] = res["parent_us"]["median"] / res["new_us"]["median"]
    # bytes the kernel must move: logw, scores, poses in; weight, index, poses, logw out (4 + 4 + 8 + 4 + 4 + 8 + 4)
    res["kernel_GB_per_s"] = 36.0 * m * k / res["kernel_us"]["median"] / 1e3
    if scan is not None:
        res["pose_scores_32_beams_us"] = summary(runs["scan"])
        res["resample_share_of_update"] = res["new_us"]["median"] / (
            res["new_us"]["median"] + res["pose_scores_32_beams_us"]["median"])
        res["parent_share_of_update"] = res["parent_us"]["median"] / (
            res["parent_us"]["median"] + res["pose_scores_32_beams_us"]["median"])
        env.check_errors()
        env.close()
    print(json.dumps(res))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--shape", default=None, help=argparse.SUPPRESS)  # the child's shape
    ap.add_argument("--out", default=None, help="also write the result (indented) to this file")
    args = ap.parse_args()
    if args.shape:
        return child(args)
    result = {"tool": "tools/bench_pf_resample.py", "runs": args.runs, "launches": args.launches, "quick": args.quick,
              "score_scale": SCALE, "ess_frac": ESS_FRAC}
    rc = 0
    for name in args.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--shape", name,
               "--runs", str(args.runs), "--launches", str(args.launches)] + (["--quick"] if args.quick else [])
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if proc.returncode != 0:  # a failed or timed-out shape ends the run: nothing more starts on the GPU
            result[name] = {"failed": proc.returncode}
            rc = 1
            break
        result[name] = json.loads(proc.stdout.strip().splitlines()[-1])
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    print(json.dumps(result))
    return rc


if __name__ == "__main__":
    sys.exit(main())
