#!/usr/bin/env python
"""Measure k_scan_spread (lidar_scan_spread) on one GPU against what a user wrote for the same quantity before it
existed, and against the scan alone.

    python tools/bench_scan_spread.py [--runs 3] [--launches 10] [--out profiles/scan_spread.json]

Prints one JSON line.  The driver itself never touches the GPU: every shape runs in a child process of its own under
`timeout -k 10 <seconds>`, and the first one that fails (or times out) ends the run.

  new     lidar_scan_spread into a preallocated [M, A] tensor: one launch, no scan written to memory
  scan    lidar_scan_poses alone on the same M * A * K * B rays, into a preallocated [M, A * K, B] tensor: the walk
          that `new` cannot do without, plus the store of every reading
  parent  lidar_scan_poses into [M, A * K, B], then the weighted variance in float64 torch ops: normalised weights,
          the weighted mean over K, the weighted squared deviations, the sums over K and B.  Its result depends on
          torch's reduction order; the largest difference from `new` is reported (the quantisation of `new` allows
          B * 2^-10, tests/test_scan_spread_host.py)

Shapes, on 64 x 64 rooms with 32 beams, poses uniform in the map, weights uniform in [0, 1]: (a) M = 1024, A = 8,
K = 256; (b) M = 65 536, A = 4, K = 16; (c) M = 1, A = 16, K = 4096 -- 16 workgroups on 256 CUs: the case the work
split leaves under-filled.

Every timing is the median of `--launches` launches between device events, taken `--runs` times with the sides
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

SHAPES = {"a": (1024, 8, 256), "b": (65536, 4, 16), "c": (1, 16, 4096)}
QUICK = {"a": (16, 8, 256), "b": (512, 4, 16), "c": (1, 2, 4096)}
CHILD_SECONDS = 300
SIDE, BEAMS, RANGE = 64, 32, 5.0


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
        print("bench_scan_spread: needs a GPU (nothing is measured without one)", file=sys.stderr)
        return 2
    import ap_gym_amd as ap
    from ap_gym_amd.map_bits import words_per_row

    m, a, k = QUICK[args.shape] if args.quick else SHAPES[args.shape]
    dev = torch.device("cuda:0")
    env = ap.LIDARLocalization2DVectorEnv(num_envs=m, dataset=ap.FloorMapDatasetRooms(SIDE, SIDE), device=dev,
                                          array_backend="torch", map_obs="bits", lidar_beam_count=BEAMS,
                                          lidar_range=RANGE)
    env.reset(seed=0)
    bits = env._t["occ"].view(m, SIDE, words_per_row(SIDE))
    g = torch.Generator(device=dev).manual_seed(0)
    poses = torch.rand((m, a, k, 2), device=dev, generator=g) * SIDE
    weight = torch.rand((m, k), device=dev, generator=g)
    flat = poses.view(m, a * k, 2)
    spread_out = torch.empty((m, a), dtype=torch.float32, device=dev)
    scan_out = torch.empty((m, a * k, BEAMS), dtype=torch.float32, device=dev)
    kw = dict(beams=BEAMS, lidar_range=RANGE, beam_dirs=env._t["beam_dirs"])
    out = {}

    def new():
        ap.lidar_scan_spread(bits, SIDE, poses, weight, out=spread_out, **kw)

    def scan():
        ap.lidar_scan_poses(bits, SIDE, flat, out=scan_out, **kw)

    def parent():
        ap.lidar_scan_poses(bits, SIDE, flat, out=scan_out, **kw)
        z = scan_out.view(m, a, k, BEAMS).double()
        w = weight.double()
        wn = (w / w.sum(dim=1, keepdim=True))[:, None, :, None]
        mu = (wn * z).sum(dim=2, keepdim=True)
        out["parent"] = (wn * (z - mu) ** 2).sum(dim=2).sum(dim=-1)

    for fn in (new, scan, parent):  # warm up every side at the timed shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = {"M": m, "A": a, "K": k, "beams": BEAMS, "rays": m * a * k * BEAMS}
    res["max_abs_diff_new_vs_parent"] = float((spread_out.double() - out["parent"]).abs().max())
    res["allowed_by_quantisation"] = BEAMS * 2.0 ** -10
    res["spread_mean"] = float(spread_out.double().mean())
    out.clear()
    sides = (("new", new), ("scan", scan), ("parent", parent))
    runs = {name: [] for name, _ in sides}
    for run in range(args.runs):  # alternate inside a run: the order turns by one each run
        for name, fn in sides[run % 3:] + sides[:run % 3]:
            runs[name].append(time_launches(fn, args.launches))
            out.clear()
    for name in runs:
        res[name + "_us"] = summary(runs[name])
    res["new_over_scan"] = res["new_us"]["median"] / res["scan_us"]["median"]
    res["parent_over_new"] = res["parent_us"]["median"] / res["new_us"]["median"]
    res["new_rays_per_us"] = res["rays"] / res["new_us"]["median"]
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
    result = {"tool": "tools/bench_scan_spread.py", "runs": args.runs, "launches": args.launches, "quick": args.quick,
              "map": f"{SIDE}x{SIDE} rooms", "beams": BEAMS, "lidar_range": RANGE}
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
