#!/usr/bin/env python
"""Measure k_glimpse_scores (image_glimpse_scores) on one GPU against what the library offered before it for the same
result.

    python tools/bench_glimpse_scores.py [--runs 3] [--launches 10] [--out profiles/glimpse_scores.json]

Prints one JSON line.  The driver itself never touches the GPU: every shape runs in a child process of its own under
`timeout -k 10 <seconds>`, and the first one that fails (or times out) ends the run.

  new     one launch of k_glimpse_scores: the scores [M, K]; no glimpse is written to memory
  parent  apg_image_glimpse (k_glimpse_sep) into a float32 [M, K, s0, s1, C] tensor, then torch's
          ((g - o[:, None]) ** 2).mean((-3, -2, -1))

Shapes: (a) MNIST-shaped 28 x 28 u8, sensor 5 x 5, M = 65 536, K = 16; (b) TinyImageNet-shaped 64 x 64 RGB in the tiled
pool layout, sensor 12 x 12, M = 32 768, K = 16; (c) the same with K = 64; (d) one template search on the pool of (b):
M = 1 024 with K = 1 024 positions, a 32 x 32 linspace grid over [-1, 1]^2 (the form of the unique sampler's grid).
Pools are random bytes (300 images); indices and, except in (d), positions are uniform; `observed` is each set's
glimpse at a random position.

Every timing is the median of `--launches` launches between device events, taken `--runs` times with the two sides
alternating inside a run; the runs' medians are all reported with their spread (max - min) / median.  Clocks as found.
Before timing, both sides' results are compared at the timed size: the parent's scores come from torch's reduction,
which sums in another order, so the largest difference is reported, not asserted to be zero; the glimpses behind the
scores (new: glimpse_out of a second launch) must be equal bit for bit.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "active-perception-gym_amd"))

#         M, K, image (H, W, C), sensor, positions
SHAPES = {"a": (65536, 16, (28, 28, 1), (5, 5), "uniform"),
          "b": (32768, 16, (64, 64, 3), (12, 12), "uniform"),
          "c": (32768, 64, (64, 64, 3), (12, 12), "uniform"),
          "d": (1024, 1024, (64, 64, 3), (12, 12), "grid")}
QUICK = {"a": (512, 16), "b": (256, 16), "c": (256, 64), "d": (8, 1024)}
POOL_LEN = 300
CHILD_SECONDS = 300


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
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        print("bench_glimpse_scores: needs a GPU (nothing is measured without one)", file=sys.stderr)
        return 2
    import ap_gym_amd as ap
    from ap_gym_amd import _native as N
    from ap_gym_amd import image_env as ie

    m, k, (h, w, c), sensor, how = SHAPES[args.shape]
    if args.quick:
        m, k = QUICK[args.shape]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    host = rng.integers(0, 256, (POOL_LEN, h, w, c), dtype=np.uint8)
    tiled = c == 3
    pool = ie.device_pool_u8_tiled(host, dev) if tiled else ie.device_pool_u8(host, dev)
    geo = dict(image_size=(h, w), sensor_size=sensor, channels=c, tiled=tiled)
    g = torch.Generator(device=dev).manual_seed(0)
    index = torch.randint(0, POOL_LEN, (m,), device=dev, generator=g)
    if how == "grid":
        side = int(round(k ** 0.5))
        grid = np.stack(np.meshgrid(np.linspace(-1, 1, side), np.linspace(-1, 1, side), indexing="ij"), -1)
        pos = torch.as_tensor(grid.reshape(1, k, 2), device=dev).expand(m, k, 2).contiguous()
    else:
        pos = torch.rand((m, k, 2), dtype=torch.float64, device=dev, generator=g) * 2 - 1
    at = torch.rand((m, 1, 2), dtype=torch.float64, device=dev, generator=g) * 2 - 1
    observed = ap.image_glimpses_at(pool, index, at, **geo)[:, 0].contiguous()
    L = sensor[0] * sensor[1] * c
    score = torch.empty((m, k), dtype=torch.float32, device=dev)
    glim = torch.empty((m, k, *sensor, c), dtype=torch.float32, device=dev)
    cfg = N.ImageConfig(num_envs=m, kind=N.APG_IMAGE_CLASSIFY, height=h, width=w, pool_channels=c, channels=c,
                        pool_dtype=N.APG_POOL_U8_TILED if tiled else N.APG_POOL_U8, sensor_h=sensor[0],
                        sensor_w=sensor[1], step_limit=16, num_classes=10, invert_labels=0, top_k=10, unique_points=0,
                        num_envs_total=m, env_offset=0, pool_len=POOL_LEN, sensor_scale=1.0,
                        max_step=(ctypes.c_double * 2)(0.2, 0.2), cell=(ctypes.c_double * 2)(0.0, 0.0), ce_scale=1.0,
                        ce_offset=0.0, mse_scale=1.0, mse_offset=0.0)
    fn_glimpse, stream = N.lib().apg_image_glimpse, N.stream_handle(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    parent_out = {}

    def new():
        ap.image_glimpse_scores(pool, index, pos, observed, out=score, **geo)

    def parent():
        N.check(fn_glimpse(ctypes.byref(cfg), N.ptr(pool), N.ptr(index), N.ptr(pos), 0, k, N.ptr(glim), N.ptr(err),
                           stream), "apg_image_glimpse")
        parent_out["score"] = ((glim - observed[:, None]) ** 2).mean((-3, -2, -1))

    for fn in (new, parent):  # warm up both sides at the timed shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = {"M": m, "K": k, "image": [h, w, c], "pool": "u8 tiled" if tiled else "u8", "sensor": list(sensor), "L": L,
           "positions": how, "units": m * k}
    # results first: the same values from both sides
    both = torch.empty_like(glim)
    ap.image_glimpse_scores(pool, index, pos, observed, glimpse_out=both, **geo)
    res["glimpses_bit_equal"] = bool(torch.equal(both.view(torch.int32), glim.view(torch.int32)))
    del both
    res["scores_max_abs_diff_to_torch_mean"] = float((score - parent_out["score"]).abs().max())
    res["scores_max"] = float(score.max())
    res["err_bits"] = int(err.item())
    parent_out.clear()
    runs = {"new": [], "parent": []}
    for run in range(args.runs):  # alternate inside a run, either side first in turn
        for name, fn in (("new", new), ("parent", parent))[::-1 if run % 2 else 1]:
            runs[name].append(time_launches(fn, args.launches))
    res["new_us"], res["parent_us"] = summary(runs["new"]), summary(runs["parent"])
    res["parent_over_new"] = res["parent_us"]["median"] / res["new_us"]["median"]
    # bytes each side has to move through memory (the algorithm's, from the shapes: positions, index, observed,
    # scores, and for the parent six passes over [M, K, L] floats: the glimpses written and read, the differences
    # written and read, the squares written and read; the pool reads, equal on both sides and mostly cache hits, are
    # not counted)
    n = m * k * L
    common = m * k * 16 + m * 8 + m * L * 4 + m * k * 4
    res["bytes_new"], res["bytes_parent"] = common, common + 6 * n * 4
    res["new_units_per_us"] = m * k / res["new_us"]["median"]
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
    result = {"tool": "tools/bench_glimpse_scores.py", "runs": args.runs, "launches": args.launches,
              "quick": args.quick}
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
