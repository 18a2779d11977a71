#!/usr/bin/env python
"""Measure k_overlap_scores (image_overlap_scores with the fused belief update) on one GPU against what the library
offered before it for the same result.

    python tools/bench_overlap_scores.py [--runs 3] [--launches 10] [--out profiles/overlap_scores.json]

Prints one JSON line.  The driver itself never touches the GPU: every shape runs in a child process of its own under
`timeout -k 10 <seconds>`, and the first one that fails (or times out) ends the run.

  new     one launch of k_overlap_scores: sse, count and the updated log-weights [M, K]
  parent  the same quantity composed from torch ops (the definition of apg_image_overlap_scores, include/apgym_capi.h:
          shifts in float64, gathers of the four taps, the bilinear prediction, squared error, mask and sum in
          float32), in chunks of sets so that its [sets, K, L] temporaries fit (about 16M elements each)

Shapes: (a) MNIST-shaped 28 x 28, sensor 5 x 5 x 1, M = 65 536, K = 256: a 16 x 16 linspace grid shared by all sets;
(b) TinyImageNet-shaped 64 x 64, sensor 12 x 12 x 3, M = 32 768, K = 1 024: a 32 x 32 grid; (c) as (b) with every
hypothesis within one sensor width of the glimpse position (per-set hypotheses), so everything overlaps.  Glimpses are
uniform random floats, glimpse positions uniform over [-1, 1]^2.

Every timing is the median of `--launches` launches between device events, taken `--runs` times with the two sides
alternating inside a run; the runs' medians are all reported with their spread (max - min) / median.  Clocks as found.
Before timing, both sides' results are compared at the timed size: torch's reduction sums in another order, so the
largest difference of sse (absolute, and relative to the largest sse) is reported, not asserted to be zero; the counts
must be equal.
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

#         M, grid side (K = side ** 2), image (H, W), sensor (s0, s1, C), hypotheses
SHAPES = {"a": (65536, 16, (28, 28), (5, 5, 1), "grid"),
          "b": (32768, 32, (64, 64), (12, 12, 3), "grid"),
          "c": (32768, 32, (64, 64), (12, 12, 3), "near")}
QUICK = {"a": 512, "b": 64, "c": 64}
CHUNK_ELEMS = 16 * 1024 * 1024
CHILD_SECONDS = 420
GAIN, TAU = 12.5, 0.01  # sigma = 0.2


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


def torch_chain(g, q, G, h, lim, scale, logw, gain, tau, sse, count, logw_out, sets):
    """The definition composed from torch ops, `sets` sets at a time, into sse / count / logw_out."""
    import torch

    m, s0, s1, c = g.shape
    dev = g.device
    ar, br = torch.arange(s0, device=dev), torch.arange(s1, device=dev)
    for lo in range(0, m, sets):
        hi = min(m, lo + sets)
        hh = (h if h.dim() == 2 else h[lo:hi]).double()
        qq = q[lo:hi].double()[:, None, :]
        d = (qq - hh) * lim / scale
        dy, dx = d[..., 1], d[..., 0]
        ok = torch.isfinite(d).all(-1) & (dy.abs() < s0) & (dx.abs() < s1)
        dy, dx = torch.where(ok, dy, 0.0), torch.where(ok, dx, 0.0)
        iy, ix = dy.floor(), dx.floor()
        fy, fx = (dy - iy).float()[..., None, None, None], (dx - ix).float()[..., None, None, None]
        ay, bx = ar + dy[..., None], br + dx[..., None]
        in_a = (ay >= 0) & (ay <= s0 - 1) & ok[..., None]
        in_b = (bx >= 0) & (bx <= s1 - 1) & ok[..., None]
        r0 = (ar + iy.long()[..., None]).clamp(0, s0 - 1)[:, :, :, None]
        c0 = (br + ix.long()[..., None]).clamp(0, s1 - 1)[:, :, None, :]
        r1, c1 = (r0 + 1).clamp(max=s0 - 1), (c0 + 1).clamp(max=s1 - 1)
        Gm, mi = G[lo:hi], torch.arange(hi - lo, device=dev)[:, None, None, None]
        top = Gm[mi, r0, c0] * (1 - fx) + Gm[mi, r0, c1] * fx
        bot = Gm[mi, r1, c0] * (1 - fx) + Gm[mi, r1, c1] * fx
        diff = g[lo:hi, None] - (top * (1 - fy) + bot * fy)
        e = torch.where((in_a[:, :, :, None] & in_b[:, :, None, :])[..., None], diff * diff, 0.0)
        torch.sum(e, (-3, -2, -1), out=sse[lo:hi])
        count[lo:hi] = c * in_a.sum(-1) * in_b.sum(-1)
        logw_out[lo:hi] = logw[lo:hi] + gain * (tau * count[lo:hi].float() - sse[lo:hi])


def child(args) -> int:
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        print("bench_overlap_scores: needs a GPU (nothing is measured without one)", file=sys.stderr)
        return 2
    import ap_gym_amd as ap
    from ap_gym_amd.image_env import sensor_pos_lim_pixels

    m, side, image, (s0, s1, c), how = SHAPES[args.shape]
    if args.quick:
        m = QUICK[args.shape]
    k, L = side * side, s0 * s1 * c
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    g = torch.rand((m, s0, s1, c), dtype=torch.float32, device=dev, generator=gen)
    G = torch.rand((m, s0, s1, c), dtype=torch.float32, device=dev, generator=gen)
    q = torch.rand((m, 2), dtype=torch.float32, device=dev, generator=gen) * 2 - 1
    lim = sensor_pos_lim_pixels(image, (s0, s1), 1.0)
    if how == "grid":
        t = np.linspace(-1, 1, side).astype(np.float32)
        h = torch.as_tensor(np.stack(np.meshgrid(t, t, indexing="xy"), -1).reshape(k, 2), device=dev)
    else:  # within one sensor width of q: every hypothesis overlaps
        reach = torch.as_tensor(np.array([s1, s0]) / lim * 0.999, dtype=torch.float32, device=dev)
        h = q[:, None, :] + (torch.rand((m, k, 2), dtype=torch.float32, device=dev, generator=gen) * 2 - 1) * reach
    logw = torch.randn((m, k), dtype=torch.float32, device=dev, generator=gen)
    geo = dict(image_size=image, sensor_size=(s0, s1))
    out = torch.empty((m, k), dtype=torch.float32, device=dev)
    p_sse, p_lw = torch.empty_like(out), torch.empty_like(out)
    p_count = torch.empty((m, k), dtype=torch.int32, device=dev)
    lim_t = torch.as_tensor(lim, dtype=torch.float64, device=dev)
    sets = max(1, CHUNK_ELEMS // (k * L))
    last = {}

    def new():
        last["res"] = ap.image_overlap_scores(g, q, G, h, logw=logw, gain=GAIN, tau=TAU, logw_out=out, **geo)

    def parent():
        torch_chain(g, q, G, h, lim_t, 1.0, logw, GAIN, TAU, p_sse, p_count, p_lw, sets)

    for fn in (new, parent):  # warm up both sides at the timed shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = {"M": m, "K": k, "image": list(image), "sensor": [s0, s1, c], "L": L, "hypotheses": how,
           "units": m * k, "parent_sets_per_chunk": sets}
    r = last["res"]
    res["overlapping_fraction"] = float((r.count > 0).float().mean())
    res["counts_equal"] = bool(torch.equal(r.count, p_count))
    res["sse_max_abs_diff_to_torch"] = float((r.sse - p_sse).abs().max())
    res["sse_max"] = float(r.sse.max())
    res["logw_max_abs_diff_to_torch"] = float((r.logw - p_lw).abs().max())
    if not res["counts_equal"]:
        print(json.dumps(res))
        return 1
    runs = {"new": [], "parent": []}
    for run in range(args.runs):  # alternate inside a run, either side first in turn
        for name, fn in (("new", new), ("parent", parent))[::-1 if run % 2 else 1]:
            runs[name].append(time_launches(fn, args.launches))
    res["new_us"], res["parent_us"] = summary(runs["new"]), summary(runs["parent"])
    res["parent_over_new"] = res["parent_us"]["median"] / res["new_us"]["median"]
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
    result = {"tool": "tools/bench_overlap_scores.py", "runs": args.runs, "launches": args.launches,
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
