#!/usr/bin/env python
"""Measure the packed-bit map observation (map_obs="bits") and the device unpack kernel on one GPU.

    python tools/bench_map_bits.py [--runs 3] [--launches 20] [--out profiles/map_bits.json]

Prints one JSON line.  The driver itself never touches the GPU: every section runs in a child process of its own
under `timeout -k 10 <seconds>`, and the first section that fails (or times out) ends the run.

  kernel     k_unpack_maps against a device-to-device Tensor.copy_ of the same output size in the same process
             (the copy moves twice the bytes: it also reads them), float32 / bfloat16 / uint8 output at
             N = 65 536 maps of 64 x 64, a 4 096-id random gather, and 127 x 127 at N = 262 144
  env_torch  the cfg-2 env (LIDARLocRooms-v0, N = 65 536, 64 x 64, 32 beams), map_obs="bits" against "dense" in the
             same run, alternating: ordinary step and autoreset step (device events around env.step), whole-episode
             env-steps/s (host clock around synchronised work), torch.cuda.memory_allocated after construction
  env_torch_bits_first  the same with the bits env constructed before the dense one (env_torch: dense first), so the
             two envs' buffers swap places in the allocator: does a difference follow the mode or the addresses?
  env_numpy  the same env with the numpy backend and copy=True: env-steps/s, bits against dense

Every timing is the median of `--launches` launches (the autoreset step: one per 101-step episode, so `--launches`
episodes), taken `--runs` times; the runs' medians are all reported, with their spread (max - min) / median.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "active-perception-gym_amd"))

SECTIONS = {"kernel": 420, "env_torch": 420, "env_torch_bits_first": 420, "env_numpy": 420}  # seconds per child
EPISODE = 101  # TimeLimit(100) + the autoreset step
HBM_COPY_TBS = 6.3  # the achievable HBM rate the microarchitecture notes give for a streaming copy


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


def section_kernel(args) -> dict:
    import torch

    import ap_gym_amd as ap

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}

    def case(name, n, size, dtype, ids=None, with_copy=False):
        bits = torch.randint(-2**63, 2**63 - 1, (n, size, (size + 63) // 64), dtype=torch.int64, device=dev,
                             generator=g)
        m = n if ids is None else len(ids)
        dst = torch.empty((m, size, size, 1), dtype=dtype, device=dev)
        src = torch.zeros_like(dst) if with_copy else None
        fns = {"unpack": lambda: ap.unpack_map_bits(bits, size, ids, out=dst)}
        if with_copy:
            fns["copy"] = lambda: dst.copy_(src)
        for fn in fns.values():  # warm up every shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in fns}
        for _ in range(args.runs):  # alternate inside a run
            for k, fn in fns.items():
                runs[k].append(time_launches(fn, args.launches))
        nbytes = dst.numel() * dst.element_size()
        r = {"maps": m, "map": f"{size}x{size}", "dtype": str(dtype).split(".")[1], "bytes_out": nbytes,
             "bytes_in": m * size * ((size + 63) // 64) * 8, "unpack_us": summary(runs["unpack"])}
        r["write_TBps"] = nbytes / (r["unpack_us"]["median"] * 1e-6) / 1e12
        r["share_of_copy_rate"] = r["write_TBps"] / HBM_COPY_TBS
        if with_copy:
            r["copy_us"] = summary(runs["copy"])
            r["copy_TBps_read_plus_write"] = 2 * nbytes / (r["copy_us"]["median"] * 1e-6) / 1e12
            r["unpack_over_copy"] = r["unpack_us"]["median"] / r["copy_us"]["median"]
        out[name] = r
        del bits, dst, src
        torch.cuda.empty_cache()

    n, big = (65536, 262144) if not args.quick else (512, 256)
    case("f32_64x64", n, 64, torch.float32, with_copy=True)
    case("bf16_64x64", n, 64, torch.bfloat16)
    case("f16_64x64", n, 64, torch.float16)
    case("u8_64x64", n, 64, torch.uint8)
    ids = torch.randint(0, n, (4096 if not args.quick else 64,), device=dev, generator=g)
    case("f32_64x64_gather4096", n, 64, torch.float32, ids=ids)
    case("f32_127x127", big, 127, torch.float32)
    case("bf16_127x127", big, 127, torch.bfloat16)
    return out


def make_env(args, backend: str, map_obs: str, **kw):
    import ap_gym_amd as ap

    n = 65536 if not args.quick else 1024
    return ap.make_vec("LIDARLocRooms-v0", num_envs=n, lidar_beam_count=32, dataset=ap.FloorMapDatasetRooms(64, 64),
                       device="cuda:0", array_backend=backend, map_obs=map_obs, **kw)


def section_env_torch(args, order=("dense", "bits")) -> dict:
    import torch

    dev = torch.device("cuda:0")
    out = {"constructed_in_order": list(order), "memory_allocated_after_construction": {}}
    envs = {}
    for mode in order:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        envs[mode] = make_env(args, "torch", mode)
        out["memory_allocated_after_construction"][mode] = torch.cuda.memory_allocated(dev) - before
    m = out["memory_allocated_after_construction"]
    n = envs["bits"].num_envs
    m["dense_minus_bits"] = m["dense"] - m["bits"]
    m["N*H*W*4"] = n * 64 * 64 * 4
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.rand((n, 2), device=dev, generator=g) * 2 - 1
    p = torch.rand((n, 2), device=dev, generator=g) * 2 - 1
    act = {"action": a, "prediction": p}
    for env in envs.values():  # warm-up: a whole episode, its autoreset step included
        env.reset(seed=0)
        for _ in range(EPISODE):
            env.step(act)
    torch.cuda.synchronize()
    res = {mode: {"ordinary_us": [], "reset_us": [], "env_steps_per_s": []} for mode in envs}
    for run in range(args.runs):
        for mode, env in list(envs.items())[::-1 if run % 2 else 1]:  # alternate the modes, either one first in turn
            env.reset(seed=1)
            steps = EPISODE * args.launches
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for b, e in ev:
                b.record()
                env.step(act)
                e.record()
            torch.cuda.synchronize()
            us = [b.elapsed_time(e) * 1e3 for b, e in ev]
            res[mode]["reset_us"].append(statistics.median(us[EPISODE - 1::EPISODE]))
            res[mode]["ordinary_us"].append(statistics.median(u for t, u in enumerate(us) if (t + 1) % EPISODE))
            env.reset(seed=2)  # whole episodes on the host clock, no events
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(EPISODE * 5):
                env.step(act)
            torch.cuda.synchronize()
            res[mode]["env_steps_per_s"].append(n * EPISODE * 5 / (time.perf_counter() - t0))
            env.check_errors()
    for mode in envs:
        out[mode] = {k: summary(v) for k, v in res[mode].items()}
    out["reset_step_dense_over_bits"] = out["dense"]["reset_us"]["median"] / out["bits"]["reset_us"]["median"]
    out["num_envs"] = n
    return out


def section_env_numpy(args) -> dict:
    import numpy as np

    out = {}
    envs = {mode: make_env(args, "numpy", mode, copy=True) for mode in ("dense", "bits")}
    n = envs["bits"].num_envs
    rng = np.random.default_rng(0)
    act = {"action": rng.uniform(-1, 1, (n, 2)).astype(np.float32),
           "prediction": rng.uniform(-1, 1, (n, 2)).astype(np.float32)}
    for env in envs.values():
        env.reset(seed=0)
        for _ in range(EPISODE):
            env.step(act)
    res = {mode: [] for mode in envs}
    for run in range(args.runs):
        for mode, env in list(envs.items())[::-1 if run % 2 else 1]:
            env.reset(seed=1)
            t0 = time.perf_counter()
            for _ in range(EPISODE):
                env.step(act)  # (the numpy backend synchronises in every step)
            res[mode].append(n * EPISODE / (time.perf_counter() - t0))
    for mode in envs:
        out[mode] = {"env_steps_per_s": summary(res[mode])}
    out["bits_over_dense"] = out["bits"]["env_steps_per_s"]["median"] / out["dense"]["env_steps_per_s"]["median"]
    out["num_envs"] = n
    return out


def child(args) -> int:
    import torch

    if not torch.cuda.is_available():
        print("bench_map_bits: needs a GPU (nothing is measured without one)", file=sys.stderr)
        return 2
    res = {"kernel": section_kernel, "env_torch": section_env_torch,
           "env_torch_bits_first": lambda a: section_env_torch(a, ("bits", "dense")),
           "env_numpy": section_env_numpy}[args.section](args)
    print(json.dumps(res))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)  # the child's section
    ap.add_argument("--out", default=None, help="also write the result (indented) to this file")
    args = ap.parse_args()
    if args.section:
        return child(args)
    result = {"tool": "tools/bench_map_bits.py", "runs": args.runs, "launches": args.launches, "quick": args.quick,
              "hbm_copy_TBps_reference": HBM_COPY_TBS}
    rc = 0
    for name in args.sections.split(","):
        cmd = ["timeout", "-k", "10", str(SECTIONS[name]), sys.executable, os.path.abspath(__file__), "--section", name,
               "--runs", str(args.runs), "--launches", str(args.launches)] + (["--quick"] if args.quick else [])
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if proc.returncode != 0:  # a failed or timed-out section ends the run: nothing more starts on the GPU
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
