#!/usr/bin/env python3
"""Uformer-B forward built for 64x64 patches (img_size 64: 4x4-window bottleneck, uf_uformer_win4_fwd) against the same
architecture built for 128 (uf_uformer_fwd) on 256x256 inputs, one process, regions interleaved r64 / r128.  Device events around
each timed region of --steps calls; the median of --regions regions is reported.
    python scripts/time_win4.py [--batch 16] [--steps 20] [--regions 7] [--dtype bf16] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from uformer_amd import model, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    dev = torch.device("cuda:0")
    x = spec.synth_input(a.batch, a.img, a.img, 1234).to(dev)
    ms = {}
    for ctor in (64, 128):
        m = model.get_arch("Uformer_B", train_ps=ctor, compute_dtype=T)
        m.load_state_dict(spec.synth_state_dict(spec.arch_config("Uformer_B", img_size=ctor), 1234), strict=True)
        ms[ctor] = m.to(dev).eval()
    times = {64: [], 128: []}
    with torch.no_grad():
        for ctor in (64, 128):                       # warm-up: packing, workspaces, code objects
            for _ in range(3):
                y = ms[ctor](x)
        torch.cuda.synchronize()
        for _ in range(a.regions):
            for ctor in (64, 128):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    y = ms[ctor](x)
                e1.record()
                e1.synchronize()
                times[ctor].append(e0.elapsed_time(e1) / a.steps)
                assert torch.isfinite(y).all()
    res = {"workload": f"Uformer_B {a.dtype} forward, {a.img}x{a.img}, batch {a.batch}", "steps": a.steps, "regions": a.regions}
    for ctor in (64, 128):
        med = statistics.median(times[ctor])
        res[f"r{ctor}"] = {"ms_per_call": med, "images_per_s": a.batch / med * 1e3, "regions_ms": times[ctor]}
    res["r64_over_r128_throughput"] = res["r64"]["images_per_s"] / res["r128"]["images_per_s"]
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "regions_ms"} if isinstance(v, dict) else v) for k, v in res.items()}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
