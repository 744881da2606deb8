#!/usr/bin/env python3
"""Time UNet(dim=32) forwards at 256x256, batch 16: the HIP model (uf_unet_fwd) in bf16 / f16 / f32 against PyTorch eager on the same
GPU (channels_last, autocast for the 2-byte types), each output's max |delta| against the fp32 restatement (tests/unet_composition.py).

    python scripts/time_unet.py [--out profiles/unet_fwd.json] [--steps 20]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from unet_composition import unet_forward  # noqa: E402
from uformer_amd import model, spec  # noqa: E402


def timed(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "unet_fwd.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    B, S, dim = args.batch, args.size, 32
    sd = spec.synth_unet_state_dict(dim, 1234)
    sdc = {k: v.cuda() for k, v in sd.items()}
    x = spec.synth_input(B, S, S, 1234).cuda()
    res = {"arch": "UNet", "dim": dim, "batch": B, "H": S, "W": S, "gpu": torch.cuda.get_device_name(0), "rows": []}
    with torch.no_grad():
        ref = unet_forward(x, sdc)
        xcl = x.contiguous(memory_format=torch.channels_last)
        sdcl = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sdc.items()}
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            m = model.UNet(dim=dim, compute_dtype=dt).eval()
            m.load_state_dict(sd, strict=True)
            m = m.cuda()
            y = m(x)
            ms = timed(lambda: m(x), args.steps)
            if dt == torch.float32:
                ye = unet_forward(xcl, sdcl)
                ms_e = timed(lambda: unet_forward(xcl, sdcl), args.steps)
            else:
                with torch.autocast("cuda", dtype=dt):
                    ye = unet_forward(xcl, sdcl).float()
                    ms_e = timed(lambda: unet_forward(xcl, sdcl), args.steps)
            row = {"dtype": str(dt).replace("torch.", ""), "hip_ms": ms, "hip_img_s": B * 1000.0 / ms,
                   "eager_ms": ms_e, "eager_img_s": B * 1000.0 / ms_e, "hip_vs_eager": ms_e / ms,
                   "hip_maxabs_vs_f32_restatement": (y - ref).abs().max().item(),
                   "eager_maxabs_vs_f32_restatement": (ye.float() - ref).abs().max().item()}
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
            del m
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
