#!/usr/bin/env python3
"""Time the ConvProjection producer (uf_ln_convqkv_fwd) against the LinearProjection producer (uf_ln_qkv_fwd) at the same shape -- the same
LayerNorm and the same (3C, C) GEMM without the three window stencils: the yardstick -- per block width at the token counts of Uformer-B
256x256 batch 16, in bf16, f16 and f32, and the whole ``token_projection='conv'`` Uformer-B forward.  HIP-event timing; the two kernels alternate
inside one process and every figure is kept per repeat, so the run-to-run spread is in the file next to the ratio it qualifies.

    python scripts/time_convproj.py [--out profiles/convproj_fwd.json] [--steps 20] [--repeats 3]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from uformer_amd import _lib, model, ops, packing, spec  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "convproj_fwd.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    B, S = args.batch, args.size
    lib = _lib.load()
    cfg = dataclasses.replace(spec.arch_config("Uformer_B", img_size=S), token_projection="conv")
    shapes = sorted({(c, (S // d), h) for c, d, h in zip(cfg.stage_dims(), cfg.stage_res_div(), cfg.num_heads)})   # (width, map side, heads) of the nine stages
    res = {"arch": "Uformer_B", "token_projection": "conv", "batch": B, "H": S, "W": S, "gpu": torch.cuda.get_device_name(0), "steps": args.steps,
           "repeats": args.repeats, "kernel_rows": [], "model_rows": []}
    st = lambda: torch.cuda.current_stream().cuda_stream                     # noqa: E731
    g = torch.Generator().manual_seed(1)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        udt = ops.uf_dtype(dt)
        for C, side, heads in shapes:
            M = B * side * side
            x = (torch.randn(M, C, generator=g) * 1.5).cuda()
            gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
            w_fm = packing.pack_frag((torch.randn(3 * C, C, generator=g) / C ** 0.5).cuda(), dt)
            bias = torch.zeros(3 * C).cuda()
            dw9, bdw = (0.3 * torch.randn(3, 9, C, generator=g)).cuda(), torch.zeros(3, C).cuda()
            q, k, vt = (torch.empty(M * C, dtype=dt, device="cuda") for _ in range(3))

            def conv():
                _lib.check(lib.uf_ln_convqkv_fwd(x.data_ptr(), C, gamma.data_ptr(), beta.data_ptr(), None, dw9.data_ptr(), bdw.data_ptr(), w_fm.data_ptr(),
                                                 bias.data_ptr(), q.data_ptr(), k.data_ptr(), vt.data_ptr(), B, side, side, C, heads, 0, udt, st()), "uf_ln_convqkv_fwd")

            def linear():
                _lib.check(lib.uf_ln_qkv_fwd(x.data_ptr(), C, gamma.data_ptr(), beta.data_ptr(), None, w_fm.data_ptr(), bias.data_ptr(), q.data_ptr(),
                                             k.data_ptr(), vt.data_ptr(), B, side, side, C, heads, 0, udt, st()), "uf_ln_qkv_fwd")

            tc, tl = [], []
            for _ in range(args.repeats):                                    # alternate the two kernels
                tc.append(timed(conv, args.steps))
                tl.append(timed(linear, args.steps))
            mc, ml = statistics.median(tc), statistics.median(tl)
            row = {"dtype": str(dt).replace("torch.", ""), "C": C, "M": M, "heads": heads, "conv_ms": tc, "linear_ms": tl, "conv_ms_median": mc,
                   "linear_ms_median": ml, "conv_spread": (max(tc) - min(tc)) / mc, "linear_spread": (max(tl) - min(tl)) / ml,
                   "conv_over_linear": mc / ml, "conv_tflops": (6.0 * M * C * C + 54.0 * M * C) / mc / 1e9}
            print(json.dumps(row), flush=True)
            res["kernel_rows"].append(row)
            del x, q, k, vt
    if not args.no_model:
        sd = spec.synth_state_dict(cfg, 1234)
        xin = spec.synth_input(B, S, S, 1234).cuda()
        with torch.no_grad():
            for dt in (torch.bfloat16, torch.float16):
                m = model.Uformer(img_size=S, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), modulator=True,
                                  dd_in=cfg.dd_in, token_projection="conv", compute_dtype=dt).eval()
                m.load_state_dict(sd, strict=True)
                m = m.cuda()
                ms = [timed(lambda: m(xin), args.steps) for _ in range(args.repeats)]
                row = {"dtype": str(dt).replace("torch.", ""), "forward_ms": ms, "img_s": B * 1000.0 / statistics.median(ms)}
                print(json.dumps(row), flush=True)
                res["model_rows"].append(row)
                del m
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
