#!/usr/bin/env python3
"""Time the cross-modulator attention kernel (uf_cross_attn_fwd) against the attention half of a block (uf_lewin_attn_fwd) at the same shape -- the
new kernel runs two of that half's four C x C GEMMs and the same attention arithmetic against 64 keys, and no LayerNorm, so the expectation under
test is that it is not slower -- at the four decoder shapes of Uformer-B 256x256 batch 16, in bf16, f16 and f32, and the whole Uformer-B forward
with and without ``cross_modulator=True``.  HIP-event timing; the two kernels alternate inside one process and every figure is kept per repeat,
so the run-to-run spread is in the file next to the ratio it qualifies.

    python scripts/time_crossmod.py [--out profiles/crossmod_fwd.json] [--steps 20] [--repeats 3]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "crossmod_fwd.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    B, S = args.batch, args.size
    lib = _lib.load()
    cfg = dataclasses.replace(spec.arch_config("Uformer_B", img_size=S), cross_modulator=True)
    shapes = [(cfg.stage_dims()[s], S // cfg.stage_res_div()[s], cfg.num_heads[s]) for s in range(5, 9)]      # (width, map side, heads) of the decoder stages
    res = {"arch": "Uformer_B", "cross_modulator": True, "batch": B, "H": S, "W": S, "gpu": torch.cuda.get_device_name(0), "steps": args.steps,
           "repeats": args.repeats, "kernel_rows": [], "model_rows": []}
    st = lambda: torch.cuda.current_stream().cuda_stream                     # noqa: E731
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        udt = ops.uf_dtype(dt)
        for C, side, heads in shapes:
            M = B * side * side
            torch.manual_seed(C)
            blk = model.LeWinTransformerBlock(C, (side, side), heads, modulator=True, cross_modulator=True).cuda()
            sd = blk.state_dict()
            cp, ckeep = packing.pack_cross(sd, "", heads, dt)
            bp, bkeep = packing.pack_block(sd, "", heads, 0, dt)
            x = (torch.randn(M, C) * 0.5).cuda()
            nbytes = lib.uf_block_workspace_bytes(M, C, udt)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

            def cross():
                _lib.check(lib.uf_cross_attn_fwd(cp, x.data_ptr(), C, M, C, udt, st()), "uf_cross_attn_fwd")

            def attn():
                _lib.check(lib.uf_lewin_attn_fwd(bp, x.data_ptr(), C, B, side, side, C, None, 0, udt, ws.data_ptr(), nbytes, st()), "uf_lewin_attn_fwd")

            tc, ta = [], []
            for _ in range(args.repeats):                                    # alternate the two kernels
                tc.append(timed(cross, args.steps))
                ta.append(timed(attn, args.steps))
            mc, ma = statistics.median(tc), statistics.median(ta)
            row = {"dtype": str(dt).replace("torch.", ""), "C": C, "M": M, "heads": heads, "cross_ms": tc, "attn_ms": ta, "cross_ms_median": mc,
                   "attn_ms_median": ma, "cross_spread": (max(tc) - min(tc)) / mc, "attn_spread": (max(ta) - min(ta)) / ma,
                   "cross_over_attn": mc / ma, "cross_tflops": (4.0 * M * C * C + 256.0 * M * C) / mc / 1e9,
                   "cross_stream_gbs": 8.0 * M * C / mc / 1e6}
            print(json.dumps(row), flush=True)
            res["kernel_rows"].append(row)
            del x, ws, blk
    if not args.no_model:
        xin = spec.synth_input(B, S, S, 1234).cuda()
        with torch.no_grad():
            for dt in (torch.bfloat16, torch.float16):
                ms = {}
                models = {}
                for flag in (False, True):
                    c = dataclasses.replace(cfg, cross_modulator=flag)
                    m = model.Uformer(img_size=S, embed_dim=c.embed_dim, depths=list(c.depths), num_heads=list(c.num_heads), modulator=True,
                                      dd_in=c.dd_in, cross_modulator=flag, compute_dtype=dt).eval()
                    m.load_state_dict(spec.synth_state_dict(c, 1234), strict=True)
                    models[flag] = m.cuda()
                    ms[flag] = []
                for _ in range(args.repeats):                                # alternate the two models
                    for flag in (False, True):
                        ms[flag].append(timed(lambda: models[flag](xin), args.steps))
                row = {"dtype": str(dt).replace("torch.", ""), "plain_forward_ms": ms[False], "cross_forward_ms": ms[True],
                       "plain_img_s": B * 1000.0 / statistics.median(ms[False]), "cross_img_s": B * 1000.0 / statistics.median(ms[True])}
                print(json.dumps(row), flush=True)
                res["model_rows"].append(row)
                del models
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
