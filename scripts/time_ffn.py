#!/usr/bin/env python3
"""Time the fused Mlp feed-forward kernel (uf_ffn_fwd) against the unfused composition of existing entry points on the same build
(uf_ln_linear_gelu_fwd writing h to HBM, then uf_linear_residual_fwd), per block width at the token counts of Uformer-B 256x256 batch 16,
and the whole ``token_mlp='ffn'`` Uformer-B forward.  HIP-event timing; the two versions alternate inside one process and every figure is
kept per repeat, so the run-to-run spread is in the file next to the difference it qualifies.

    python scripts/time_ffn.py [--out profiles/ffn_fwd.json] [--steps 20] [--repeats 3]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ffn_fwd.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    B, S = args.batch, args.size
    lib = _lib.load()
    cfg = dataclasses.replace(spec.arch_config("Uformer_B", img_size=S), token_mlp="ffn")
    shapes = sorted({(c, (S // d)) for c, d in zip(cfg.stage_dims(), cfg.stage_res_div())})        # (width, map side) of the nine stages
    res = {"arch": "Uformer_B", "token_mlp": "ffn", "batch": B, "H": S, "W": S, "gpu": torch.cuda.get_device_name(0), "steps": args.steps,
           "repeats": args.repeats, "kernel_rows": [], "model_rows": []}
    st = lambda: torch.cuda.current_stream().cuda_stream                     # noqa: E731
    g = torch.Generator().manual_seed(1)
    for dt in (torch.bfloat16, torch.float16):
        udt = ops.uf_dtype(dt)
        for C, side in shapes:
            M = B * side * side
            x = (torch.randn(M, C, generator=g) * 1.5).cuda()
            gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
            w1 = (torch.randn(4 * C, C, generator=g) / C ** 0.5).cuda().to(dt)
            w2 = (torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5).cuda().to(dt)
            b1, b2 = torch.zeros(4 * C).cuda(), torch.zeros(C).cuda()
            w1_fm, w2_fm = packing.pack_frag(w1, dt), packing.pack_frag(w2, dt)
            h = torch.empty(M, 4 * C, dtype=dt, device="cuda")
            xf, xu = x.clone(), x.clone()

            def fused():
                _lib.check(lib.uf_ffn_fwd(xf.data_ptr(), C, gamma.data_ptr(), beta.data_ptr(), w1_fm.data_ptr(), b1.data_ptr(), w2_fm.data_ptr(),
                                          b2.data_ptr(), None, B, M, C, udt, st()), "uf_ffn_fwd")

            def unfused():
                _lib.check(lib.uf_ln_linear_gelu_fwd(xu.data_ptr(), C, gamma.data_ptr(), beta.data_ptr(), w1_fm.data_ptr(), b1.data_ptr(), h.data_ptr(),
                                                     M, 4 * C, C, udt, st()), "uf_ln_linear_gelu_fwd")
                _lib.check(lib.uf_linear_residual_fwd(h.data_ptr(), w2.data_ptr(), b2.data_ptr(), xu.data_ptr(), xu.data_ptr(), None, B, side, side,
                                                      C, 4 * C, 0, 0, udt, st()), "uf_linear_residual_fwd")

            tf, tu = [], []
            for _ in range(args.repeats):                                    # alternate the two versions
                tf.append(timed(fused, args.steps))
                tu.append(timed(unfused, args.steps))
            mf, mu = statistics.median(tf), statistics.median(tu)
            flops = 16.0 * M * C * C
            row = {"dtype": str(dt).replace("torch.", ""), "C": C, "M": M, "fused_ms": tf, "unfused_ms": tu, "fused_ms_median": mf,
                   "unfused_ms_median": mu, "fused_spread": (max(tf) - min(tf)) / mf, "unfused_spread": (max(tu) - min(tu)) / mu,
                   "unfused_over_fused": mu / mf, "fused_tflops": flops / mf / 1e9, "route": "fused"}
            print(json.dumps(row), flush=True)
            res["kernel_rows"].append(row)
            del x, xf, xu, h
    if not args.no_model:
        sd = spec.synth_state_dict(cfg, 1234)
        xin = spec.synth_input(B, S, S, 1234).cuda()
        with torch.no_grad():
            for dt in (torch.bfloat16, torch.float16):
                m = model.Uformer(img_size=S, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), modulator=True,
                                  dd_in=cfg.dd_in, token_mlp="ffn", compute_dtype=dt).eval()
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
