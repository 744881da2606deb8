#!/usr/bin/env python3
"""Time uformer_amd.infer.restore on 1280 x 720 frames with the reference's square canvas (canvas="square": 1280 x 1280) against the
per-axis canvas (canvas="rect": 768 x 1280), Uformer-B (synthetic weights, constructor 256 as bench.py's p720 mode), batch 1 and 8,
bf16 and f16.  Device events around each timed region of --steps calls; the median of --regions regions is reported per frame.
    python scripts/time_rect_canvas.py [--steps 5] [--regions 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from uformer_amd import infer, model, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = spec.arch_config("Uformer_B", img_size=256)
    sd = spec.synth_state_dict(cfg, 1234)
    res = {"workload": "Uformer_B (ctor 256), 1280x720 frames through infer.restore", "steps": a.steps, "regions": a.regions, "runs": []}
    for dname in a.dtypes.split(","):
        T = {"bf16": torch.bfloat16, "f16": torch.float16}[dname]
        m = model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                          modulator=cfg.modulator, dd_in=cfg.dd_in, compute_dtype=T)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval()
        for B in (int(b) for b in a.batches.split(",")):
            frames = spec.synth_input(B, 720, 1280, 4321).to(dev)
            row = {"dtype": dname, "batch": B}
            with torch.no_grad():
                for canvas in ("square", "rect"):
                    infer.restore(m, frames, canvas=canvas)              # warm-up: packing, workspace
                    torch.cuda.synchronize()
                    ts = []
                    for _ in range(a.regions):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.steps):
                            y = infer.restore(m, frames, canvas=canvas)
                        e1.record()
                        e1.synchronize()
                        ts.append(e0.elapsed_time(e1) / a.steps)
                    assert torch.isfinite(y).all() and tuple(y.shape) == (B, 3, 720, 1280)
                    row[canvas + "_ms_per_call"] = statistics.median(ts)
                    row[canvas + "_ms_per_frame"] = statistics.median(ts) / B
                    row[canvas + "_regions_ms"] = ts
            row["rect_over_square"] = row["rect_ms_per_call"] / row["square_ms_per_call"]
            res["runs"].append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_regions_ms")}), flush=True)
            del frames, y
        del m
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
