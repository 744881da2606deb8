#!/usr/bin/env python3
"""What the geometric self-ensemble costs, Uformer-B bf16 (synthetic weights, constructor 256 as bench.py's p720 mode), float32 images on the device in
and out, three ways in one process:

  (a) "aten"      the ensemble as a caller writes it around infer.restore: eight restore calls, torch.rot90 / flip either side, seven adds, a scale,
                  the clamp
  (b) "ensemble"  infer.restore_ensemble: one uf_tta_gather per parity, the members as one batch, one uf_tta_merge
  (c) "single"    one plain infer.restore

Shapes: 256x256 at B = 1, and 1280x720 on the square and on the rect canvas.  Every method restores the same image --calls times per repeat; the
repeats alternate over the methods (a b c, a b c, ...), the median of --repeats and the spread (min, max) are reported, with the speed-up (a)/(b)
and (b)/(c), the price of the ensemble in forwards.
The two kernels alone at 1280x720 on the square canvas (device events around --launches launches, alternating repeats): achieved bytes/s, and
the four-odd-member call (the transposing path) against the four-even-member call of the same size.
    timeout -k 10 900 python scripts/time_ensemble.py --out profiles/ensemble.json"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from uformer_amd import infer, model, ops, spec

SHAPES = {"256x256": dict(h=256, w=256, canvas="square", calls=20), "1280x720 square": dict(h=720, w=1280, canvas="square", calls=3),
          "1280x720 rect": dict(h=720, w=1280, canvas="rect", calls=3)}
EVEN, ODD = (0, 2, 4, 6), (1, 3, 5, 7)


def aten_ensemble(m, img, canvas):
    acc = None
    for k in range(8):
        t = torch.rot90(img, k & 3, dims=[-1, -2])
        t = t.flip(-2) if k >= 4 else t
        y = infer.restore(m, t.contiguous(), canvas=canvas, clamp=False)
        y = y.flip(-2) if k >= 4 else y
        y = torch.rot90(y, -(k & 3), dims=[-1, -2])
        acc = y if acc is None else acc + y
    return torch.clamp(acc * 0.125, 0, 1)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def time_calls(fns, calls, repeats):
    """ms per call of each fn: host clock around `calls` calls that end in a synchronise, repeats alternating over the fns"""
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return {k: stats(v) for k, v in ms.items()}


def time_launches(fns, launches, repeats):
    """ms per launch of each fn by device events, repeats alternating over the fns"""
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / launches)
    return {k: stats(v) for k, v in ms.items()}


def kernels_alone(launches, repeats):
    h, w, X, C = 720, 1280, 1280, 3
    dev = torch.device("cuda:0")
    planes = torch.rand(1, C, h, w, device=dev)
    frames = torch.randint(0, 256, (1, h, w, C), dtype=torch.uint8, device=dev)
    batch = torch.empty(4, C, X, X, dtype=torch.float32, device=dev)
    members = torch.rand(8, C, X, X, device=dev)
    out_f32 = torch.empty(1, C, h, w, dtype=torch.float32, device=dev)
    out_u8 = torch.empty(1, h, w, C, dtype=torch.uint8, device=dev)
    canvas_b, image_b = 4 * C * X * X, 4 * C * h * w                  # bytes of one f32 canvas, of one f32 image
    fns = {"gather f32 even": lambda: ops.tta_gather(planes, EVEN, X, X, out=batch), "gather f32 odd": lambda: ops.tta_gather(planes, ODD, X, X, out=batch),
           "gather u8 even": lambda: ops.tta_gather(frames, EVEN, X, X, hwc=True, out=batch), "gather u8 odd": lambda: ops.tta_gather(frames, ODD, X, X, hwc=True, out=batch),
           "merge even4 f32": lambda: ops.tta_merge(members[:4], EVEN, None, (), h, w, out=out_f32),
           "merge odd4 f32": lambda: ops.tta_merge(None, (), members[4:], ODD, h, w, out=out_f32),
           "merge 8 f32": lambda: ops.tta_merge(members[:4], EVEN, members[4:], ODD, h, w, out=out_f32),
           "merge 8 u8": lambda: ops.tta_merge(members[:4], EVEN, members[4:], ODD, h, w, u8=True, out=out_u8)}
    # bytes the algorithm needs: a gather writes its canvases and reads the image once per member; a merge reads each member's image region and writes the result
    need = {"gather f32 even": 4 * canvas_b + 4 * image_b, "gather f32 odd": 4 * canvas_b + 4 * image_b, "gather u8 even": 4 * canvas_b + image_b, "gather u8 odd": 4 * canvas_b + image_b,
            "merge even4 f32": 5 * image_b, "merge odd4 f32": 5 * image_b, "merge 8 f32": 9 * image_b, "merge 8 u8": 8 * image_b + image_b // 4}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = time_launches(fns, launches, repeats)
    rows = {k: {"ms": v, "bytes": need[k], "GB_per_s": need[k] / (v["median"] * 1e-3) / 1e9} for k, v in ms.items()}
    ratios = {}
    for a, b in (("gather f32 odd", "gather f32 even"), ("gather u8 odd", "gather u8 even"), ("merge odd4 f32", "merge even4 f32")):
        spread = max((ms[k]["max"] - ms[k]["min"]) / ms[k]["median"] for k in (a, b))
        ratios[f"{a} / {b}"] = {"ratio": ms[a]["median"] / ms[b]["median"], "run_to_run_spread": spread}
    return {"frame": "1280x720", "canvas": "1280x1280", "channels": C, "launches_per_repeat": launches, "repeats": repeats, "kernels": rows, "odd_over_even": ratios}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = spec.arch_config("Uformer_B", img_size=256)
    m = model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), modulator=cfg.modulator,
                      dd_in=cfg.dd_in, compute_dtype=torch.bfloat16)
    m.load_state_dict(spec.synth_state_dict(cfg, 1234), strict=True)
    m = m.to(dev).eval()
    res = {"workload": "Uformer_B bf16 (ctor 256), float32 image on the device -> restored float32 image, ms per call", "shapes": {}}
    with torch.no_grad():
        for name, s in SHAPES.items():
            img = spec.synth_input(1, s["h"], s["w"], 7).clamp(0, 1).to(dev)
            fns = {"aten": lambda: aten_ensemble(m, img, s["canvas"]), "ensemble": lambda: infer.restore_ensemble(m, img, canvas=s["canvas"]),
                   "single": lambda: infer.restore(m, img, canvas=s["canvas"])}
            first = {k: fn() for k, fn in fns.items()}                                   # warm-up: packing, workspaces of every batch shape; and the outputs
            diff = (first["aten"] - first["ensemble"]).abs().max().item()
            del first
            ms = time_calls(fns, s["calls"], a.repeats)
            med = {k: v["median"] for k, v in ms.items()}
            row = {"canvas": s["canvas"], "calls_per_repeat": s["calls"], "repeats": a.repeats, "ms": ms, "aten_vs_ensemble_max_abs": diff,
                   "speedup_aten_over_ensemble": med["aten"] / med["ensemble"], "ensemble_in_forwards": med["ensemble"] / med["single"],
                   "aten_in_forwards": med["aten"] / med["single"]}
            res["shapes"][name] = row
            print(json.dumps({"shape": name, "ms_median": med} | {k: v for k, v in row.items() if k not in ("ms",)}), flush=True)
        res["kernels_alone"] = kernels_alone(a.launches, a.repeats)
        print(json.dumps({"kernels_GB_per_s": {k: round(v["GB_per_s"], 1) for k, v in res["kernels_alone"]["kernels"].items()},
                          "odd_over_even": res["kernels_alone"]["odd_over_even"]}), flush=True)
    sh = res["shapes"]
    res["expectation"] = {"ensemble faster than aten at every shape": all(r["speedup_aten_over_ensemble"] > 1 for r in sh.values()),
                          "ensemble costs under 8 forwards at 256x256": sh["256x256"]["ensemble_in_forwards"] < 8}
    print(json.dumps(res["expectation"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
