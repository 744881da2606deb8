#!/usr/bin/env python3
"""Frames per second, host uint8 to host uint8, of Uformer-B bf16 (synthetic weights, constructor 256 as bench.py's p720 mode) on frames that
start and end as pageable numpy arrays, three ways in one process:

  (a) "float"     the float path as a caller writes it around the existing interface, synchronous:
                  torch.from_numpy(f).cuda().permute(2,0,1)[None].float().div(255) -> infer.restore(canvas="rect") / infer.restore_tiled ->
                  .mul(255).round().byte().permute(1,2,0).cpu()
  (b) "frames"    infer.restore_frames on the device with plain synchronous copies either side
  (c) "depthN"    infer.FrameRestorer (pinned buffers, copies and forward on a stream per slot), N = 1, 2, 3 frames in flight

Cases: "720p" = 1280x720 on the rect canvas; "2160p" = 3840x2160 with tile=768.  Every method restores the same --frames frames per repeat; the
repeats alternate over the methods (a b c1 c2 c3, a b c1 ...), the median of --repeats and the spread (min, max) are reported.  For (b) the parts
are timed on their own (copy in, device work, copy out; medians of the same number of frames) so that a bound can be named.
One case per invocation, so that a driver gives each its own time limit; results are merged into --out:
    timeout -k 10 300 python scripts/time_frames.py --case 720p  --out profiles/frames_u8.json
    timeout -k 10 600 python scripts/time_frames.py --case 2160p --out profiles/frames_u8.json"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from uformer_amd import infer, model, spec

CASES = {"720p": dict(h=720, w=1280, tile=None, frames=24), "2160p": dict(h=2160, w=3840, tile=768, frames=8)}


def float_path(m, f, tile):
    x = torch.from_numpy(f).cuda().permute(2, 0, 1)[None].float().div(255)
    y = infer.restore(m, x, canvas="rect") if tile is None else infer.restore_tiled(m, x, tile=tile)
    return y[0].mul(255).round().byte().permute(1, 2, 0).cpu().numpy()


def frames_path(m, f, tile):
    y = infer.restore_frames(m, torch.from_numpy(f)[None].cuda(), canvas="rect", tile=tile)
    return y.cpu().numpy()[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--frames", type=int, default=0, help="frames per repeat (default: 24 at 720p, 8 at 2160p)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    case = CASES[a.case]
    h, w, tile, n = case["h"], case["w"], case["tile"], a.frames or case["frames"]
    dev = torch.device("cuda:0")
    cfg = spec.arch_config("Uformer_B", img_size=256)
    m = model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), modulator=cfg.modulator,
                      dd_in=cfg.dd_in, compute_dtype=torch.bfloat16)
    m.load_state_dict(spec.synth_state_dict(cfg, 1234), strict=True)
    m = m.to(dev).eval()
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]          # pageable host memory
    restorers = {d: infer.FrameRestorer(m, (h, w, 3), depth=d, canvas="rect", tile=tile) for d in (1, 2, 3)}
    methods = {"float": lambda: [float_path(m, f, tile) for f in frames], "frames": lambda: [frames_path(m, f, tile) for f in frames]}
    for d, r in restorers.items():
        methods[f"depth{d}"] = (lambda r=r: list(r.map(frames)))

    with torch.no_grad():
        first = {k: fn() for k, fn in methods.items()}                                     # warm-up: packing, workspaces, pinned buffers; and the outputs
        same = {k: all(np.array_equal(x, y) for x, y in zip(first["frames"], v)) for k, v in first.items()}
        assert all(same[f"depth{d}"] for d in (1, 2, 3)), "FrameRestorer must return restore_frames' frames"
        off = max(int(np.abs(x.astype(np.int16) - y.astype(np.int16)).max()) for x, y in zip(first["frames"], first["float"]))
        del first
        fps = {k: [] for k in methods}
        for _ in range(a.repeats):
            for k, fn in methods.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                dt = time.perf_counter() - t0
                assert len(out) == n and out[-1].shape == (h, w, 3) and out[-1].dtype == np.uint8
                fps[k].append(n / dt)
        # the parts of (b), each synchronised on its own
        parts = {"copy_in_ms": [], "device_ms": [], "copy_out_ms": []}
        for f in frames:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fd = torch.from_numpy(f)[None].cuda()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            y = infer.restore_frames(m, fd, canvas="rect", tile=tile)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            y.cpu()
            t3 = time.perf_counter()
            for key, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
                parts[key].append(v * 1e3)
        float_device = []
        for f in frames:
            fd = torch.from_numpy(f).cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = fd.permute(2, 0, 1)[None].float().div(255)
            y = infer.restore(m, x, canvas="rect") if tile is None else infer.restore_tiled(m, x, tile=tile)
            q = y[0].mul(255).round().byte().permute(1, 2, 0).contiguous()
            torch.cuda.synchronize()
            float_device.append((time.perf_counter() - t0) * 1e3)
    for r in restorers.values():
        r.close()

    row = {"frame": f"{w}x{h}", "tile": tile, "canvas": "rect", "frames_per_repeat": n, "repeats": a.repeats,
           "fps": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for k, v in fps.items()},
           "frames_path_parts_ms": {k: statistics.median(v) for k, v in parts.items()}, "float_path_device_ms": statistics.median(float_device),
           "depth_equals_frames": all(same[f"depth{d}"] for d in (1, 2, 3)), "float_equals_frames": same["float"], "float_vs_frames_max_levels": off}
    med = {k: v["median"] for k, v in row["fps"].items()}
    row["expectation"] = {"frames >= float": med["frames"] >= med["float"], "best depth >= frames": max(med["depth1"], med["depth2"], med["depth3"]) >= med["frames"]}
    print(json.dumps({k: v for k, v in row.items() if k != "fps"} | {"fps_median": med}), flush=True)
    if a.out:
        res = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        res.setdefault("workload", "Uformer_B bf16 (ctor 256), host uint8 frames (pageable numpy) -> restored host uint8 frames, frames per second")
        res.setdefault("cases", {})[a.case] = row
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
