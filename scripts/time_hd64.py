#!/usr/bin/env python3
"""embed_dim 64 (head_dim 64 at every stage) against PyTorch-ROCm eager on the same GPU, one process, regions interleaved.

Models: get_arch('Uformer', embed_dim=64) (depths [2] * 9) and the Uformer-B depths at embed_dim 64 built through the constructor.
Forward at --img x --img, batch --batch, in bf16 / f16 / f32: the HIP path against oracle/vendor_forward.py (f32 eager, and autocast of
the operand type).  One training step (forward + backward + AdamW, batch --train-batch) against eager autograd of the same composition
with torch.optim.AdamW.  Device events around each region of --steps calls; regions alternate ours / vendor; the median of --regions
regions is reported, every region is stored.  Also the max abs error of both 2-byte forwards against the f32 eager forward.
No target ratio lives here: the condition is that the HIP path is not slower than eager in any dtype.

    python scripts/time_hd64.py [--out profiles/hd64.json] [--only fwd|train] [--profile-step | --profile-forward]
--profile-step: run a few bf16 training steps of get_arch('Uformer', embed_dim=64) and nothing else (to be run under
`rocprofv3 --kernel-trace --stats`, on its own).
--profile-forward: five bf16 inference forwards of the same model at batch --batch and nothing else (likewise: the share of the
C = 1024 blocks' weight unpack, which only the inference path runs)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from oracle import vendor_forward as V  # noqa: E402
from uformer_amd import losses, model, optim, spec  # noqa: E402

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
ARCHS = {"Uformer_e64": (2,) * 9, "Uformer_B_depths_e64": (1, 2, 8, 8, 2, 8, 8, 2, 1)}


def region(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def interleave(fns, steps, regions, warm=2):
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(regions):
        for k, f in fns.items():
            t[k].append(region(f, steps))
    return {k: {"ms": statistics.median(v), "regions_ms": v} for k, v in t.items()}


def build(depths, T, img, train=False):
    cfg = spec.UformerConfig(img_size=img, embed_dim=64, depths=tuple(depths), modulator=True)
    m = model.Uformer(img_size=img, embed_dim=64, depths=list(depths), modulator=True, compute_dtype=T)
    sd = spec.synth_state_dict(cfg, 1234)
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    return cfg, sd, (m.train() if train else m.eval())


def kw(cfg):
    return dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in)


def time_forward(a, res):
    x = spec.synth_input(a.batch, a.img, a.img, 1234).cuda()
    for name, depths in ARCHS.items():
        out = res.setdefault("forward", {}).setdefault(name, {})
        ref = None
        for tag in ("f32", "bf16", "f16"):
            T = DT[tag]
            cfg, sd, m = build(depths, T, a.img)
            sdc = {k: v.cuda() for k, v in sd.items()}

            def ours():
                with torch.no_grad():
                    return m(x)

            def vendor():
                with torch.no_grad():
                    if T == torch.float32:
                        return V.forward(x, sdc, **kw(cfg))
                    with torch.autocast("cuda", dtype=T):
                        return V.forward(x, sdc, **kw(cfg))

            r = interleave({"hip": ours, "vendor_eager": vendor}, a.steps, a.regions)
            yo, yv = ours().float(), vendor().float()
            if ref is None:
                ref = yv                                          # f32 eager: the reference of the error pair
            rec = {"hip_ms": r["hip"]["ms"], "vendor_ms": r["vendor_eager"]["ms"], "vendor_over_hip": r["vendor_eager"]["ms"] / r["hip"]["ms"],
                   "hip_images_per_s": a.batch / r["hip"]["ms"] * 1e3, "hip_regions_ms": r["hip"]["regions_ms"], "vendor_regions_ms": r["vendor_eager"]["regions_ms"],
                   "err_hip_vs_f32_eager": (yo - ref).abs().max().item(), "err_vendor_vs_f32_eager": (yv - ref).abs().max().item()}
            out[tag] = rec
            print(name, tag, {k: v for k, v in rec.items() if not k.endswith("regions_ms")}, flush=True)
            del m, sdc
            torch.cuda.empty_cache()


def time_train(a, res):
    B = a.train_batch
    x, target = spec.synth_input(B, a.img, a.img, 11).cuda(), spec.synth_input(B, a.img, a.img, 12).cuda()
    for name, depths in ARCHS.items():
        out = res.setdefault("train_step", {}).setdefault(name, {})
        for tag in ("bf16", "f16", "f32"):
            T = DT[tag]
            torch.manual_seed(1234)
            cfg, sd, m = build(depths, T, a.img, train=True)
            opt = optim.AdamW(m.parameters(), lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
            scaler = optim.GradScaler() if T == torch.float16 else None
            crit = losses.CharbonnierLoss()

            def ours():
                opt.zero_grad(set_to_none=True)
                loss = crit(m(x), target)
                if scaler is not None:
                    scaler.scale(loss).backward()
                    scaler.step(opt)
                    scaler.update()
                else:
                    loss.backward()
                    opt.step()

            pv = {k: (v.cuda().clone().requires_grad_(True) if v.is_floating_point() else v.cuda()) for k, v in sd.items()}
            vopt = torch.optim.AdamW([v for v in pv.values() if v.requires_grad], lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
            vscaler = torch.amp.GradScaler("cuda") if T == torch.float16 else None

            def vendor():                                        # eval-mode composition (no DropPath): eager autograd does strictly less work than ours
                vopt.zero_grad(set_to_none=True)
                if T == torch.float32:
                    y = V.forward(x, pv, **kw(cfg))
                else:
                    with torch.autocast("cuda", dtype=T):
                        y = V.forward(x, pv, **kw(cfg))
                d = y.float() - target
                loss = torch.sqrt(d * d + 1e-6).mean()
                if vscaler is not None:
                    vscaler.scale(loss).backward()
                    vscaler.step(vopt)
                    vscaler.update()
                else:
                    loss.backward()
                    vopt.step()

            r = interleave({"hip": ours, "vendor_eager": vendor}, a.train_steps, a.regions, warm=1)
            rec = {"batch": B, "hip_ms": r["hip"]["ms"], "vendor_ms": r["vendor_eager"]["ms"], "vendor_over_hip": r["vendor_eager"]["ms"] / r["hip"]["ms"],
                   "hip_images_per_s": B / r["hip"]["ms"] * 1e3, "hip_regions_ms": r["hip"]["regions_ms"], "vendor_regions_ms": r["vendor_eager"]["regions_ms"]}
            out[tag] = rec
            print("train", name, tag, {k: v for k, v in rec.items() if not k.endswith("regions_ms")}, flush=True)
            del m, opt, pv, vopt
            torch.cuda.empty_cache()


def profile_step(a):
    torch.manual_seed(1234)
    cfg, sd, m = build(ARCHS["Uformer_e64"], torch.bfloat16, a.img, train=True)
    opt = optim.AdamW(m.parameters(), lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    x, target = spec.synth_input(a.train_batch, a.img, a.img, 11).cuda(), spec.synth_input(a.train_batch, a.img, a.img, 12).cuda()
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        losses.CharbonnierLoss()(m(x), target).backward()
        opt.step()
    torch.cuda.synchronize()


def profile_forward(a):
    cfg, sd, m = build(ARCHS["Uformer_e64"], torch.bfloat16, a.img)
    x = spec.synth_input(a.batch, a.img, a.img, 1234).cuda()
    with torch.no_grad():
        for _ in range(5):
            m(x)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--train-batch", type=int, default=8)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=2)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--only", default="", choices=["", "fwd", "train"])
    ap.add_argument("--profile-step", action="store_true")
    ap.add_argument("--profile-forward", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.profile_step:
        return profile_step(a)
    if a.profile_forward:
        return profile_forward(a)
    res = {"workload": f"embed_dim 64, {a.img}x{a.img}: forward batch {a.batch}, training step batch {a.train_batch}; HIP path against PyTorch-ROCm eager "
                       "(oracle/vendor_forward.py; autocast for the 2-byte types), regions interleaved in one process, medians",
           "device": torch.cuda.get_device_name(0), "steps": a.steps, "train_steps": a.train_steps, "regions": a.regions}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = {**json.load(f), **res}
    if a.only != "train":
        time_forward(a, res)
    if a.only != "fwd":
        time_train(a, res)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
