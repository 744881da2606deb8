#!/usr/bin/env python3
"""Fixtures of the models built for 64x64 patches (img_size 64: the bottleneck runs on 4x4 windows), FROM THE REFERENCE ITSELF.

Runs only in the build container (needs the reference checkout), on the pattern of make_golden.py, whose 3-symbol timm shim and
helpers it reuses:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_win4.py

Writes
  * win4_spec.json            the reference's (key, shape) state_dict layout of Uformer_B and Uformer_T at img_size 64, and the
                              (16, 16) relative_position_index of a 4x4-window block;
  * model_win4_<tag>.npz      forward outputs on spec.synth_input (the tests regenerate the inputs, they are not stored);
  * grad_model_tiny32_64.npz  Charbonnier loss, d loss / d x and every parameter gradient as probes (tests/gradproj.py): norms,
                              two signed projections, a seeded 256-element gather or the full tensor (both bottleneck
                              relative-position tables in full) and a few 64x64 blocks.  Its forward output is model_win4_tiny32_64's.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

import make_golden as mg  # noqa: E402  (installs the timm shim and imports the reference's model.py as mg.ref)
from gradproj import gather_index, proj_vector  # noqa: E402
from uformer_amd import spec  # noqa: E402

ref = mg.ref
FULL = ("conv.blocks.0.attn.relative_position_bias_table", "conv.blocks.1.attn.relative_position_bias_table",
        "decoderlayer_0.blocks.0.attn.relative_position_bias_table", "input_proj.proj.0.weight", "output_proj.proj.0.bias")
BLOCK64 = ("conv.blocks.0.attn.qkv.to_kv.weight", "conv.blocks.1.mlp.linear2.0.weight", "dowsample_3.conv.0.weight", "upsample_0.deconv.0.weight")
N_GATHER = 256


def ref_model(cfg):
    m = ref.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                    win_size=8, token_projection="linear", token_mlp="leff", modulator=cfg.modulator, dd_in=cfg.dd_in).eval()
    assert list(m.state_dict().keys()) == [k for k, _, _ in spec.state_dict_spec(cfg)], "state_dict key order/layout drifted"
    return m


def main():
    torch.set_num_threads(8)
    # ---------------- state_dict layout + the 4x4 index --------------------------------------------------
    layout = {}
    for arch in ("Uformer_B", "Uformer_T"):
        m = ref_model(spec.arch_config(arch, img_size=64))
        layout[arch] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    blk = m.conv.blocks[0]
    path = os.path.join(HERE, "win4_spec.json")
    with open(path, "w") as f:
        json.dump({"img_size": 64, "state_dict": layout, "relative_position_index_4": blk.attn.relative_position_index.tolist(),
                   "conv_win_size": blk.win_size, "conv_shift_size": blk.shift_size}, f)
    print(f"win4_spec.json  {os.path.getsize(path) / 1024:.0f} KiB")

    # ---------------- forward outputs --------------------------------------------------------------------
    def run_model(tag, arch, B, H, W, seed=1234, in_seed=1234):
        cfg = spec.arch_config(arch, img_size=64)
        sd = spec.synth_state_dict(cfg, seed)
        m = ref_model(cfg)
        m.load_state_dict(sd, strict=True)
        x = spec.synth_input(B, H, W, in_seed)
        with torch.no_grad():
            y = m(x)
        mg.save("model_win4_" + tag, y=y, arch=arch, img_size=64, B=B, H=H, W=W, seed=seed, in_seed=in_seed, sd_sha256=mg.sd_digest(sd))

    run_model("B_64", "Uformer_B", 2, 64, 64)
    run_model("B_256", "Uformer_B", 1, 256, 256)          # train_denoise.py's validation shape: a 16x16 bottleneck of sixteen windows
    run_model("tiny_64", "tiny", 2, 64, 64)
    run_model("tiny32_64", "tiny32", 2, 64, 64)

    # ---------------- gradients of tiny32 (eval(): DropPath is the identity) --------------------------------
    import losses as ref_losses  # noqa: E402  (the reference's losses.py)
    cfg = spec.arch_config("tiny32", img_size=64)
    sd = spec.synth_state_dict(cfg, 1234)
    m = ref_model(cfg)
    m.load_state_dict(sd, strict=True)
    x = spec.synth_input(2, 64, 64, 1234).requires_grad_(True)
    target = spec.synth_input(2, 64, 64, 1235)
    y = m(x)
    loss = ref_losses.CharbonnierLoss()(y, target)
    loss.backward()
    names, norms, proj, probes = [], [], [], {}
    for n, p_ in m.named_parameters():
        gr = p_.grad.detach()
        names.append(n)
        norms.append([float(gr.double().norm()), float(gr.abs().max())])
        proj.append([float((gr.double() * proj_vector(n, k, gr.shape).double()).sum()) for k in range(2)])
        if n in FULL or gr.numel() <= N_GATHER:
            probes["full." + n] = gr
        else:
            probes["gather." + n] = gr.reshape(-1)[gather_index(n, gr.numel(), N_GATHER)]
        if n in BLOCK64:
            probes["block64." + n] = gr.reshape(gr.shape[0], -1)[:64, :64]
    mg.save("grad_model_tiny32_64", loss=loss.detach(), dx=x.grad, param_names=np.array(names),
            norms=np.array(norms), proj=np.array(proj), **probes)
    print("loss %.6f  params %d" % (float(loss), len(names)))


if __name__ == "__main__":
    main()
