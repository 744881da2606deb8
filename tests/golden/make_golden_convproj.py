#!/usr/bin/env python3
"""Fixtures of ``token_projection='conv'`` models (the reference's ConvProjection in place of LinearProjection, model.py:480-481), FROM THE
REFERENCE ITSELF.

Runs only where the reference checkout is (on the pattern of make_golden_ffn.py; reuses make_golden.py's 3-symbol timm shim and helpers and
runs the reference's ``model.py`` unmodified):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_convproj.py

Weights of the whole-model fixtures come from spec.synth_state_dict and inputs from spec.synth_input; neither is stored.  Writes
  * convproj_spec.json                 the reference's (key, shape) state_dict layout and parameter count of tiny32 with token_projection='conv'
                                       at img_size 128, its ``flops()`` and the two terms by which the reference's count differs from this
                                       project's exact count (LayerNorm channels, the 4x over-count of Upsample, model.py:776);
  * convproj_lewin_block_a.npz         LeWinTransformerBlock(32, (16, 16), 1 head, shift 4, modulator, token_projection='conv'): x, weights, y;
  * convproj_lewin_block_b.npz         LeWinTransformerBlock(64, (16, 16), 2 heads, shift 0, token_projection='conv'): x, weights, y;
  * convproj_model_tiny32_128.npz      the reference's forward of tiny32 / 'conv' built at img_size 128 on a 2x3x128x128 input;
  * convproj_model_tiny32_128x256.npz  the same weights on a 1x3x128x256 input.  The reference is square-only (model.py:910-911), so this one
                                       comes from tests/convproj_composition.py, which this script first pins to the reference's own output
                                       at 128x128 (max |diff| printed and asserted < 2e-5).
"""
import dataclasses
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

import make_golden as mg  # noqa: E402  (installs the timm shim and imports the reference's model.py as mg.ref)
import convproj_composition as CC  # noqa: E402
from uformer_amd import spec  # noqa: E402

ref = mg.ref


def int_dilation_(module):
    """ConvProjection passes ``bias`` (True) in SepConv2d's ``dilation`` slot (model.py:390-392), so its depthwise Conv2d carries
    dilation (True, True): the torch the reference was written for read that as 1, this one rejects a bool.  Same module, same value, as ints."""
    for c in module.modules():
        if isinstance(c, torch.nn.Conv2d):
            c.dilation = tuple(int(d) for d in c.dilation)
    return module


def main():
    torch.set_num_threads(8)
    cfg = dataclasses.replace(spec.arch_config("tiny32", img_size=128), token_projection="conv")
    kw = dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), win_size=8,
              token_projection="conv", token_mlp="leff", modulator=cfg.modulator, dd_in=cfg.dd_in)
    m = int_dilation_(ref.Uformer(**kw)).eval()
    assert list(m.state_dict().keys()) == [k for k, _, _ in spec.state_dict_spec(cfg)], "state_dict key order/layout drifted"

    # ---------------- layout, parameter count and flops -----------------------------------------------------------
    devnull = open(os.devnull, "w")
    stdout, sys.stdout = sys.stdout, devnull          # the reference's flops() prints per module
    try:
        ref_flops = float(m.flops())
    finally:
        sys.stdout = stdout
    dims, div = cfg.stage_dims(), cfg.stage_res_div()
    ln_term = sum(cfg.depths[s] * 2 * dims[s] * (cfg.img_size // div[s]) ** 2 for s in range(9))          # norm1 + norm2 channels, model.py:1000-1004
    up_term = sum(3 * (cfg.img_size // div[4 + k]) ** 2 * 4 * cin * cout for k, (cin, cout) in enumerate(cfg.upsample_io()))   # model.py:776 counts H*2*W*2*Cin*Cout*2*2
    with open(os.path.join(HERE, "convproj_spec.json"), "w") as f:
        json.dump({"arch": "tiny32", "token_projection": "conv", "img_size": 128, "embed_dim": cfg.embed_dim, "depths": list(cfg.depths),
                   "num_heads": list(cfg.num_heads), "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                   "n_parameters": int(sum(p_.numel() for p_ in m.parameters())), "flops": ref_flops,
                   "flops_layernorm_term": float(ln_term), "flops_upsample_overcount": float(up_term)}, f)
    print(f"convproj_spec.json  reference flops {ref_flops:.0f}  (LayerNorm term {ln_term}, Upsample over-count {up_term})")

    # ---------------- single blocks -----------------------------------------------------------------------------------
    with torch.no_grad():
        blk = int_dilation_(ref.LeWinTransformerBlock(32, (16, 16), 1, win_size=8, shift_size=4, token_projection="conv", modulator=True)).eval()
        mg.randomize_(blk, 401)
        x = torch.randn(2, 256, 32, generator=mg.g(402))
        mg.save("convproj_lewin_block_a", C=32, heads=1, shift=4, x=x, y=blk(x), **{"p." + k: v for k, v in blk.state_dict().items()})
        blk = int_dilation_(ref.LeWinTransformerBlock(64, (16, 16), 2, win_size=8, shift_size=0, token_projection="conv")).eval()
        mg.randomize_(blk, 411)
        x = torch.randn(2, 256, 64, generator=mg.g(412))
        mg.save("convproj_lewin_block_b", C=64, heads=2, shift=0, x=x, y=blk(x), **{"p." + k: v for k, v in blk.state_dict().items()})

    # ---------------- whole model -------------------------------------------------------------------------------------
    sd = spec.synth_state_dict(cfg, 1234)
    m.load_state_dict(sd, strict=True)
    ckw = dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in)
    with torch.no_grad():
        x = spec.synth_input(2, 128, 128, 1234)
        y = m(x)
        mg.save("convproj_model_tiny32_128", y=y, arch="tiny32", token_projection="conv", img_size=128, B=2, H=128, W=128, seed=1234, in_seed=1234,
                sd_sha256=mg.sd_digest(sd))
        pin = (CC.uformer_forward(x, sd, **ckw) - y).abs().max().item()
        print(f"convproj_composition vs the reference at 128x128: max |diff| = {pin:.3e}")
        assert pin < 2e-5
        xr = spec.synth_input(1, 128, 256, 1236)
        mg.save("convproj_model_tiny32_128x256", y=CC.uformer_forward(xr, sd, **ckw), arch="tiny32", token_projection="conv", img_size=128, B=1, H=128,
                W=256, seed=1234, in_seed=1236, sd_sha256=mg.sd_digest(sd), pinned_to_reference_at_128=pin)


if __name__ == "__main__":
    main()
