#!/usr/bin/env python3
"""Fixtures of ``cross_modulator=True`` models (the reference's cross_modulator / cross_attn / norm_cross in every decoder block, model.py:873-877,
:945-949, :1196-1245), FROM THE REFERENCE ITSELF.

Runs only where the reference checkout is (on the pattern of make_golden_convproj.py; reuses make_golden.py's 3-symbol timm shim and helpers and
runs the reference's ``model.py`` unmodified):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_crossmod.py

Weights of the whole-model fixtures come from spec.synth_state_dict and inputs from spec.synth_input; neither is stored.  Writes
  * crossmod_spec.json                 the reference's (key, shape) state_dict layout and parameter count of tiny32 with cross_modulator=True at
                                       img_size 128, its ``flops()`` and the two terms by which the reference's count differs from this project's
                                       exact count (LayerNorm channels -- norm_cross among them, which the reference counts and whose output it
                                       discards, model.py:995-996 -- and the 4x over-count of Upsample, model.py:776);
  * crossmod_lewin_block_a.npz         LeWinTransformerBlock(32, (16, 16), 1 head, shift 4, modulator, cross_modulator): x, weights, y;
  * crossmod_lewin_block_b.npz         LeWinTransformerBlock(64, (16, 16), 4 heads (head_dim 16), shift 0, cross_modulator): x, weights, y;
  * crossmod_model_tiny32_128.npz      the reference's forward of tiny32 / cross_modulator built at img_size 128 on a 2x3x128x128 input;
  * crossmod_model_tiny32_128x256.npz  the same weights on a 1x3x128x256 input.  The reference is square-only (model.py:910-911), so this one
                                       comes from tests/crossmod_composition.py, which this script first pins to the reference's own output
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
import crossmod_composition as XC  # noqa: E402
from uformer_amd import spec  # noqa: E402

ref = mg.ref


def quiet(fn):
    """The reference's flops() prints per module."""
    devnull = open(os.devnull, "w")
    stdout, sys.stdout = sys.stdout, devnull
    try:
        return fn()
    finally:
        sys.stdout = stdout


def main():
    torch.set_num_threads(8)
    cfg = dataclasses.replace(spec.arch_config("tiny32", img_size=128), cross_modulator=True)
    kw = dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), win_size=8,
              token_projection="linear", token_mlp="leff", modulator=cfg.modulator, cross_modulator=True, dd_in=cfg.dd_in)
    m = ref.Uformer(**kw).eval()
    assert list(m.state_dict().keys()) == [k for k, _, _ in spec.state_dict_spec(cfg)], "state_dict key order/layout drifted"

    # ---------------- layout, parameter count and flops -----------------------------------------------------------
    ref_flops = float(quiet(m.flops))
    dims, div = cfg.stage_dims(), cfg.stage_res_div()
    ln_term = sum(cfg.depths[s] * (3 if cfg.stage_has_cross_modulator(s) else 2) * dims[s] * (cfg.img_size // div[s]) ** 2
                  for s in range(9))          # norm1 + norm2 (+ norm_cross) channels, model.py:995-1004
    up_term = sum(3 * (cfg.img_size // div[4 + k]) ** 2 * 4 * cin * cout for k, (cin, cout) in enumerate(cfg.upsample_io()))   # model.py:776 counts H*2*W*2*Cin*Cout*2*2
    with open(os.path.join(HERE, "crossmod_spec.json"), "w") as f:
        json.dump({"arch": "tiny32", "cross_modulator": True, "img_size": 128, "embed_dim": cfg.embed_dim, "depths": list(cfg.depths),
                   "num_heads": list(cfg.num_heads), "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                   "n_parameters": int(sum(p_.numel() for p_ in m.parameters())), "flops": ref_flops,
                   "flops_layernorm_term": float(ln_term), "flops_upsample_overcount": float(up_term)}, f)
    print(f"crossmod_spec.json  reference flops {ref_flops:.0f}  (LayerNorm term {ln_term}, Upsample over-count {up_term})")

    # ---------------- single blocks -----------------------------------------------------------------------------------
    with torch.no_grad():
        blk = ref.LeWinTransformerBlock(32, (16, 16), 1, win_size=8, shift_size=4, modulator=True, cross_modulator=True).eval()
        mg.randomize_(blk, 501)
        x = torch.randn(2, 256, 32, generator=mg.g(502))
        mg.save("crossmod_lewin_block_a", C=32, heads=1, shift=4, x=x, y=blk(x), **{"p." + k: v for k, v in blk.state_dict().items()})
        blk = ref.LeWinTransformerBlock(64, (16, 16), 4, win_size=8, shift_size=0, cross_modulator=True).eval()
        mg.randomize_(blk, 511)
        x = torch.randn(2, 256, 64, generator=mg.g(512))
        mg.save("crossmod_lewin_block_b", C=64, heads=4, shift=0, x=x, y=blk(x), **{"p." + k: v for k, v in blk.state_dict().items()})

    # ---------------- whole model -------------------------------------------------------------------------------------
    sd = spec.synth_state_dict(cfg, 1234)
    m.load_state_dict(sd, strict=True)
    ckw = dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in)
    with torch.no_grad():
        x = spec.synth_input(2, 128, 128, 1234)
        y = m(x)
        mg.save("crossmod_model_tiny32_128", y=y, arch="tiny32", cross_modulator=True, img_size=128, B=2, H=128, W=128, seed=1234, in_seed=1234,
                sd_sha256=mg.sd_digest(sd))
        pin = (XC.uformer_forward(x, sd, **ckw) - y).abs().max().item()
        print(f"crossmod_composition vs the reference at 128x128: max |diff| = {pin:.3e}")
        assert pin < 2e-5
        xr = spec.synth_input(1, 128, 256, 1236)
        mg.save("crossmod_model_tiny32_128x256", y=XC.uformer_forward(xr, sd, **ckw), arch="tiny32", cross_modulator=True, img_size=128, B=1, H=128,
                W=256, seed=1234, in_seed=1236, sd_sha256=mg.sd_digest(sd), pinned_to_reference_at_128=pin)


if __name__ == "__main__":
    main()
