#!/usr/bin/env python3
"""Fixtures of models whose image channel counts are not 3 -> 3 (``Uformer(in_chans=..., dd_in=...)``, model.py:1100-1101, :1305: dual-pixel
pairs 6 -> 3, one raw plane 1 -> 1, packed Bayer 4 -> 4, image + map 4 -> 3), FROM THE REFERENCE ITSELF.

Runs only where the reference checkout is (on the pattern of make_golden_crossmod.py; reuses make_golden.py's 3-symbol timm shim and helpers and
runs the reference's ``model.py`` unmodified):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chans.py

Weights come from spec.synth_state_dict and inputs from spec.synth_input(..., channels=dd_in); neither is stored.  Writes
  * chans_spec.json                         per (dd_in, in_chans): the reference's (key, shape) state_dict layout of tiny32 at img_size 128, its
                                            parameter count and its ``flops()`` with the two terms by which that count differs from this project's
                                            exact count (LayerNorm channels, the 4x over-count of Upsample, model.py:776);
  * chans_model_tiny32_128_d{6x3,1x1,4x4,4x3}.npz
                                            the reference's eval forward of tiny32 on a 2 x dd_in x 128 x 128 input;
  * chans_model_tiny32_128x256_d6x3.npz     the 6 -> 3 weights on a 1 x 6 x 128 x 256 input.  The reference is square-only (model.py:910-911), so
                                            this one comes from tests/rect_composition.py, which this script first pins to the reference's own
                                            output at 128 x 128 (max |diff| printed and asserted < 2e-5);
  * chans_grad_tiny_128_d{6x3,4x4}.npz      'tiny' (embed_dim 16) in train() mode at drop_path_rate 0.3 under the reference's CharbonnierLoss, the
                                            DropPath masks it drew recorded as make_golden_grad.py records them: loss, restored images, d loss /
                                            d input (centre crop and 16 x 16 pooled map: the caller asks for it, the model needs none when
                                            dd_in != 3) and, for EVERY parameter gradient, its l2 norm, its largest magnitude and two signed random
                                            projections (tests/gradproj.py); the stem's and the head's gradients and one tensor of every other
                                            kind are stored in full.
"""
import dataclasses
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
import rect_composition as R  # noqa: E402
from gradproj import proj_vector  # noqa: E402
from uformer_amd import spec  # noqa: E402

sys.path.insert(0, mg.REF)
import losses as ref_losses  # noqa: E402  (reference losses.py: torch only)

ref = mg.ref
PAIRS = [(6, 3), (1, 1), (4, 4), (4, 3)]          # (dd_in, in_chans)
GRAD_PAIRS = [(6, 3), (4, 4)]
FULL_GRADS = ("input_proj.proj.0.weight", "input_proj.proj.0.bias", "output_proj.proj.0.weight", "output_proj.proj.0.bias",
              "encoderlayer_0.blocks.0.attn.qkv.to_q.weight", "encoderlayer_0.blocks.0.attn.relative_position_bias_table",
              "encoderlayer_0.blocks.0.norm1.weight", "encoderlayer_0.blocks.0.mlp.dwconv.0.weight", "decoderlayer_3.blocks.0.modulator.weight",
              "decoderlayer_3.blocks.0.mlp.linear2.0.weight", "dowsample_0.conv.0.weight", "upsample_3.deconv.0.weight")


def quiet(fn):
    """The reference's flops() prints per module."""
    devnull = open(os.devnull, "w")
    stdout, sys.stdout = sys.stdout, devnull
    try:
        return fn()
    finally:
        sys.stdout = stdout


def ref_model(cfg, **extra):
    return ref.Uformer(img_size=cfg.img_size, in_chans=cfg.in_chans, dd_in=cfg.dd_in, embed_dim=cfg.embed_dim, depths=list(cfg.depths),
                       num_heads=list(cfg.num_heads), win_size=8, token_projection="linear", token_mlp="leff", modulator=cfg.modulator, **extra)


def forward_fixtures():
    layouts = {}
    for dd_in, in_chans in PAIRS:
        tag = f"d{dd_in}x{in_chans}"
        cfg = dataclasses.replace(spec.arch_config("tiny32", img_size=128), dd_in=dd_in, in_chans=in_chans)
        m = ref_model(cfg).eval()
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s, _ in spec.state_dict_spec(cfg)], \
            "state_dict key order/layout drifted"
        ref_flops = float(quiet(m.flops))
        dims, div = cfg.stage_dims(), cfg.stage_res_div()
        ln_term = sum(cfg.depths[s] * 2 * dims[s] * (cfg.img_size // div[s]) ** 2 for s in range(9))        # norm1 + norm2 channels, model.py:995-1004
        up_term = sum(3 * (cfg.img_size // div[4 + k]) ** 2 * 4 * cin * cout for k, (cin, cout) in enumerate(cfg.upsample_io()))   # model.py:776
        layouts[tag] = {"dd_in": dd_in, "in_chans": in_chans, "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                        "n_parameters": int(sum(p_.numel() for p_ in m.parameters())), "flops": ref_flops,
                        "flops_layernorm_term": float(ln_term), "flops_upsample_overcount": float(up_term)}
        sd = spec.synth_state_dict(cfg, 1234)
        m.load_state_dict(sd, strict=True)
        with torch.no_grad():
            x = spec.synth_input(2, 128, 128, 1234, channels=dd_in)
            y = m(x)
            assert tuple(y.shape) == (2, in_chans, 128, 128)
            mg.save(f"chans_model_tiny32_128_{tag}", y=y, arch="tiny32", dd_in=dd_in, in_chans=in_chans, img_size=128, B=2, H=128, W=128, seed=1234,
                    in_seed=1234, sd_sha256=mg.sd_digest(sd))
            if (dd_in, in_chans) == (6, 3):
                ckw = dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in)
                pin = (R.uformer_forward(x, sd, **ckw) - y).abs().max().item()
                print(f"rect_composition vs the reference at 128x128 ({tag}): max |diff| = {pin:.3e}")
                assert pin < 2e-5
                xr = spec.synth_input(1, 128, 256, 1236, channels=dd_in)
                mg.save(f"chans_model_tiny32_128x256_{tag}", y=R.uformer_forward(xr, sd, **ckw), arch="tiny32", dd_in=dd_in, in_chans=in_chans,
                        img_size=128, B=1, H=128, W=256, seed=1234, in_seed=1236, sd_sha256=mg.sd_digest(sd), pinned_to_reference_at_128=pin)
    with open(os.path.join(HERE, "chans_spec.json"), "w") as f:
        json.dump({"arch": "tiny32", "img_size": 128, "models": layouts}, f)
    print("chans_spec.json  " + ", ".join(f"{t}: {v['n_parameters']} parameters" for t, v in layouts.items()))


def grad_fixture(dd_in, in_chans):
    import timm.models.layers as tl
    tag = f"d{dd_in}x{in_chans}"
    cfg = dataclasses.replace(spec.arch_config("tiny", img_size=128), dd_in=dd_in, in_chans=in_chans)
    sd = spec.synth_state_dict(cfg, 1234)
    masks = []
    orig_fwd = tl.DropPath.forward

    def recording_forward(self, x):
        if self.drop_prob == 0. or not self.training:
            masks.append(torch.ones(x.shape[0]))
            return x
        keep = 1 - self.drop_prob
        r = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        r.div_(keep)
        masks.append(r.reshape(-1).clone())
        return x * r

    tl.DropPath.forward = recording_forward
    torch.manual_seed(100 + dd_in)
    m = ref_model(cfg, drop_path_rate=0.3).train()
    m.load_state_dict(sd, strict=True)
    xin = spec.synth_input(2, 128, 128, 6321, channels=dd_in).requires_grad_(True)
    target = spec.synth_input(2, 128, 128, 6322, channels=in_chans)
    y = m(xin)
    loss = ref_losses.CharbonnierLoss()(y, target)
    loss.backward()
    tl.DropPath.forward = orig_fwd
    # blocks whose rate is 0 hold nn.Identity instead of DropPath (model.py:883): rows of ones, so that there are two rows for EVERY block
    full, it = [], iter(masks)
    blocks = [m_ for m_ in m.modules() if isinstance(m_, ref.LeWinTransformerBlock)]
    for blk in blocks:
        for _ in range(2):
            full.append(next(it) if isinstance(blk.drop_path, tl.DropPath) else torch.ones(xin.shape[0]))
    assert next(it, None) is None
    masks = torch.stack(full)
    rates = [float(b.drop_path.drop_prob) if isinstance(b.drop_path, tl.DropPath) else 0.0 for b in blocks]
    named = list(m.named_parameters())
    names = [k for k, _ in named]
    proj = np.zeros((len(names), 2), dtype=np.float64)
    norms = np.zeros((len(names), 2), dtype=np.float64)
    for i, (k, p_) in enumerate(named):
        gr = p_.grad.detach()
        for j in range(2):
            proj[i, j] = float((gr.double() * proj_vector(k, j, gr.shape).double()).sum())
        norms[i] = (float(gr.double().pow(2).sum().sqrt()), float(gr.abs().max()))
    fulls = {"full." + k: p_.grad for k, p_ in named if k in FULL_GRADS}
    assert len(fulls) == len(FULL_GRADS), sorted(fulls)
    dx = xin.grad
    mg.save(f"chans_grad_tiny_128_{tag}", loss=loss.detach().double(), y=y.detach(), dx_crop=dx[:, :, 32:96, 32:96], dx_pooled16=torch.nn.functional.avg_pool2d(dx, 16),
            dx_absmax=dx.abs().max(), masks=masks, drop_rates=np.array(rates), param_names=np.array(names), proj=proj, norms=norms, dd_in=dd_in,
            in_chans=in_chans, seed=1234, in_seed=6321, target_seed=6322, sd_sha256=mg.sd_digest(sd), **fulls)
    print(f"tiny {tag} train-mode loss {float(loss):.6f}; masks {tuple(masks.shape)}, {int((masks == 0).sum())} dropped branch-samples; {len(names)} parameters")


def main():
    torch.set_num_threads(8)
    forward_fixtures()
    for dd_in, in_chans in GRAD_PAIRS:
        grad_fixture(dd_in, in_chans)


if __name__ == "__main__":
    main()
