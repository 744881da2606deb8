#!/usr/bin/env python3
"""Fixtures of ``token_mlp='ffn'`` models (the reference's Mlp in place of LeFF, model.py:890-891), FROM THE REFERENCE ITSELF.

Runs only where the reference checkout is (on the pattern of make_golden_hd64.py; reuses make_golden.py's 3-symbol timm shim and
helpers and runs the reference's ``model.py`` unmodified):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ffn.py

Weights of the whole-model fixtures come from spec.synth_state_dict and inputs from spec.synth_input; neither is stored.  Writes
  * ffn_spec.json                 (a) the reference's (key, shape) state_dict layout, parameter count and ``flops()`` of tiny32 with
                                  token_mlp='ffn' at img_size 128, and the two terms by which the reference's count differs from this
                                  project's exact count (LayerNorm channels, the 4x over-count of Upsample, model.py:776);
  * ffn_lewin_block_a.npz         (b) LeWinTransformerBlock(32, (16, 16), 1 head, shift 4, modulator, token_mlp='ffn'): x, weights, y;
  * ffn_lewin_block_b.npz         (b) LeWinTransformerBlock(64, (16, 16), 2 heads, shift 0, token_mlp='ffn'): x, weights, y;
  * ffn_model_tiny32_128.npz      (c) the reference's forward of tiny32 / 'ffn' built at img_size 128 on a 2x3x128x128 input;
  * ffn_model_tiny32_128x256.npz  (c) the same weights on a 1x3x128x256 input.  The reference is square-only (model.py:910-911), so this
                                  one comes from tests/ffn_composition.py, which this script first pins to the reference's own output
                                  at 128x128 (max |diff| printed and asserted < 2e-5);
  * ffn_grad_tiny32_128.npz       (d) train() mode with drop_path_rate 0.5, the DropPath masks the reference drew recorded: Charbonnier
                                  loss, the forward output y, and every gradient of the reference's autograd as probes
                                  (tests/gradproj.py): norms, two signed projections, a seeded 256-element gather or the full tensor;
                                  d loss / d x the same way with a 4096-element gather.
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
import ffn_composition as FC  # noqa: E402
from gradproj import gather_index, proj_vector  # noqa: E402
from uformer_amd import spec  # noqa: E402

ref = mg.ref
N_GATHER = 256
FULL = ("encoderlayer_0.blocks.0.attn.relative_position_bias_table", "conv.blocks.0.mlp.fc1.bias", "output_proj.proj.0.bias")


def probes_of(named):
    names, norms, proj, probes = [], [], [], {}
    for n, gr in named:
        names.append(n)
        norms.append([float(gr.double().norm()), float(gr.abs().max())])
        proj.append([float((gr.double() * proj_vector(n, k, gr.shape).double()).sum()) for k in range(2)])
        if n in FULL or gr.numel() <= N_GATHER:
            probes["full." + n] = gr
        else:
            probes["gather." + n] = gr.reshape(-1)[gather_index(n, gr.numel(), N_GATHER)]
    return names, norms, proj, probes


def main():
    torch.set_num_threads(8)
    cfg = spec.arch_config("tiny32", img_size=128)
    cfg = type(cfg)(**{**cfg.__dict__, "token_mlp": "ffn"})
    kw = dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), win_size=8,
              token_projection="linear", token_mlp="ffn", modulator=cfg.modulator, dd_in=cfg.dd_in)
    m = ref.Uformer(**kw).eval()
    assert list(m.state_dict().keys()) == [k for k, _, _ in spec.state_dict_spec(cfg)], "state_dict key order/layout drifted"

    # ---------------- (a) layout and flops ------------------------------------------------------------------
    devnull = open(os.devnull, "w")
    stdout, sys.stdout = sys.stdout, devnull          # the reference's flops() prints per module
    try:
        ref_flops = float(m.flops())
    finally:
        sys.stdout = stdout
    dims, div = cfg.stage_dims(), cfg.stage_res_div()
    ln_term = sum(cfg.depths[s] * 2 * dims[s] * (cfg.img_size // div[s]) ** 2 for s in range(9))          # norm1 + norm2 channels, model.py:1000-1004
    up_term = sum(3 * (cfg.img_size // div[4 + k]) ** 2 * 4 * cin * cout for k, (cin, cout) in enumerate(cfg.upsample_io()))   # model.py:776 counts H*2*W*2*Cin*Cout*2*2
    with open(os.path.join(HERE, "ffn_spec.json"), "w") as f:
        json.dump({"arch": "tiny32", "token_mlp": "ffn", "img_size": 128, "embed_dim": cfg.embed_dim, "depths": list(cfg.depths),
                   "num_heads": list(cfg.num_heads), "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                   "n_parameters": int(sum(p_.numel() for p_ in m.parameters())), "flops": ref_flops,
                   "flops_layernorm_term": float(ln_term), "flops_upsample_overcount": float(up_term)}, f)
    print(f"ffn_spec.json  reference flops {ref_flops:.0f}  (LayerNorm term {ln_term}, Upsample over-count {up_term})")

    # ---------------- (b) single blocks -----------------------------------------------------------------------
    with torch.no_grad():
        blk = ref.LeWinTransformerBlock(32, (16, 16), 1, win_size=8, shift_size=4, token_mlp="ffn", modulator=True).eval()
        mg.randomize_(blk, 301)
        x = torch.randn(2, 256, 32, generator=mg.g(302))
        mg.save("ffn_lewin_block_a", C=32, heads=1, shift=4, x=x, y=blk(x), **{"p." + k: v for k, v in blk.state_dict().items()})
        blk = ref.LeWinTransformerBlock(64, (16, 16), 2, win_size=8, shift_size=0, token_mlp="ffn").eval()
        mg.randomize_(blk, 311)
        x = torch.randn(2, 256, 64, generator=mg.g(312))
        mg.save("ffn_lewin_block_b", C=64, heads=2, shift=0, x=x, y=blk(x), **{"p." + k: v for k, v in blk.state_dict().items()})

    # ---------------- (c) whole model ----------------------------------------------------------------------------
    sd = spec.synth_state_dict(cfg, 1234)
    m.load_state_dict(sd, strict=True)
    ckw = dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in)
    with torch.no_grad():
        x = spec.synth_input(2, 128, 128, 1234)
        y = m(x)
        mg.save("ffn_model_tiny32_128", y=y, arch="tiny32", token_mlp="ffn", img_size=128, B=2, H=128, W=128, seed=1234, in_seed=1234,
                sd_sha256=mg.sd_digest(sd))
        pin = (FC.uformer_forward(x, sd, **ckw) - y).abs().max().item()
        print(f"ffn_composition vs the reference at 128x128: max |diff| = {pin:.3e}")
        assert pin < 2e-5
        xr = spec.synth_input(1, 128, 256, 1236)
        mg.save("ffn_model_tiny32_128x256", y=FC.uformer_forward(xr, sd, **ckw), arch="tiny32", token_mlp="ffn", img_size=128, B=1, H=128, W=256,
                seed=1234, in_seed=1236, sd_sha256=mg.sd_digest(sd), pinned_to_reference_at_128=pin)

    # ---------------- (d) train() mode gradients, DropPath masks recorded (as make_golden_grad.py records them) -------
    import losses as ref_losses  # noqa: E402  (the reference's losses.py)
    import timm.models.layers as tl
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
    torch.manual_seed(79)
    mt = ref.Uformer(drop_path_rate=0.5, **kw).train()
    mt.load_state_dict(sd, strict=True)
    xin = spec.synth_input(2, 128, 128, 4321).requires_grad_(True)
    target = spec.synth_input(2, 128, 128, 4322)
    out = mt(xin)
    loss = ref_losses.CharbonnierLoss()(out, target)
    loss.backward()
    tl.DropPath.forward = orig_fwd
    full, it = [], iter(masks)
    for blk in [m_ for m_ in mt.modules() if isinstance(m_, ref.LeWinTransformerBlock)]:
        for _ in range(2):      # a block whose rate is 0 holds nn.Identity (model.py:887): rows of ones
            full.append(next(it) if isinstance(blk.drop_path, tl.DropPath) else torch.ones(xin.shape[0]))
    assert next(it, None) is None
    masks = torch.stack(full)
    names, norms, proj, probes = probes_of([(n, p_.grad.detach()) for n, p_ in mt.named_parameters()])
    dx = xin.grad.detach()
    mg.save("ffn_grad_tiny32_128", loss=loss.detach(), y=out.detach(), masks=masks, drop_path_rate=0.5, param_names=np.array(names),
            norms=np.array(norms), proj=np.array(proj),
            dx_norms=np.array([float(dx.double().norm()), float(dx.abs().max())]),
            dx_proj=np.array([float((dx.double() * proj_vector("dx", k, dx.shape).double()).sum()) for k in range(2)]),
            dx_gather=dx.reshape(-1)[gather_index("dx", dx.numel(), 4096)], **probes)
    print("train-mode loss %.6f  masks %s  dropped branches %d of %d  params %d" % (float(loss), tuple(masks.shape), int((masks == 0).sum()),
                                                                                     masks.numel(), len(names)))


if __name__ == "__main__":
    main()
