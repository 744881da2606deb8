"""CPU: ``token_projection='conv'`` (the reference's ConvProjection in place of LinearProjection, model.py:480-481) at the module boundary --
key layout, strict loading, packing, flops, what is refused -- the fp32 restatement tests/convproj_composition.py pinned to the reference's own
outputs (tests/golden/convproj_*.npz, tests/golden/make_golden_convproj.py), and ``uf_ln_convqkv_fwd``'s argument validation, which runs
before any launch."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import convproj_composition as CC
from uformer_amd import _lib, model, packing, spec, train

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def conv_spec():
    with open(os.path.join(GOLDEN, "convproj_spec.json")) as f:
        return json.load(f)


def conv_cfg(img_size=128, **kw):
    return dataclasses.replace(spec.arch_config("tiny32", img_size=img_size), token_projection="conv", **kw)


def build(cfg, **kw):
    return model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                         modulator=cfg.modulator, dd_in=cfg.dd_in, token_mlp=cfg.token_mlp, token_projection=cfg.token_projection, **kw)


def test_key_layout_matches_the_reference(conv_spec):
    cfg = conv_cfg()
    want = [(k, tuple(s)) for k, s in conv_spec["state_dict"]]
    assert [(k, tuple(s)) for k, s, _ in spec.state_dict_spec(cfg)] == want
    m = build(cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert sum(p.numel() for p in m.parameters()) == conv_spec["n_parameters"]
    assert isinstance(m.conv.blocks[0].attn.qkv, model.ConvProjection) and isinstance(m.conv.blocks[0].attn.qkv.to_k, model.SepConv2d)
    assert m.cfg.token_projection == "conv" and "token_projection=conv" in m.extra_repr()
    sd = spec.synth_state_dict(cfg, 3)
    assert list(sd) == [k for k, _ in want] and all(tuple(sd[k].shape) == s for k, s in want)
    assert spec.UformerConfig().token_projection == "linear"                    # the default, and the linear layout, are unchanged
    lin = spec.arch_config("tiny32", img_size=128)
    assert sum(k.endswith("attn.qkv.to_kv.weight") for k, _, _ in spec.state_dict_spec(lin)) == sum(lin.depths)


def test_strict_loading_in_the_three_payload_forms():
    cfg = conv_cfg()
    sd = spec.synth_state_dict(cfg, 1234)
    for payload in (sd, {"epoch": 1, "state_dict": sd}, {"state_dict": {"module." + k: v for k, v in sd.items()}}, {"module." + k: v for k, v in sd.items()}):
        m = build(cfg)
        m.load_state_dict(payload, strict=True)
        assert torch.equal(m.conv.blocks[1].attn.qkv.to_v.depthwise.weight, sd["conv.blocks.1.attn.qkv.to_v.depthwise.weight"])
    with pytest.raises(RuntimeError):           # a 'linear' checkpoint does not load into a 'conv' model, and vice versa
        build(cfg).load_state_dict(spec.synth_state_dict(spec.arch_config("tiny32", img_size=128), 1234), strict=True)
    with pytest.raises(RuntimeError):
        build(spec.arch_config("tiny32", img_size=128)).load_state_dict(sd, strict=True)


def test_flops_equal_the_reference_count(conv_spec):
    """As tests/test_ffn.py: the exact count plus the reference's two documented extra terms is the reference's figure; against a 'linear' model the
    difference is the 27 depthwise taps per token and channel."""
    m = build(conv_cfg())
    assert m.flops() + conv_spec["flops_layernorm_term"] + conv_spec["flops_upsample_overcount"] == conv_spec["flops"]
    lin = build(spec.arch_config("tiny32", img_size=128))
    dims, div = lin.cfg.stage_dims(), lin.cfg.stage_res_div()
    assert m.flops() - lin.flops() == sum(lin.cfg.depths[s] * (128 // div[s]) ** 2 * dims[s] * 27 for s in range(9))


def test_packing_shapes_and_tap_order():
    C = 32
    blk = model.LeWinTransformerBlock(C, (16, 16), 1, shift_size=4, token_projection="conv", modulator=True)
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.copy_(torch.randn(p_.shape))
    sd = blk.state_dict()
    assert packing.conv_projection_keys(sd, "") and not packing.conv_projection_keys(model.LeWinTransformerBlock(C, (16, 16), 1).state_dict(), "")
    wpw, bpw, dw9, bdw = packing.pack_conv_projection(sd, "")
    assert tuple(wpw.shape) == (3 * C, C) and tuple(bpw.shape) == (3 * C,) and tuple(dw9.shape) == (3, 9, C) and tuple(bdw.shape) == (3, C)
    assert dw9.dtype == bdw.dtype == bpw.dtype == torch.float32 and dw9.is_contiguous() and bdw.is_contiguous()
    for j, name in enumerate("qkv"):
        w = sd[f"attn.qkv.to_{name}.depthwise.weight"]
        for ky in range(3):
            for kx in range(3):
                assert torch.equal(dw9[j, ky * 3 + kx], w[:, 0, ky, kx])                    # tap-major, tap = ky * 3 + kx (cross-correlation order)
        assert torch.equal(bdw[j], sd[f"attn.qkv.to_{name}.depthwise.bias"])
        assert torch.equal(wpw[j * C:(j + 1) * C], sd[f"attn.qkv.to_{name}.pointwise.weight"][:, :, 0, 0])     # row = output channel
        assert torch.equal(bpw[j * C:(j + 1) * C], sd[f"attn.qkv.to_{name}.pointwise.bias"])
    bp, keep = packing.pack_block(sd, "", 1, 4, torch.bfloat16)
    assert bp.qkv_dw9 == keep["qkv_dw9"].data_ptr() and bp.qkv_bdw == keep["qkv_bdw"].data_ptr() and bp.shift == 4 and bp.heads == 1
    assert torch.equal(keep["wqkv_fm"], packing.pack_frag(wpw, torch.bfloat16)) and torch.equal(keep["bqkv"], bpw)
    bp, _ = packing.pack_block(model.LeWinTransformerBlock(C, (16, 16), 1).state_dict(), "", 1, 0, torch.bfloat16)
    assert bp.qkv_dw9 is None and bp.qkv_bdw is None                                        # a linear block leaves the new fields NULL
    names = [n for n, _ in _lib.BlockParams._fields_]
    assert names[-4:] == ["shift", "heads", "qkv_dw9", "qkv_bdw"] and _lib.BlockParams.shift.offset == 19 * 8   # appended: no earlier field moved


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_matches_the_reference_block(golden, tag):
    g = golden("convproj_lewin_block_" + tag)
    p = {k[2:]: t(v) for k, v in g.items() if k.startswith("p.")}
    y = CC.lewin_block(t(g["x"]), p, "", int(g["heads"]), int(g["shift"]), 16, 16)
    assert (y - t(g["y"])).abs().max().item() < 2e-5          # f32 round-off of O(1) activations over one block
    blk = model.LeWinTransformerBlock(int(g["C"]), (16, 16), int(g["heads"]), shift_size=int(g["shift"]), token_projection="conv", modulator=(tag == "a"))
    blk.load_state_dict(p, strict=True)                        # the reference block's own state_dict loads strictly


def test_restatement_matches_the_reference_model(golden):
    g = golden("convproj_model_tiny32_128")
    cfg = conv_cfg()
    sd = spec.synth_state_dict(cfg, int(g["seed"]))
    kw = dict(img_size=128, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads)
    with torch.no_grad():
        y = CC.uformer_forward(spec.synth_input(2, 128, 128, int(g["in_seed"])), sd, **kw)
        assert (y - t(g["y"])).abs().max().item() < 2e-5
        gr = golden("convproj_model_tiny32_128x256")          # this composition's own output (the reference is square-only): it must reproduce
        yr = CC.uformer_forward(spec.synth_input(1, 128, 256, int(gr["in_seed"])), sd, **kw)
        assert (yr - t(gr["y"])).abs().max().item() < 2e-5


def test_constructors_accept_conv():
    assert isinstance(model.WindowAttention(32, (8, 8), 1, token_projection="conv").qkv, model.ConvProjection)
    assert model.LeWinTransformerBlock(64, (16, 16), 2, token_projection="conv").token_projection == "conv"
    lay = model.BasicUformerLayer(32, 32, (16, 16), 2, 1, 8, token_projection="conv", token_mlp="leff")
    assert [b.shift_size for b in lay.blocks] == [0, 4] and isinstance(lay.blocks[1].attn.qkv, model.ConvProjection)
    m = model.get_arch("Uformer_T", 128, token_projection="conv")
    assert m.token_projection == "conv" and isinstance(m.decoderlayer_3.blocks[0].attn.qkv, model.ConvProjection)
    assert isinstance(model.get_arch("Uformer_T", 128).conv.blocks[0].attn.qkv, model.LinearProjection)
    both = build(conv_cfg(token_mlp="ffn"))                                                 # the two halves are independent
    assert isinstance(both.conv.blocks[0].mlp, model.Mlp) and isinstance(both.conv.blocks[0].attn.qkv, model.ConvProjection)
    assert list(both.state_dict()) == [k for k, _, _ in spec.state_dict_spec(conv_cfg(token_mlp="ffn"))]
    with pytest.raises(NotImplementedError, match="token_projection"):
        model.WindowAttention(32, (8, 8), 1, token_projection="linear_concat")


def test_what_is_refused_names_token_projection():
    with pytest.raises(NotImplementedError, match="token_projection"):          # 4x4 bottleneck windows
        model.Uformer(img_size=64, token_projection="conv")
    with pytest.raises(NotImplementedError, match="token_projection"):          # C = 1024 at the bottleneck
        model.Uformer(img_size=128, embed_dim=64, token_projection="conv")
    with pytest.raises(NotImplementedError, match="token_projection"):
        model.Uformer(img_size=128, use_checkpoint=True, token_projection="conv")
    cfg = conv_cfg()
    m = build(cfg)
    x = spec.synth_input(1, 128, 128, 1)
    with pytest.raises(NotImplementedError, match="token_projection"):          # grad mode on, parameters requiring grad: the autograd path
        m(x)
    with pytest.raises(NotImplementedError, match="token_projection"):
        m.eval()(x.requires_grad_(True))
    blk = model.LeWinTransformerBlock(32, (16, 16), 1, token_projection="conv")
    with pytest.raises(NotImplementedError, match="token_projection"):
        blk(torch.zeros(1, 256, 32))
    with pytest.raises(NotImplementedError, match="token_projection"):          # no stand-alone forward: the projection runs fused behind norm1
        blk.attn(torch.zeros(4, 64, 32))
    sd = spec.synth_state_dict(cfg, 1)
    with pytest.raises(NotImplementedError, match="token_projection"):          # the training tape
        train.UformerTape(sd, cfg, torch.bfloat16)
    with pytest.raises(NotImplementedError, match="token_projection"):
        train.BlockPack(sd, "conv.blocks.0.", 16, 0, torch.bfloat16, fused=False)
    with pytest.raises(NotImplementedError, match="token_projection"):
        train.NativeBlockPack(sd, "conv.blocks.0.", 16, 0, torch.bfloat16)
    with pytest.raises(NotImplementedError, match="token_projection"):
        packing.pack_block4(sd, "conv.blocks.0.", 16, torch.bfloat16)


def test_uf_ln_convqkv_fwd_validates_its_arguments_without_a_gpu():
    """On the pattern of test_uf_ffn_fwd_validates_its_arguments_without_a_gpu: every rejection happens before a launch (fake, aligned
    addresses are never read)."""
    lib = _lib.load()
    A = 4096

    def call(x=A, ld=64, g=A, b=A, mod=None, dw9=A, bdw=A, w=A, bpw=A, q=A, k=A, vt=A, B=1, H=8, W=8, C=64, heads=2, shift=0, dt=1):
        return lib.uf_ln_convqkv_fwd(x, ld, g, b, mod, dw9, bdw, w, bpw, q, k, vt, B, H, W, C, heads, shift, dt, None)

    for name in ("x", "g", "b", "dw9", "bdw", "w", "bpw", "q", "k", "vt"):
        assert call(**{name: None}) == -6 and "null" in _lib.last_error()
    for C in (8, 48, 96, 1024):
        assert call(C=C, ld=1024, heads=1) == -2 and f"C={C}" in _lib.last_error()
    assert call(dt=7) == -2
    assert call(heads=3) == -1 and call(heads=0) == -1
    assert call(C=512, ld=512, heads=4) == -2 and "head_dim 128" in _lib.last_error()
    assert call(H=12) == -1 and call(B=0) == -1 and call(shift=8) == -1
    assert call(ld=32) == -3 and call(ld=66) == -3                  # ld < C; rows not 16-byte aligned
    assert call(x=A + 4) == -3 and call(w=A + 8) == -3 and call(dw9=A + 4) == -3 and call(vt=A + 8) == -3 and call(mod=A + 4) == -3
    bp = _lib.BlockParams()
    bp.heads, bp.qkv_dw9 = 2, A                                      # half a ConvProjection
    assert lib.uf_lewin_block_fwd(ctypes.byref(bp), A, 64, 1, 8, 8, 64, None, 0, 1, A, 1 << 20, None) == -6 and "qkv_bdw" in _lib.last_error()
    bp.qkv_bdw = A
    assert lib.uf_lewin_block_fwd(ctypes.byref(bp), A, 1024, 1, 8, 8, 1024, None, 0, 1, A, 1 << 30, None) == -2 and "token_projection" in _lib.last_error()
    assert lib.uf_lewin_block_train_fwd(ctypes.byref(bp), A, 64, 1, 8, 8, 64, None, None, 1, A, 1 << 20, None) == -2 and "token_projection" in _lib.last_error()
    assert lib.uf_lewin_attn_train_fwd(ctypes.byref(bp), A, 64, A, 64, 1, 8, 8, 64, None, 1, A, A, A, A, A, A, A, None) == -2
    assert "token_projection" in _lib.last_error()
