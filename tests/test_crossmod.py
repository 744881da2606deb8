"""CPU: ``cross_modulator=True`` (the reference's cross_modulator / cross_attn / norm_cross in every decoder block, model.py:873-877, :945-949) at the
module boundary -- key layout, strict loading, packing, flops, what is refused -- the fp32 restatement tests/crossmod_composition.py pinned to the
reference's own outputs (tests/golden/crossmod_*.npz, tests/golden/make_golden_crossmod.py), and ``uf_cross_attn_fwd``'s argument validation, which
runs before any launch."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import crossmod_composition as XC
from uformer_amd import _lib, model, packing, spec, train

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def cross_spec():
    with open(os.path.join(GOLDEN, "crossmod_spec.json")) as f:
        return json.load(f)


def cross_cfg(img_size=128, **kw):
    return dataclasses.replace(spec.arch_config("tiny32", img_size=img_size), cross_modulator=True, **kw)


def build(cfg, **kw):
    return model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                         modulator=cfg.modulator, dd_in=cfg.dd_in, token_mlp=cfg.token_mlp, token_projection=cfg.token_projection,
                         cross_modulator=cfg.cross_modulator, **kw)


def test_key_layout_matches_the_reference(cross_spec):
    cfg = cross_cfg()
    want = [(k, tuple(s)) for k, s in cross_spec["state_dict"]]
    assert [(k, tuple(s)) for k, s, _ in spec.state_dict_spec(cfg)] == want
    m = build(cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert list(m.state_dict()) == [k for k, _ in want]
    assert sum(p.numel() for p in m.parameters()) == cross_spec["n_parameters"]
    sd = spec.synth_state_dict(cfg, 3)
    assert list(sd) == [k for k, _ in want] and all(tuple(sd[k].shape) == s for k, s in want)
    assert m.cfg.cross_modulator and [m.cfg.stage_has_cross_modulator(s) for s in range(9)] == [False] * 5 + [True] * 4
    assert not spec.UformerConfig().cross_modulator                                 # the default, and the default layout, are unchanged
    plain = spec.arch_config("tiny32", img_size=128)
    assert not any("cross" in k for k, _, _ in spec.state_dict_spec(plain))
    assert sum(k.endswith("cross_modulator.weight") for k, _ in want) == sum(cfg.depths[5:])


def test_submodules_are_registered_in_the_reference_order():
    blk = model.LeWinTransformerBlock(32, (16, 16), 1, shift_size=4, modulator=True, cross_modulator=True)
    assert [n for n, _ in blk.named_children()] == ["modulator", "cross_modulator", "cross_attn", "norm_cross", "norm1", "attn", "norm2", "mlp"]
    assert isinstance(blk.cross_attn, model.Attention) and isinstance(blk.cross_attn.qkv, model.LinearProjection)
    assert tuple(blk.cross_modulator.weight.shape) == (64, 32) and isinstance(blk.norm_cross, torch.nn.LayerNorm)
    assert not hasattr(blk.cross_attn, "relative_position_bias_table")
    conv = model.LeWinTransformerBlock(32, (16, 16), 1, token_projection="conv", cross_modulator=True)   # Attention builds a LinearProjection whatever
    assert isinstance(conv.cross_attn.qkv, model.LinearProjection) and isinstance(conv.attn.qkv, model.ConvProjection)   # token_projection says
    assert model.LeWinTransformerBlock(32, (16, 16), 1).cross_modulator is None
    lay = model.BasicUformerLayer(32, 32, (16, 16), 2, 1, 8, token_mlp="leff", cross_modulator=True)
    assert all(b.cross_modulator is not None for b in lay.blocks)
    m = build(cross_cfg())
    for name in spec.STAGES[:5]:
        assert all(b.cross_modulator is None for b in getattr(m, name).blocks)
    for name in spec.STAGES[5:]:
        assert all(b.cross_modulator is not None for b in getattr(m, name).blocks)
    g = model.get_arch("Uformer_T", 128, cross_modulator=True)
    assert g.cfg.cross_modulator and g.decoderlayer_0.blocks[0].cross_attn.num_heads == 16
    assert model.get_arch("Uformer_T", 128).decoderlayer_0.blocks[0].cross_modulator is None
    both = build(cross_cfg(token_mlp="ffn", token_projection="conv"))
    assert list(both.state_dict()) == [k for k, _, _ in spec.state_dict_spec(cross_cfg(token_mlp="ffn", token_projection="conv"))]


def test_strict_loading():
    cfg = cross_cfg()
    sd = spec.synth_state_dict(cfg, 1234)
    for payload in (sd, {"epoch": 1, "state_dict": sd}, {"module." + k: v for k, v in sd.items()}):
        m = build(cfg)
        m.load_state_dict(payload, strict=True)
        assert torch.equal(m.decoderlayer_1.blocks[1].cross_attn.qkv.to_kv.weight, sd["decoderlayer_1.blocks.1.cross_attn.qkv.to_kv.weight"])
    with pytest.raises(RuntimeError):           # a checkpoint without the cross-modulator does not load into a model with it, and vice versa
        build(cfg).load_state_dict(spec.synth_state_dict(spec.arch_config("tiny32", img_size=128), 1234), strict=True)
    with pytest.raises(RuntimeError):
        build(spec.arch_config("tiny32", img_size=128)).load_state_dict(sd, strict=True)


def test_flops_equal_the_reference_count(cross_spec):
    """As tests/test_convproj.py: the exact count plus the reference's two documented extra terms is the reference's figure (the LayerNorm term counts
    norm_cross, whose output the reference discards); against a model without the flag the difference is the cross attention's own terms."""
    m = build(cross_cfg())
    assert m.flops() + cross_spec["flops_layernorm_term"] + cross_spec["flops_upsample_overcount"] == cross_spec["flops"]
    plain = build(spec.arch_config("tiny32", img_size=128))
    dims, div = plain.cfg.stage_dims(), plain.cfg.stage_res_div()
    want = 0
    for s in range(5, 9):
        L, C = (128 // div[s]) ** 2, dims[s]
        a = m.decoderlayer_0.blocks[0].cross_attn if s == 5 else getattr(m, spec.STAGES[s]).blocks[0].cross_attn
        assert a.flops(L, 64) == L * C * C + 64 * C * 2 * C + 2 * L * C * 64 + L * C * C
        want += plain.cfg.depths[s] * a.flops(L, 64)
    assert m.flops() - plain.flops() == want


def test_pack_cross_layouts():
    C, heads = 64, 4
    hd = C // heads
    blk = model.LeWinTransformerBlock(C, (16, 16), heads, cross_modulator=True)
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.copy_(torch.randn(p_.shape))
    sd = blk.state_dict()
    assert packing.cross_modulator_keys(sd, "") and not packing.cross_modulator_keys(model.LeWinTransformerBlock(C, (16, 16), heads).state_dict(), "")
    for dtype in (torch.float32, torch.bfloat16):
        cp, keep = packing.pack_cross(sd, "", heads, dtype)
        kv = torch.nn.functional.linear(sd["cross_modulator.weight"], sd["cross_attn.qkv.to_kv.weight"], sd["cross_attn.qkv.to_kv.bias"])
        assert tuple(keep["k"].shape) == (heads, 64, hd) and tuple(keep["vt"].shape) == (heads, hd, 64) and keep["k"].dtype == keep["vt"].dtype == dtype
        for h in range(heads):
            assert torch.equal(keep["k"][h], kv[:, h * hd:(h + 1) * hd].to(dtype))                       # NOT scaled by hd^-0.5
            assert torch.equal(keep["vt"][h], kv[:, C + h * hd:C + (h + 1) * hd].t().to(dtype))          # transposed: [d][key]
        assert torch.equal(keep["wq_fm"], packing.pack_frag(sd["cross_attn.qkv.to_q.weight"], dtype))
        assert torch.equal(keep["wp_fm"], packing.pack_frag(sd["cross_attn.proj.weight"], dtype))
        assert torch.equal(keep["bq"], sd["cross_attn.qkv.to_q.bias"]) and torch.equal(keep["bp"], sd["cross_attn.proj.bias"])
        assert keep["bq"].dtype == keep["bp"].dtype == torch.float32
        assert all(keep[n].is_contiguous() and getattr(cp, n) == keep[n].data_ptr() for n in ("wq_fm", "bq", "k", "vt", "wp_fm", "bp")) and cp.heads == heads
    cp, keep = packing.pack_cross(model.LeWinTransformerBlock(C, (16, 16), heads).state_dict(), "", heads, torch.bfloat16)
    assert cp.wq_fm is None and cp.k is None and not keep                                               # no flag: the NULL entry
    names = [n for n, _ in _lib.CrossParams._fields_]
    assert names == ["wq_fm", "bq", "k", "vt", "wp_fm", "bp", "heads"] and _lib.CrossParams.heads.offset == 6 * 8
    # uf_block_params is unchanged and uf_model_desc gained one pointer at its end
    assert [n for n, _ in _lib.BlockParams._fields_][-4:] == ["shift", "heads", "qkv_dw9", "qkv_bdw"] and _lib.BlockParams.shift.offset == 19 * 8
    assert [n for n, _ in _lib.ModelDesc._fields_][-2:] == ["down_w_fm", "cross"] and _lib.ModelDesc.cross.offset == _lib.ModelDesc.down_w_fm.offset + 32
    # the block's own pack is cached and follows (data_ptr, _version)
    a = blk._pack_cross(torch.bfloat16)
    assert blk._pack_cross(torch.bfloat16) is a
    with torch.no_grad():
        blk.cross_modulator.weight.add_(1.0)
    b = blk._pack_cross(torch.bfloat16)
    assert b is not a and blk._pack_cross(torch.bfloat16) is b


def test_packed_model_aligns_the_cross_entries_with_the_blocks():
    cfg = cross_cfg()
    sd = spec.synth_state_dict(cfg, 5)
    pk = packing.PackedModel(cfg, sd, torch.bfloat16)
    n_enc = sum(cfg.depths[:5])
    assert len(pk.cross) == sum(cfg.depths) and all(pk.cross[i].wq_fm is None for i in range(n_enc))
    assert all(pk.cross[i].wq_fm is not None and pk.cross[i].heads == pk.blocks[i].heads for i in range(n_enc, sum(cfg.depths)))
    assert ctypes.cast(pk.desc.cross, ctypes.c_void_p).value == ctypes.addressof(pk.cross)
    plain = spec.arch_config("tiny32", img_size=128)
    pp = packing.PackedModel(plain, spec.synth_state_dict(plain, 5), torch.bfloat16)
    assert pp.cross is None and not pp.desc.cross                                   # NULL: the same launches as before
    lib = _lib.load()
    for dt in (0, 1, 2):
        for B, H, W in ((1, 128, 128), (8, 128, 256)):
            assert lib.uf_uformer_workspace_bytes(pk.desc, B, H, W, dt) == lib.uf_uformer_workspace_bytes(pp.desc, B, H, W, dt) > 0


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_matches_the_reference_block(golden, tag):
    g = golden("crossmod_lewin_block_" + tag)
    p = {k[2:]: t(v) for k, v in g.items() if k.startswith("p.")}
    y = XC.lewin_block(t(g["x"]), p, "", int(g["heads"]), int(g["shift"]), 16, 16)
    assert (y - t(g["y"])).abs().max().item() < 2e-5          # f32 round-off of O(1) activations over one block
    noisy = dict(p, **{"norm_cross.weight": p["norm_cross.weight"] * 3 + 1, "norm_cross.bias": p["norm_cross.bias"] - 2})
    assert torch.equal(XC.lewin_block(t(g["x"]), noisy, "", int(g["heads"]), int(g["shift"]), 16, 16), y)     # norm_cross is never read
    blk = model.LeWinTransformerBlock(int(g["C"]), (16, 16), int(g["heads"]), shift_size=int(g["shift"]), modulator=(tag == "a"), cross_modulator=True)
    blk.load_state_dict(p, strict=True)                        # the reference block's own state_dict loads strictly
    assert list(blk.state_dict()) == list(p)


def test_restatement_matches_the_reference_model(golden):
    g = golden("crossmod_model_tiny32_128")
    cfg = cross_cfg()
    sd = spec.synth_state_dict(cfg, int(g["seed"]))
    kw = dict(img_size=128, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads)
    with torch.no_grad():
        y = XC.uformer_forward(spec.synth_input(2, 128, 128, int(g["in_seed"])), sd, **kw)
        assert (y - t(g["y"])).abs().max().item() < 2e-5
        gr = golden("crossmod_model_tiny32_128x256")          # this composition's own output (the reference is square-only): it must reproduce
        yr = XC.uformer_forward(spec.synth_input(1, 128, 256, int(gr["in_seed"])), sd, **kw)
        assert (yr - t(gr["y"])).abs().max().item() < 2e-5


def test_what_is_refused_names_cross_modulator():
    with pytest.raises(NotImplementedError, match="cross_modulator"):          # 4x4 bottleneck windows
        model.Uformer(img_size=64, cross_modulator=True)
    with pytest.raises(NotImplementedError, match="cross_modulator"):          # head_dim 64
        model.Uformer(img_size=128, embed_dim=64, cross_modulator=True)
    with pytest.raises(NotImplementedError, match="cross_modulator"):
        model.Uformer(img_size=128, use_checkpoint=True, cross_modulator=True)
    with pytest.raises(NotImplementedError, match="cross_modulator"):
        model.BasicUformerLayer(32, 32, (16, 16), 2, 1, 8, use_checkpoint=True, cross_modulator=True)
    cfg = cross_cfg()
    m = build(cfg)
    x = spec.synth_input(1, 128, 128, 1)
    with pytest.raises(NotImplementedError, match="cross_modulator"):          # grad mode on, parameters requiring grad: the autograd path
        m(x)
    with pytest.raises(NotImplementedError, match="cross_modulator"):
        m.eval()(x.requires_grad_(True))
    blk = model.LeWinTransformerBlock(32, (16, 16), 1, cross_modulator=True)
    with pytest.raises(NotImplementedError, match="cross_modulator"):
        blk(torch.zeros(1, 256, 32))
    with pytest.raises(NotImplementedError, match="cross_modulator"):          # no stand-alone forward: the cross attention runs fused in its block
        blk.cross_attn(torch.zeros(1, 256, 32), blk.cross_modulator.weight)
    with pytest.raises(NotImplementedError, match="cross-modulator"):          # WindowAttention(attn_kv=...) stays refused as before
        blk.attn(torch.zeros(4, 64, 32), attn_kv=blk.cross_modulator.weight)
    sd = spec.synth_state_dict(cfg, 1)
    with pytest.raises(NotImplementedError, match="cross_modulator"):          # the training tape
        train.UformerTape(sd, cfg, torch.bfloat16)
    with pytest.raises(NotImplementedError, match="cross_modulator"):
        train.BlockPack(sd, "decoderlayer_0.blocks.0.", 16, 0, torch.bfloat16, fused=False)
    with pytest.raises(NotImplementedError, match="cross_modulator"):
        train.NativeBlockPack(sd, "decoderlayer_0.blocks.0.", 16, 0, torch.bfloat16)
    with pytest.raises(NotImplementedError, match="cross_modulator"):
        packing.pack_block4(sd, "decoderlayer_0.blocks.0.", 16, torch.bfloat16)
    assert train.CROSS_MODULATOR_TRAINING.startswith("cross_modulator")
    assert not packing.cross_modulator_keys(sd, "encoderlayer_0.blocks.0.")      # told by the parameter names: encoder blocks carry none


def test_uf_cross_attn_fwd_validates_its_arguments_without_a_gpu():
    """On the pattern of test_uf_ln_convqkv_fwd_validates_its_arguments_without_a_gpu: every rejection happens before a launch (fake, aligned
    addresses are never read)."""
    lib = _lib.load()
    A = 4096

    def call(x=A, ld=64, M=64, C=64, heads=2, dt=1, p=True, **fields):
        cp = _lib.CrossParams()
        for n in ("wq_fm", "bq", "k", "vt", "wp_fm", "bp"):
            setattr(cp, n, fields.get(n, A))
        cp.heads = heads
        return lib.uf_cross_attn_fwd(ctypes.byref(cp) if p else None, x, ld, M, C, dt, None)

    assert call(p=False) == -6 and "null" in _lib.last_error()
    assert call(x=None) == -6 and "x is null" in _lib.last_error()
    for name in ("wq_fm", "bq", "k", "vt", "wp_fm", "bp"):
        assert call(**{name: None}) == -6 and name in _lib.last_error()
    for C in (8, 48, 96, 1024):
        assert call(C=C, ld=1024, heads=1) == -2 and f"C={C}" in _lib.last_error()
    assert call(dt=7) == -2 and "dtype" in _lib.last_error()
    assert call(heads=3) == -1 and "heads=3" in _lib.last_error()
    assert call(heads=0) == -1 and "heads=0" in _lib.last_error()
    assert call(heads=1) == -2 and "head_dim 64" in _lib.last_error()              # C = 64, one head
    assert call(C=512, ld=512, heads=64) == -2 and "head_dim 8" in _lib.last_error()
    for M in (0, -64, 32, 100):
        assert call(M=M) == -1 and f"M={M}" in _lib.last_error()
    assert call(ld=32) == -1 and "ld=32" in _lib.last_error()                      # ld < C
    assert call(ld=66) == -1 and "ld=66" in _lib.last_error()                      # rows not 16-byte aligned
    for bad in (dict(x=A + 4), dict(wq_fm=A + 8), dict(bq=A + 4), dict(k=A + 2), dict(vt=A + 8), dict(wp_fm=A + 8), dict(bp=A + 4)):
        assert call(**bad) == -3 and "aligned" in _lib.last_error()
