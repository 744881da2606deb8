"""CPU: ``token_mlp='ffn'`` (the reference's Mlp in place of LeFF, model.py:890-891) at the module boundary -- key layout, strict loading,
flops, what still raises -- the fp32 restatement tests/ffn_composition.py pinned to the reference's own outputs
(tests/golden/ffn_*.npz, tests/golden/make_golden_ffn.py), and ``uf_ffn_fwd``'s argument validation, which runs before any launch."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ffn_composition as FC
from uformer_amd import _lib, model, spec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def ffn_spec():
    with open(os.path.join(GOLDEN, "ffn_spec.json")) as f:
        return json.load(f)


def ffn_cfg(img_size=128):
    import dataclasses
    return dataclasses.replace(spec.arch_config("tiny32", img_size=img_size), token_mlp="ffn")


def build(cfg, **kw):
    return model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                         modulator=cfg.modulator, dd_in=cfg.dd_in, token_mlp=cfg.token_mlp, **kw)


def test_key_layout_matches_the_reference(ffn_spec):
    cfg = ffn_cfg()
    want = [(k, tuple(s)) for k, s in ffn_spec["state_dict"]]
    assert [(k, tuple(s)) for k, s, _ in spec.state_dict_spec(cfg)] == want
    m = build(cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert sum(p.numel() for p in m.parameters()) == ffn_spec["n_parameters"]
    assert isinstance(m.conv.blocks[0].mlp, model.Mlp) and m.cfg.token_mlp == "ffn"
    assert "token_mlp=ffn" in m.extra_repr()
    sd = spec.synth_state_dict(cfg, 3)
    assert list(sd) == [k for k, _ in want] and all(tuple(sd[k].shape) == s for k, s in want)
    for alias in ("mlp",):       # model.py:890: both names build Mlp
        assert list(build(dataclasses_replace(cfg, alias)).state_dict()) == [k for k, _ in want]


def dataclasses_replace(cfg, token_mlp):
    import dataclasses
    return dataclasses.replace(cfg, token_mlp=token_mlp)


def test_strict_loading_in_the_three_payload_forms():
    cfg = ffn_cfg()
    sd = spec.synth_state_dict(cfg, 1234)
    for payload in (sd, {"epoch": 1, "state_dict": sd}, {"state_dict": {"module." + k: v for k, v in sd.items()}}, {"module." + k: v for k, v in sd.items()}):
        m = build(cfg)
        m.load_state_dict(payload, strict=True)
        assert torch.equal(m.conv.blocks[1].mlp.fc2.weight, sd["conv.blocks.1.mlp.fc2.weight"])
    with pytest.raises(RuntimeError):           # a LeFF checkpoint does not load into an 'ffn' model, and vice versa
        build(cfg).load_state_dict(spec.synth_state_dict(spec.arch_config("tiny32", img_size=128), 1234), strict=True)
    with pytest.raises(RuntimeError):
        build(spec.arch_config("tiny32", img_size=128)).load_state_dict(sd, strict=True)


def test_flops_equal_the_reference_count(ffn_spec):
    """Uformer.flops() is the exact multiply-accumulate count; the reference's adds one per LayerNorm channel and counts Upsample 4x
    (model.py:776, :1000-1004).  With those two documented terms (computed by the fixture script) it is the reference's figure."""
    m = build(ffn_cfg())
    assert m.flops() + ffn_spec["flops_layernorm_term"] + ffn_spec["flops_upsample_overcount"] == ffn_spec["flops"]
    leff = build(spec.arch_config("tiny32", img_size=128))
    dims, div = leff.cfg.stage_dims(), leff.cfg.stage_res_div()
    assert leff.flops() - m.flops() == sum(leff.cfg.depths[s] * (128 // div[s]) ** 2 * dims[s] * 36 for s in range(9))   # the 9 depthwise taps x 4C


def test_other_token_mlps_still_raise_and_leff_is_unchanged():
    with pytest.raises(NotImplementedError, match="fastleff"):
        model.Uformer(img_size=128, token_mlp="fastleff")
    with pytest.raises(NotImplementedError):
        model.LeWinTransformerBlock(32, (16, 16), 1, token_mlp="conv")
    with pytest.raises(NotImplementedError, match="token_mlp"):     # 4x4 bottleneck windows and C = 1024 stay LeFF-only
        model.Uformer(img_size=64, token_mlp="ffn")
    with pytest.raises(NotImplementedError, match="token_mlp"):
        model.Uformer(img_size=128, embed_dim=64, token_mlp="ffn")
    cfg = spec.arch_config("tiny32", img_size=128)
    assert cfg.token_mlp == "leff"
    m = build(cfg)
    keys = list(m.state_dict())
    assert keys == [k for k, _, _ in spec.state_dict_spec(cfg)]
    assert sum(k.endswith("mlp.dwconv.0.weight") for k in keys) == sum(cfg.depths) and not any(".fc1." in k for k in keys)
    assert isinstance(model.get_arch("Uformer_T", 128).conv.blocks[0].mlp, model.LeFF)
    assert abs(model.get_arch("Uformer_B", 256).flops() / 1e9 - 86.574) < 1e-2


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_matches_the_reference_block(golden, tag):
    g = golden("ffn_lewin_block_" + tag)
    p = {k[2:]: t(v) for k, v in g.items() if k.startswith("p.")}
    y = FC.lewin_block(t(g["x"]), p, "", int(g["heads"]), int(g["shift"]), 16, 16)
    assert (y - t(g["y"])).abs().max().item() < 2e-5          # f32 round-off of O(1) activations over one block


def test_restatement_matches_the_reference_model(golden):
    g = golden("ffn_model_tiny32_128")
    cfg = ffn_cfg()
    sd = spec.synth_state_dict(cfg, int(g["seed"]))
    kw = dict(img_size=128, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads)
    with torch.no_grad():
        y = FC.uformer_forward(spec.synth_input(2, 128, 128, int(g["in_seed"])), sd, **kw)
        assert (y - t(g["y"])).abs().max().item() < 2e-5
        # the rectangular fixture is this composition's own output (the reference is square-only): it must reproduce, and its two square halves'
        # worth of geometry must not be a transposed or mis-strided variant -- an all-ones DropPath scale is the identity
        gr = golden("ffn_model_tiny32_128x256")
        xr = spec.synth_input(1, 128, 256, int(gr["in_seed"]))
        yr = FC.uformer_forward(xr, sd, **kw)
        assert (yr - t(gr["y"])).abs().max().item() < 2e-5
        ones = torch.ones(2 * sum(cfg.depths), 1)
        assert torch.equal(FC.uformer_forward(xr, sd, drop_scales=ones, **kw), yr)


def test_uf_ffn_fwd_validates_its_arguments_without_a_gpu():
    """On the pattern of test_errors_cross_the_abi_as_codes: every rejection happens before a launch (fake, aligned addresses are never read)."""
    lib = _lib.load()
    A = 4096

    def call(x=A, ld=64, g=A, b=A, w1=A, b1=A, w2=A, b2=A, scale=None, B=1, M=64, C=64, dt=1):
        return lib.uf_ffn_fwd(x, ld, g, b, w1, b1, w2, b2, scale, B, M, C, dt, None)

    for name in ("x", "g", "b", "w1", "b1", "w2", "b2"):
        assert call(**{name: None}) == -6 and "null" in _lib.last_error()
    for C in (0, 8, 48, 96, 1024):
        assert call(C=C, ld=1024) == -2 and f"C={C}" in _lib.last_error()
    assert call(dt=7) == -2
    assert call(M=96) == -1 and "M=96" in _lib.last_error()          # M % 64
    assert call(M=0) == -1 and call(B=0) == -1
    assert call(M=192, B=2) == -1                                   # 96 tokens per image: a 64-row tile would straddle two images
    assert call(ld=32) == -3 and call(ld=66) == -3                  # ld < C; rows not 16-byte aligned
    assert call(x=A + 4) == -3 and call(w1=A + 8) == -3 and call(b2=A + 4) == -3
    bp = _lib.BlockParams()                                          # all-NULL descriptor: wdw9 = bdw = NULL reads as an Mlp block
    assert lib.uf_mlp_fwd(ctypes.byref(bp), A, 64, 1, 8, 8, 64, 1, A, 1 << 20, None) == -1      # heads = 0 is a shape error, before anything is read
    bp.heads = 2
    assert lib.uf_mlp_fwd(ctypes.byref(bp), A, 1024, 1, 8, 8, 1024, 1, A, 1 << 30, None) == -2 and "token_mlp" in _lib.last_error()
    bp.wdw9 = A                                                      # half a LeFF
    assert lib.uf_mlp_fwd(ctypes.byref(bp), A, 64, 1, 8, 8, 64, 1, A, 1 << 20, None) == -6
    bp.bdw = A
    assert lib.uf_mlp_fwd(ctypes.byref(bp), A, 64, 1, 8, 8, 64, 1, A, 1 << 20, None) == -2 and "LeFF" in _lib.last_error()
    bp4 = _lib.Block4Params()
    assert lib.uf_lewin_block4_fwd(ctypes.byref(bp4), A, 64, 1, 4, 4, 64, None, None, 1, A, 1 << 20, None) == -2 and "token_mlp" in _lib.last_error()
