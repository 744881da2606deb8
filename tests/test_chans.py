"""CPU: models whose image channel counts are not 3 -> 3 (``Uformer(in_chans=..., dd_in=...)``, model.py:1100-1101, :1305) at the module boundary --
key layout, strict loading, packing, flops, what is refused and by what name -- the oracle against the reference's own outputs
(tests/golden/chans_*.npz, tests/golden/make_golden_chans.py), and the argument validation of the widened entry points, which runs before any launch."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import rect_composition as R
from oracle import uformer_oracle as O
from uformer_amd import _lib, data, model, packing, spec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAIRS = [(6, 3), (1, 1), (4, 4), (4, 3)]          # (dd_in, in_chans)


def t(a):
    return torch.from_numpy(np.asarray(a))


def tag_of(dd_in, in_chans):
    return f"d{dd_in}x{in_chans}"


def chans_cfg(dd_in, in_chans, arch="tiny32", img_size=128, **kw):
    return dataclasses.replace(spec.arch_config(arch, img_size=img_size), dd_in=dd_in, in_chans=in_chans, **kw)


def build(cfg, **kw):
    return model.Uformer(img_size=cfg.img_size, in_chans=cfg.in_chans, dd_in=cfg.dd_in, embed_dim=cfg.embed_dim, depths=list(cfg.depths),
                         num_heads=list(cfg.num_heads), modulator=cfg.modulator, token_mlp=cfg.token_mlp, token_projection=cfg.token_projection,
                         cross_modulator=cfg.cross_modulator, **kw)


@pytest.fixture(scope="module")
def chans_spec():
    with open(os.path.join(GOLDEN, "chans_spec.json")) as f:
        return json.load(f)


def okw(cfg):
    return dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in)


@pytest.mark.parametrize("dd_in,in_chans", PAIRS)
def test_oracle_reproduces_the_reference(golden, dd_in, in_chans):
    g = golden("chans_model_tiny32_128_" + tag_of(dd_in, in_chans))
    cfg = chans_cfg(dd_in, in_chans)
    sd = spec.synth_state_dict(cfg, int(g["seed"]))
    x = spec.synth_input(int(g["B"]), int(g["H"]), int(g["W"]), int(g["in_seed"]), channels=dd_in)
    assert tuple(x.shape) == (2, dd_in, 128, 128)
    y = O.uformer_forward(x, sd, **okw(cfg))
    assert tuple(y.shape) == (2, in_chans, 128, 128)
    err = (y - t(g["y"])).abs().max().item()
    assert err < 2e-5, err


def test_rect_composition_reproduces_the_rect_fixture(golden):
    g = golden("chans_model_tiny32_128x256_d6x3")
    assert float(g["pinned_to_reference_at_128"]) < 2e-5
    cfg = chans_cfg(6, 3)
    sd = spec.synth_state_dict(cfg, int(g["seed"]))
    x = spec.synth_input(1, 128, 256, int(g["in_seed"]), channels=6)
    err = (R.uformer_forward(x, sd, **okw(cfg)) - t(g["y"])).abs().max().item()
    assert err < 2e-5, err


def test_synth_input_channels():
    assert torch.equal(spec.synth_input(2, 8, 8, 5), spec.synth_input(2, 8, 8, 5, channels=3))      # the default draw is unchanged
    assert tuple(spec.synth_input(1, 8, 16, 5, channels=6).shape) == (1, 6, 8, 16)


@pytest.mark.parametrize("dd_in,in_chans", PAIRS)
def test_key_layout_strict_loading_and_flops(chans_spec, dd_in, in_chans):
    ref = chans_spec["models"][tag_of(dd_in, in_chans)]
    cfg = chans_cfg(dd_in, in_chans)
    want = [(k, tuple(s)) for k, s in ref["state_dict"]]
    assert [(k, tuple(s)) for k, s, _ in spec.state_dict_spec(cfg)] == want
    m = build(cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert sum(p.numel() for p in m.parameters()) == ref["n_parameters"]
    assert tuple(m.input_proj.proj[0].weight.shape) == (32, dd_in, 3, 3) and tuple(m.output_proj.proj[0].weight.shape) == (in_chans, 64, 3, 3)
    sd = spec.synth_state_dict(cfg, 1234)
    for payload in (sd, {"epoch": 1, "state_dict": sd}, {"module." + k: v for k, v in sd.items()}):
        m = build(cfg)
        m.load_state_dict(payload, strict=True)
        assert torch.equal(m.output_proj.proj[0].weight, sd["output_proj.proj.0.weight"])
    with pytest.raises(RuntimeError):           # an RGB checkpoint does not load into it, nor the other way round
        build(cfg).load_state_dict(spec.synth_state_dict(spec.arch_config("tiny32", img_size=128), 1234), strict=True)
    with pytest.raises(RuntimeError):
        build(spec.arch_config("tiny32", img_size=128)).load_state_dict(sd, strict=True)
    # the exact count plus the reference's two documented extra terms is the reference's figure (tests/test_crossmod.py does the same)
    assert m.flops() + ref["flops_layernorm_term"] + ref["flops_upsample_overcount"] == ref["flops"]
    rgb = build(spec.arch_config("tiny32", img_size=128))
    assert m.flops() - rgb.flops() == 128 * 128 * 9 * (32 * (dd_in - 3) + 64 * (in_chans - 3))


def test_the_accidental_broadcast_and_the_mismatch_are_refused_by_name():
    for k in (1, 2, 4):
        with pytest.raises(ValueError, match=r"dd_in=3.*in_chans=%d" % k):
            model.Uformer(img_size=128, embed_dim=16, depths=[1] * 9, dd_in=3, in_chans=k)
        with pytest.raises(ValueError, match="in_chans"):
            model.get_arch("Uformer_T", 128, in_chans=k)           # Uformer_T does not forward dd_in (utils/model_utils.py:66-67): it stays 3
    with pytest.raises(NotImplementedError, match="dd_in=9"):
        model.Uformer(img_size=128, embed_dim=16, depths=[1] * 9, dd_in=9, in_chans=3)
    with pytest.raises(NotImplementedError, match="dd_in=0"):
        model.Uformer(img_size=128, embed_dim=16, depths=[1] * 9, dd_in=0, in_chans=1)
    with pytest.raises(NotImplementedError, match="in_chans=5"):
        model.Uformer(img_size=128, embed_dim=16, depths=[1] * 9, dd_in=6, in_chans=5)
    with pytest.raises(NotImplementedError, match="in_chans=0"):
        model.Uformer(img_size=128, embed_dim=16, depths=[1] * 9, dd_in=6, in_chans=0)
    with pytest.raises(NotImplementedError, match="out_channel"):
        model.OutputProj(32, 5)
    for dd_in in range(1, 9):                                        # the whole supported set constructs
        for in_chans in range(1, 5):
            if dd_in == 3 and in_chans != 3:
                continue
            m = model.Uformer(img_size=128, embed_dim=16, depths=[1] * 9, dd_in=dd_in, in_chans=in_chans)
            assert (m.dd_in, m.in_chans, m.cfg.dd_in, m.cfg.in_chans) == (dd_in, in_chans, dd_in, in_chans)


def test_get_arch_forwards_dd_in_where_the_reference_does():
    b = model.get_arch("Uformer_B", 128, dd_in=6)
    assert (b.dd_in, b.in_chans) == (6, 3) and b.input_proj.proj[0].weight.shape[1] == 6
    b = model.get_arch("Uformer_B", 128, dd_in=4, in_chans=4)
    assert (b.dd_in, b.in_chans) == (4, 4) and b.output_proj.proj[0].weight.shape[0] == 4
    for arch in ("Uformer", "Uformer_T", "Uformer_S", "Uformer_S_noshift"):       # utils/model_utils.py:62-76 pass no dd_in
        assert model.get_arch(arch, 128, dd_in=6).dd_in == 3
    assert model.get_arch("UNet", 128, in_chans=3).conv10.weight.shape[0] == 3       # UNet stays 3-channel


@pytest.mark.parametrize("CO", [1, 2, 3, 4])
def test_pack_output_proj(CO):
    C2 = 32
    w = torch.arange(CO * C2 * 9, dtype=torch.float32).reshape(CO, C2, 3, 3)
    p = packing.pack_output_proj(w)
    assert tuple(p.shape) == (CO, 9, C2) and p.dtype == torch.float32 and p.is_contiguous()
    for co in range(CO):
        for ky in range(3):
            for kx in range(3):
                assert torch.equal(p[co, ky * 3 + kx], w[co, :, ky, kx])


def test_model_desc_carries_both_counts():
    cfg = chans_cfg(6, 3)
    assert (cfg.dd_in, cfg.in_chans) == (6, 3)
    w27 = packing.pack_input_proj(torch.arange(16 * 6 * 9, dtype=torch.float32).reshape(16, 6, 3, 3))
    assert tuple(w27.shape) == (54, 16) and w27[1 * 9 + 2 * 3 + 1, 5] == (5 * 6 + 1) * 9 + 2 * 3 + 1


def test_patch_loader_pairs_channel_counts():
    clean, noisy = torch.zeros(3, 40, 48, 3, dtype=torch.uint8), torch.zeros(3, 40, 48, 6, dtype=torch.uint8)
    ld = data.GpuPatchLoader(clean, noisy, 32)
    assert ld.hwc and (ld.N, ld.H, ld.W) == (3, 40, 48)
    ld = data.GpuPatchLoader(torch.zeros(3, 4, 40, 48), torch.zeros(3, 4, 40, 48), 32)
    assert not ld.hwc and (ld.N, ld.H, ld.W) == (3, 40, 48)
    ld = data.GpuPatchLoader(torch.zeros(2, 3, 40, 48), torch.zeros(2, 3, 40, 48), 32)     # the RGB guess is unchanged
    assert not ld.hwc
    with pytest.raises(ValueError, match="differ in shape"):
        data.GpuPatchLoader(torch.zeros(3, 4, 40, 48), torch.zeros(3, 4, 40, 50), 32)


def test_entry_points_refuse_bad_channel_counts_before_any_launch():
    """Null streams and bogus pointers: every call below has to return before it touches the device."""
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    rc = lib.uf_output_proj_c_fwd(one, 32, one, one, None, one, 1, 8, 8, 32, 5, 0, None)
    assert rc == -2 and "Cout=5" in _lib.last_error()
    rc = lib.uf_output_proj_c_fwd(one, 32, one, one, None, one, 1, 8, 8, 32, 0, 0, None)
    assert rc == -2 and "Cout=0" in _lib.last_error()
    rc = lib.uf_output_proj_c_fwd(one, 32, one, one, None, one, 1, 8, 8, 32, 4, 1, None)          # add_img without an image
    assert rc == -6 and "null" in _lib.last_error()
    rc = lib.uf_crop_augment_c(one, 1, 1, one, one, 1, 1, 0, 16, 16, 8, None)
    assert rc == -1 and "C=0" in _lib.last_error()
    rc = lib.uf_conv3x3_bwd(one, 1, one, None, 0.01, one, None, one, one, 1, 8, 8, 9, 16, one, 1 << 30, None)
    assert rc == -2 and "Cin=9" in _lib.last_error()
    rc = lib.uf_conv3x3_bwd(one, 1, one, None, 0.01, one, None, one, one, 1, 8, 8, 8, 64, one, 1 << 30, None)     # 8 x 64 x 9 = 4608 floats of weights
    assert rc == -2 and "Cin=8 Cout=64" in _lib.last_error()
    rc = lib.uf_conv3x3_bwd(one, 0, one, None, 0.01, one, None, one, one, 1, 8, 8, 32, 5, one, 1 << 30, None)
    assert rc == -2 and "Cout=5" in _lib.last_error()
    # the model descriptor: the field at fault is named
    d = _lib.ModelDesc()
    d.embed_dim = 32
    for i in range(9):
        d.depths[i] = 1
    d.blocks = ctypes.cast(one, type(d.blocks))
    ws = lib.uf_uformer_workspace_bytes(ctypes.byref(d), 1, 128, 128, 1)
    assert ws > 0
    for dd_in, in_chans, word in ((9, 3, "dd_in=9"), (0, 1, "dd_in=0"), (6, 5, "in_chans=5"), (6, 0, "in_chans=0"), (3, 4, "in_chans=4"), (3, 1, "in_chans=1")):
        d.dd_in, d.in_chans = dd_in, in_chans
        for B in (1, 8):                                                   # one stream, and the two-stream split
            rc = lib.uf_uformer_fwd(ctypes.byref(d), one, one, B, 128, 128, 1, one, 1 << 40, None)
            assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())
