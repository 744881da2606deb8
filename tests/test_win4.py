"""CPU: the host description of models built for 64x64 patches (img_size 64 = get_arch(..., train_ps=64): the bottleneck's window is
clamped to 4, model.py:863-866) -- per-stage windows and shifts, the reference's state_dict layout (tests/golden/win4_spec.json, written
from the reference by tests/golden/make_golden_win4.py), the (16, 16) relative_position_index, the (heads, 49) table packing, and the
errors for what is not built.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from uformer_amd import model, packing, spec
from uformer_amd._lib import UformerHipError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def spec_json():
    with open(os.path.join(GOLDEN, "win4_spec.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("img,wins,shifts3,shifts4", [
    (64, [8, 8, 8, 8, 4, 8, 8, 8, 8], [0] * 8, [0, 0]),
    (128, [8] * 9, [0, 4] * 4, [0, 0]),
    (256, [8] * 9, [0, 4] * 4, [0, 4]),
])
def test_stage_windows_and_shifts(img, wins, shifts3, shifts4):
    cfg = spec.arch_config("Uformer_B", img_size=img)
    assert cfg.stage_windows() == wins
    sh = cfg.block_shifts()
    assert sh[3] == shifts3 and sh[5] == shifts3 and sh[4] == shifts4
    assert cfg.input_multiple() == (64 if img == 64 else 128)
    assert cfg.unsupported_clamp() is None
    m = model.get_arch("Uformer_B", train_ps=img)
    assert [b.win_size for b in m.conv.blocks] == [wins[4]] * 2
    assert [b.shift_size for b in m.conv.blocks] == shifts4
    assert [b.shift_size for b in m.encoderlayer_3.blocks] == shifts3


@pytest.mark.parametrize("arch", ["Uformer_B", "Uformer_T"])
def test_state_dict_layout_equals_the_reference(arch):
    ref = [(k, tuple(s)) for k, s in spec_json()["state_dict"][arch]]
    cfg = spec.arch_config(arch, img_size=64)
    assert [(k, s) for k, s, _ in spec.state_dict_spec(cfg)] == ref
    m = model.get_arch(arch, train_ps=64)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == ref
    m.load_state_dict(spec.synth_state_dict(cfg, 1234), strict=True)         # a reference r = 64 checkpoint loads strictly


def test_synth_index_equals_the_reference_buffer():
    j = spec_json()
    assert j["conv_win_size"] == 4 and j["conv_shift_size"] == 0
    rpi = torch.tensor(j["relative_position_index_4"], dtype=torch.int64)
    assert tuple(rpi.shape) == (16, 16)
    assert torch.equal(spec.relative_position_index(4), rpi)
    sd = spec.synth_state_dict(spec.arch_config("Uformer_B", img_size=64))
    for i in range(2):
        assert torch.equal(sd[f"conv.blocks.{i}.attn.relative_position_index"], rpi)
        assert tuple(sd[f"conv.blocks.{i}.attn.relative_position_bias_table"].shape) == (49, 16)
    assert torch.equal(model.get_arch("Uformer_B", train_ps=64).conv.blocks[1].attn.relative_position_index, rpi)


def test_existing_configurations_are_unchanged():
    """8-window stages keep the (225, heads) table and the (64, 64) index; the decoders' modulator stays (64, C) at every size."""
    for img in (64, 128, 256):
        for k, shape, kind in spec.state_dict_spec(spec.arch_config("Uformer_B", img_size=img)):
            if kind == "rpb":
                assert shape[0] == (49 if (img == 64 and k.startswith("conv.")) else 225), k
            if kind == "embedding":
                assert shape[0] == 64, k


def test_rpb_table4_packing_equals_a_numpy_gather():
    heads = 5
    tab = torch.randn(49, heads, generator=torch.Generator().manual_seed(3))
    idx = spec.relative_position_index(4)
    got = packing.pack_rpb_table4(tab, idx).numpy()
    t, ix = tab.numpy(), idx.numpy()
    dense = t[ix.reshape(-1)].reshape(16, 16, heads).transpose(2, 0, 1)      # model.py:500-502
    want = np.zeros((heads, 49), np.float32)
    for i in range(16):
        for j in range(16):
            want[:, (i // 4 - j // 4 + 3) * 7 + (i % 4 - j % 4 + 3)] = dense[:, i, j]
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, t.T)                                 # the reference's index: the table transposed
    with pytest.raises(ValueError, match="Toeplitz"):
        packing.pack_rpb_table4(tab, idx.flip(0))


@pytest.mark.parametrize("img,stage,win", [(32, "encoderlayer_3", 4), (48, "encoderlayer_3", 6), (80, "conv", 5), (96, "conv", 6)])
def test_other_clamps_raise_naming_the_stage(img, stage, win):
    with pytest.raises(NotImplementedError, match=f"stage {stage} has resolution {win}.*{win}x{win} windows"):
        model.get_arch("Uformer_B", train_ps=img)


def test_input_not_a_multiple_of_64_names_the_dimension():
    m = model.get_arch("Uformer_T", train_ps=64)
    with pytest.raises(UformerHipError, match="H=96"):
        m(torch.zeros(1, 3, 96, 96))
    with pytest.raises(UformerHipError, match="W=96"):
        m(torch.zeros(1, 3, 64, 96))
    with pytest.raises(NotImplementedError, match="mask"):
        m(torch.zeros(1, 3, 64, 64), mask=torch.zeros(1, 1, 64, 64))
    with pytest.raises(UformerHipError, match="no CPU fallback"):         # a right shape reaches the usual CPU refusal
        m(torch.zeros(1, 3, 64, 128))


def test_standalone_4x4_block():
    blk = model.LeWinTransformerBlock(64, (4, 4), 2)
    assert blk.win_size == 4 and blk.shift_size == 0
    assert tuple(blk.attn.relative_position_bias_table.shape) == (49, 2)
    assert tuple(blk.attn.relative_position_index.shape) == (16, 16)
    with pytest.raises(NotImplementedError, match="modulator"):
        model.LeWinTransformerBlock(64, (4, 4), 2, modulator=True)
    with pytest.raises(NotImplementedError, match="window 6"):
        model.LeWinTransformerBlock(64, (6, 6), 2)
    x = torch.zeros(1, 16, 64)
    with pytest.raises(UformerHipError):                                      # GPU only, as every block
        blk.eval()(x)
