"""CPU: the UNet baseline's Python surface (get_arch('UNet'), state_dict layout, checkpoint loading, input checks) and the fp32
restatement tests/unet_composition.py pinned to the reference's outputs (tests/golden/model_unet_*.npz)."""
import json
import os

import numpy as np
import pytest
import torch

from unet_composition import unet_forward
from uformer_amd import model, spec
from uformer_amd._lib import UformerHipError

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _spec():
    with open(os.path.join(GOLD, "unet_spec.json")) as f:
        return json.load(f)


def test_get_arch_unet_constructs():
    m = model.get_arch("UNet")
    assert isinstance(m, model.UNet) and m.dim == 32
    assert model.get_arch("UNet", embed_dim=16).dim == 16


@pytest.mark.parametrize("dim", [16, 32])
def test_state_dict_matches_reference_layout(dim):
    ref = _spec()[str(dim)]
    m = model.UNet(dim=dim)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == ref["state_dict"]
    assert sum(p.numel() for p in m.parameters()) == ref["params"]
    assert [[k, list(s)] for k, s, _ in spec.unet_state_dict_spec(dim)] == ref["state_dict"]
    assert m.flops(256, 256) == ref["flops_256"]


def test_dim32_counts():
    m = model.get_arch("UNet", embed_dim=32)
    assert len(m.state_dict()) == 72
    assert sum(p.numel() for p in m.parameters()) == 9503779


@pytest.mark.parametrize("tag", ["d32_64", "d32_96x64", "d16_128"])
def test_restatement_matches_reference(tag):
    g = np.load(os.path.join(GOLD, f"model_unet_{tag}.npz"))
    sd = spec.synth_unet_state_dict(int(g["dim"]), int(g["seed"]))
    x = spec.synth_input(int(g["B"]), int(g["H"]), int(g["W"]), int(g["in_seed"]))
    with torch.no_grad():
        y = unet_forward(x, sd)
    assert y.shape == g["y"].shape
    assert (y - torch.from_numpy(g["y"])).abs().max().item() <= 1e-5


def test_reference_checkpoints_load_strictly():
    sd = spec.synth_unet_state_dict(16, 7)
    for payload in (sd, {"epoch": 3, "state_dict": sd, "optimizer": {}}, {"module." + k: v for k, v in sd.items()},
                    {"epoch": 3, "state_dict": {"module." + k: v for k, v in sd.items()}}):
        m = model.UNet(dim=16)
        m.load_state_dict(payload, strict=True)
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), k


def test_inputs_are_checked():
    m = model.UNet(dim=16).eval()
    with torch.no_grad():
        with pytest.raises(UformerHipError, match="no CPU fallback"):
            m(torch.zeros(1, 3, 64, 64))
        for H, W in ((64, 72), (40, 64), (0, 64)):
            with pytest.raises(UformerHipError, match="multiples of 16"):
                m(torch.zeros(1, 3, H, W))
        with pytest.raises(UformerHipError, match="B,3,H,W"):
            m(torch.zeros(1, 4, 64, 64))


def test_unsupported_options_raise():
    for dim in (8, 48, 256):
        with pytest.raises(ValueError, match="16, 32, 64 or 128"):
            model.UNet(dim=dim)
    with pytest.raises(NotImplementedError, match="stride"):
        model.ConvBlock(8, 16, strides=2)
    with pytest.raises(Exception, match="Arch error"):
        model.get_arch("Uformer_B_fastleff")
