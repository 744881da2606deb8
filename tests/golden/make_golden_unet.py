#!/usr/bin/env python3
"""Fixtures of the UNet baseline (model.py:83-174), FROM THE REFERENCE ITSELF.

Runs only in the build container (needs the reference checkout), on the pattern of make_golden_win4.py; it reuses make_golden.py's
timm shim and helpers and runs the reference's ``UNet`` unmodified:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_unet.py

Writes
  * unet_spec.json         the reference's (key, shape) state_dict layout of UNet(dim=16) and UNet(dim=32), and their parameter counts;
  * model_unet_<tag>.npz   forward outputs on spec.synth_input with the weights of spec.synth_unet_state_dict (the tests regenerate
                           inputs and weights, neither is stored).
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the timm shim and imports the reference's model.py as mg.ref)
from uformer_amd import spec  # noqa: E402

ref = mg.ref


def ref_model(dim):
    m = ref.UNet(dim=dim).eval()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, s) for k, s, _ in spec.unet_state_dict_spec(dim)], \
        "state_dict key order/layout drifted"
    return m


def main():
    torch.set_num_threads(8)
    layout = {}
    for dim in (16, 32):
        m = ref_model(dim)
        layout[str(dim)] = {"state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                            "params": sum(p.numel() for p in m.parameters()), "flops_256": float(m.flops(256, 256))}
    path = os.path.join(HERE, "unet_spec.json")
    with open(path, "w") as f:
        json.dump(layout, f)
    print(f"unet_spec.json  {os.path.getsize(path) / 1024:.0f} KiB")

    def run_model(tag, dim, B, H, W, seed=1234, in_seed=1234):
        sd = spec.synth_unet_state_dict(dim, seed)
        m = ref_model(dim)
        m.load_state_dict(sd, strict=True)
        x = spec.synth_input(B, H, W, in_seed)
        with torch.no_grad():
            y = m(x)
        mg.save("model_unet_" + tag, y=y, dim=dim, B=B, H=H, W=W, seed=seed, in_seed=in_seed, sd_sha256=mg.sd_digest(sd))

    run_model("d32_64", 32, 2, 64, 64)
    run_model("d32_96x64", 32, 1, 96, 64)
    run_model("d16_128", 16, 1, 128, 128)


if __name__ == "__main__":
    main()
