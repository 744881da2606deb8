"""CPU: the embed_dim-64 model (get_arch('Uformer', embed_dim=64): head_dim 64 at every stage, C = 1024 at the bottleneck and dec0).

* spec.arch_config("tiny64") has the reference's state_dict layout and parameter count (tests/golden/hd64_spec.json, written from the
  reference by tests/golden/make_golden_hd64.py);
* oracle/uformer_oracle.py and tests/rect_composition.py reproduce the two forward fixtures in f32 -- they are the references of the GPU
  tests at other sizes;
* the oracle's autograd reproduces the reference's gradient probes (tests/golden/grad_model_tiny64_128.npz), so the oracle is
  width-general in both directions;
* get_arch('Uformer', embed_dim=64) has the reference's keys and loads a reference-layout checkpoint strictly: the plain state_dict, the
  training loop's {'epoch', 'state_dict', 'optimizer'} payload and the ``module.`` prefix of a DataParallel-wrapped model.
No GPU."""
import json
import os
from collections import OrderedDict

import torch

import rect_composition as RC
from oracle import uformer_oracle as O
from uformer_amd import checkpoint, model, spec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32_ORACLE_TOL = 2e-5          # the oracle restates the reference in f32: the bound tests/test_oracle_golden.py holds whole models to
GRAD_RTOL = 2e-4               # tests/test_oracle_golden.py's gradient bound


def spec_json():
    with open(os.path.join(GOLDEN, "hd64_spec.json")) as f:
        return json.load(f)


def kw(cfg):
    return dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in)


def test_tiny64_layout_equals_the_reference():
    j = spec_json()
    cfg = spec.arch_config("tiny64", img_size=128)
    assert cfg.embed_dim == 64 == j["embed_dim"] and list(cfg.depths) == j["depths"] == [1, 2, 2, 2, 2, 2, 2, 2, 1] and cfg.modulator
    assert all(d // h == 64 for d, h in zip(cfg.stage_dims(), cfg.num_heads))           # head_dim == embed_dim at every stage
    ref = [(k, tuple(s)) for k, s in j["state_dict"]]
    assert [(k, s) for k, s, _ in spec.state_dict_spec(cfg)] == ref
    sd = spec.synth_state_dict(cfg, 1234)
    assert sum(v.numel() for k, v in sd.items() if not k.endswith("relative_position_index")) == j["n_parameters"]


def test_get_arch_embed_dim_64_keys_and_strict_loads(tmp_path):
    j = spec_json()
    full = spec.UformerConfig(img_size=128, embed_dim=64, modulator=True)             # get_arch('Uformer'): depths [2] * 9
    m = model.get_arch("Uformer", train_ps=128, embed_dim=64)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, s) for k, s, _ in spec.state_dict_spec(full)]
    sd = spec.synth_state_dict(full, 1234)
    m.load_state_dict(sd, strict=True)
    # tiny64's layout is the reference's own (hd64_spec.json); a model of those depths loads it strictly in all three forms
    cfg = spec.arch_config("tiny64", img_size=128)
    t = model.Uformer(img_size=128, embed_dim=64, depths=list(cfg.depths), num_heads=list(cfg.num_heads), modulator=True)
    assert [(k, tuple(v.shape)) for k, v in t.state_dict().items()] == [(k, tuple(s)) for k, s in j["state_dict"]]
    sd = spec.synth_state_dict(cfg, 1234)
    t.load_state_dict(sd, strict=True)
    for name, payload in (("plain.pth", {"epoch": 3, "state_dict": sd, "optimizer": {}}),
                          ("dp.pth", {"epoch": 3, "state_dict": OrderedDict(("module." + k, v) for k, v in sd.items()), "optimizer": {}})):
        path = str(tmp_path / name)
        torch.save(payload, path)
        t2 = model.Uformer(img_size=128, embed_dim=64, depths=list(cfg.depths), num_heads=list(cfg.num_heads), modulator=True)
        checkpoint.load_checkpoint(t2, path)
        assert all(torch.equal(v, sd[k]) for k, v in t2.state_dict().items())
        assert checkpoint.load_start_epoch(path) == 3


def test_other_widths_are_still_constructible_only():
    """embed_dim 48 builds a module (the library refuses its head_dim at the first forward on the GPU: tests/test_gpu_hd64.py)."""
    m = model.get_arch("Uformer", train_ps=128, embed_dim=48)
    assert m.state_dict()["input_proj.proj.0.weight"].shape[0] == 48


def test_oracle_reproduces_the_128_fixture(golden):
    gd = golden("model_hd64_tiny64_128")
    cfg = spec.arch_config(str(gd["arch"]), img_size=int(gd["img_size"]))
    sd = spec.synth_state_dict(cfg, int(gd["seed"]))
    x = spec.synth_input(int(gd["B"]), int(gd["H"]), int(gd["W"]), int(gd["in_seed"]))
    ref = torch.from_numpy(gd["y"])
    with torch.no_grad():
        assert (O.uformer_forward(x, sd, **kw(cfg)) - ref).abs().max().item() < F32_ORACLE_TOL
        assert (RC.uformer_forward(x, sd, **kw(cfg)) - ref).abs().max().item() < F32_ORACLE_TOL


def test_rect_composition_reproduces_the_128x256_fixture(golden):
    gd = golden("model_hd64_tiny64_128x256")
    assert float(gd["pinned_to_reference_at_128"]) < F32_ORACLE_TOL
    cfg = spec.arch_config(str(gd["arch"]), img_size=int(gd["img_size"]))
    sd = spec.synth_state_dict(cfg, int(gd["seed"]))
    x = spec.synth_input(1, 128, 256, int(gd["in_seed"]))
    with torch.no_grad():
        y = RC.uformer_forward(x, sd, **kw(cfg))
    assert tuple(y.shape) == (1, 3, 128, 256)
    assert (y - torch.from_numpy(gd["y"])).abs().max().item() < F32_ORACLE_TOL


def test_oracle_autograd_reproduces_the_reference_gradients(golden):
    """The oracle is width-general: torch autograd through O.uformer_forward at embed_dim 64 against the reference's autograd probes."""
    g = golden("grad_model_tiny64_128")
    cfg = spec.arch_config("tiny64", img_size=128)
    sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in spec.synth_state_dict(cfg, 1234).items()}
    x = spec.synth_input(2, 128, 128, 1234).requires_grad_(True)
    target = spec.synth_input(2, 128, 128, 1235)
    y = O.uformer_forward(x, sd, **kw(cfg))
    loss = O.charbonnier_loss(y, target)
    loss.backward()
    assert abs(loss.item() - float(g["loss"])) < 1e-6
    assert (y.detach()[:, :, 32:96, 32:96] - torch.from_numpy(g["y_crop"])).abs().max().item() < 5e-5
    dref = torch.from_numpy(g["dx"])
    assert (x.grad - dref).abs().max().item() <= GRAD_RTOL * dref.abs().max().item()
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point()}
    # fixture_checks.check_param_grads gathers 4096 elements; this fixture stores 256-element gathers (the probe format of grad_model_tiny32_64.npz)
    from gradproj import gather_index, proj_vector
    names = [str(n) for n in g["param_names"]]
    assert sorted(names) == sorted(grads)
    for i, n in enumerate(names):
        gr = grads[n].detach()
        l2, mx = float(g["norms"][i, 0]), float(g["norms"][i, 1])
        for k in range(2):
            dev = abs(float((gr.double() * proj_vector(n, k, gr.shape).double()).sum()) - float(g["proj"][i, k])) / max(l2, 1e-30)
            assert dev <= GRAD_RTOL, (n, k, dev)
        if "full." + n in g:
            got, want = gr, torch.from_numpy(g["full." + n])
        else:
            got, want = gr.reshape(-1)[gather_index(n, gr.numel(), 256)], torch.from_numpy(g["gather." + n])
        assert (got - want).abs().max().item() <= GRAD_RTOL * max(mx, 1e-30), n
        if "block64." + n in g:
            assert (gr.reshape(gr.shape[0], -1)[:64, :64] - torch.from_numpy(g["block64." + n])).abs().max().item() <= GRAD_RTOL * max(mx, 1e-30), n
