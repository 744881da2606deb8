"""CPU companion of tests/test_gpu_switch_matrix.py: no GPU, no library load.

* ``buildable`` against ``model.Uformer`` over the full 384-form product;
* the committed case lists against their generators, and their coverage by enumeration;
* ``reference_forward`` / ``reference_grads`` against every model-level fixture of tests/golden, at the tolerance the fixture's own CPU test uses
  (2e-5: tests/test_crossmod.py, test_ffn.py, test_convproj.py, test_chans.py, test_hd64.py's F32_ORACLE_TOL);
* gate strength: every stand-in fault a row exercises, applied to the float64 reference and cast to float32, must FAIL the row's f32 gate;
* 2-byte sanity: the reference with parameters rounded to the row's 2-byte type (arithmetic in float64) sits within half that type's gate of the
  float64 reference (bf16: half the max-abs bound AND the PSNR of half the rms error, 66.02 dB), so a 2-byte failure on the GPU is the kernel path's and not the inputs';
* the reference's run time per row, printed (budget: 20 s on 16 threads)."""
import dataclasses
import itertools
import math
import time

import pytest
import torch
import torch.nn.functional as F

import switch_matrix as SM
from gradproj import gather_index, proj_vector
from oracle import uformer_oracle as O
from uformer_amd import model, spec

FIXTURE_TOL = 2e-5
BUDGET_S = 20.0
_TIMES = {}


def t(a):
    import numpy as np
    return torch.from_numpy(np.asarray(a))


# ---- the predicate -------------------------------------------------------------------------------------------------------------------------------
def test_the_product_and_the_legal_set():
    forms = SM.all_forms()
    assert len(forms) == 384
    assert len(SM.ARCH_FORMS) == 19 and len(SM.TRAIN_FORMS) == 7        # 20 and 8 less embed_dim 64 at img_size 64 (refused: DESIGN.md 2.8)
    assert sum(SM.buildable(f) is None for f in forms) == 19 * 8
    on128 = [a for a in SM.ARCH_FORMS if a[1] == 128 and a[0] in (16, 32)]
    assert len(on128) == 16 and {a[2:] for a in on128} == set(itertools.product(("leff", "ffn"), ("lin", "conv"), ("nox", "x")))    # every triple, twice
    assert [a for a in SM.ARCH_FORMS if a[0] == 64 or a[1] == 64] == [(64, 128, "leff", "lin", "nox")] + [(e, 64, "leff", "lin", "nox") for e in (16, 32)]
    assert SM.TRAIN_FORMS == [a for a in SM.ARCH_FORMS if SM.trainable(SM.Form(*a)) is None]


def test_buildable_agrees_with_the_constructor_over_the_full_product():
    """An illegal form raises from the constructor with a message that names an option the form switches on; a legal one constructs and
    strict-loads its synthetic state dict."""
    label = {"mlp": "token_mlp", "proj": "token_projection", "cross": "cross_modulator"}
    for f in SM.all_forms():
        why = SM.buildable(f)
        if why is None:
            m = model.Uformer(**f.ctor_kwargs())
            m.load_state_dict(spec.synth_state_dict(f.cfg(), 7), strict=True)
            assert m.cfg == f.cfg(), f
            continue
        with pytest.raises((NotImplementedError, ValueError)) as ei:
            model.Uformer(**f.ctor_kwargs())
        on = [label[k] for k in SM.SWITCHES if getattr(f, k) != SM.ARCH_FACTORS[k][0]] + (["embed_dim"] if (f.e, f.img) == (64, 64) else [])
        assert why in on and any(o in str(ei.value) for o in on), (f, why, str(ei.value))


def test_training_refuses_what_trainable_refuses():
    """use_checkpoint=True is refused in the constructor for 'conv' and the cross-modulator; the kept form is refused at the first train-mode forward
    (checked on the GPU by the per-feature files): here the constructor half, over the 16 forms that build at img 128, embed_dim 16."""
    for a in SM.ARCH_FORMS:
        if a[0] != 16 or a[1] != 128:
            continue
        f = SM.Form(*a)
        if SM.trainable(f) is None:
            model.Uformer(use_checkpoint=True, **f.ctor_kwargs())
        else:
            with pytest.raises(NotImplementedError, match="use_checkpoint: (token_projection|cross_modulator)") as ei:
                model.Uformer(use_checkpoint=True, **f.ctor_kwargs())
            assert ("token_projection" in str(ei.value) and f.proj == "conv") or ("cross_modulator" in str(ei.value) and f.cross == "x")


# ---- the case lists ------------------------------------------------------------------------------------------------------------------------------
def test_case_lists_equal_the_generators_output():
    assert SM.generate_infer_rows() == SM.INFER_ROWS
    assert SM.generate_train_rows() == SM.TRAIN_ROWS
    assert len(set(SM.INFER_ROWS)) == len(SM.INFER_ROWS) and len(set(SM.TRAIN_ROWS)) == len(SM.TRAIN_ROWS)
    for n in SM.INFER_ROWS:
        assert SM.infer_name(SM.parse_infer(n)) == n
    for n in SM.TRAIN_ROWS:
        assert SM.train_name(SM.parse_train(n)) == n


def _infer_row_is_legal(r) -> bool:
    """the rules, written out on a whole row (``SM.pair_legal`` states them pair by pair)"""
    if SM.buildable(SM.form_of(r)) is not None or r["geom"] not in SM.GEOMETRIES[r["img"]]:
        return False
    return r["mask"] == "nomask" or (r["img"] == 128 and r["ex"] == "eager")


def test_inference_rows_cover_every_form_and_every_legal_pair():
    rows = [SM.parse_infer(n) for n in SM.INFER_ROWS]
    assert all(_infer_row_is_legal(r) for r in rows)
    assert {SM.form_of(r).arch() for r in rows} == set(SM.ARCH_FORMS)
    keys = SM.INFER_KEYS
    legal = set()
    # the architecture part and the run part constrain each other through img alone (geometry, mask): enumerate the legal (arch, run) halves
    arch_keys, run_keys = tuple(SM.ARCH_FACTORS), tuple(SM.RUN_FACTORS)
    for lv in itertools.product(*SM.INFER_LEVELS.values()):
        r = dict(zip(keys, lv))
        if _infer_row_is_legal(r):
            legal |= SM.row_pairs(r, keys)
    assert legal == SM.legal_pairs(SM.INFER_LEVELS)                            # the pairwise rules say what the whole-row rules say
    covered = set().union(*(SM.row_pairs(r, keys) for r in rows))
    assert covered == legal, sorted(legal - covered)[:5]
    assert arch_keys + run_keys == keys
    print(f"inference: {len(rows)} rows cover {len(SM.ARCH_FORMS)} forms and {len(legal)} legal pairs of levels")


def test_training_rows_cover_every_form_both_ways_and_every_pair_of_the_remaining_factors():
    rows = [SM.parse_train(n) for n in SM.TRAIN_ROWS]
    assert all(SM.trainable(SM.form_of(r)) is None for r in rows)
    assert {(SM.form_of(r).arch(), r["ckpt"]) for r in rows} == set(itertools.product(SM.TRAIN_FORMS, ("kept", "ckpt")))
    for a, b in zip(SM.TRAIN_ROWS[::2], SM.TRAIN_ROWS[1::2]):                 # a kept / ckpt pair: same levels, same input, same seed
        assert a.endswith("-kept") and b == a[:-5] + "-ckpt" and SM.row_seed(a) == SM.row_seed(b)
    rem = SM.TRAIN_REMAINING
    want = {(p, vp, q, vq) for p, q in itertools.combinations(rem, 2) for vp in SM.TRAIN_LEVELS[p] for vq in SM.TRAIN_LEVELS[q]}
    for ck in ("kept", "ckpt"):
        got = set().union(*(SM.row_pairs(r, rem) for r in rows if r["ckpt"] == ck))
        assert got == want, sorted(want - got)[:5]
    print(f"training: {len(rows)} rows, {len(want)} pairs of levels of {rem}")


# ---- the pieces of the reference -----------------------------------------------------------------------------------------------------------------
def test_nine_shift_depthwise_equals_conv2d_values_and_gradients():
    g = torch.Generator().manual_seed(3)
    h = torch.randn(2, 24, 16, 24, generator=g, dtype=torch.float64).permute(0, 1, 3, 2).requires_grad_(True)      # a strided view, as LeFF passes
    w = torch.randn(24, 1, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(24, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 24, 24, 16, generator=g, dtype=torch.float64)
    ga = torch.autograd.grad(SM.dwconv9(h, w, b), (h, w, b), dy)
    gb = torch.autograd.grad(F.conv2d(h, w, b, padding=1, groups=24), (h, w, b), dy)
    assert (SM.dwconv9(h, w, b) - F.conv2d(h, w, b, padding=1, groups=24)).abs().max().item() < 1e-13
    for a_, b_ in zip(ga, gb):
        assert (a_ - b_).abs().max().item() < 1e-12
    x = torch.randn(1000, generator=g, dtype=torch.float64, requires_grad=True)
    ge, = torch.autograd.grad(O.gelu_erf(x).sum(), x)
    gc, = torch.autograd.grad(SM._Gelu.apply(x).sum(), x)
    assert (ge - gc).abs().max().item() < 1e-14


def test_fast_leff_equals_the_compositions_leff_through_a_whole_model():
    name = "e16-128x64-leff-lin-nox-d6c3-mod-B1-f16-kept"
    row = SM.parse_train(name)
    sd, x, _, _ = SM.row_inputs(name, row)
    with torch.no_grad():
        a = SM.reference_forward(SM.form_of(row), sd, x, fast_dw=True)
        b = SM.reference_forward(SM.form_of(row), sd, x, fast_dw=False)
    assert (a - b).abs().max().item() < 1e-12


def test_block4_equals_the_composition_of_test_gpu_win4():
    """``block4`` against the F.layer_norm / F.linear / F.gelu composition that tests/test_gpu_win4.py holds the 4x4-window kernels to
    (``block4_ref``, restated here: that module is a GPU test), on a rectangle of 2 x 3 windows."""
    C, heads, B, H, W = 64, 4, 2, 8, 12
    cfg = spec.UformerConfig(img_size=64, embed_dim=C // 16, num_heads=(1, 1, 1, 1, heads, 1, 1, 1, 1), depths=(1,) * 9)
    pre = "conv.blocks.0."
    p = {k[len(pre):]: v.double() if v.is_floating_point() else v for k, v in spec.synth_state_dict(cfg, 5).items() if k.startswith(pre)}
    x = torch.randn(B, H * W, C, generator=torch.Generator().manual_seed(6), dtype=torch.float64)

    def part(a):
        return a.reshape(B, H // 4, 4, W // 4, 4, -1).permute(0, 1, 3, 2, 4, 5).reshape(-1, 16, a.shape[-1])

    xn = F.layer_norm(x, (C,), p["norm1.weight"], p["norm1.bias"])
    q, k, v = (part(a).reshape(-1, 16, heads, C // heads).transpose(1, 2) for a in
               (F.linear(xn, p["attn.qkv.to_q.weight"], p["attn.qkv.to_q.bias"]).reshape(B, H, W, C),
                *F.linear(xn, p["attn.qkv.to_kv.weight"], p["attn.qkv.to_kv.bias"]).reshape(B, H, W, 2 * C).split(C, -1)))
    bias = p["attn.relative_position_bias_table"][spec.relative_position_index(4).reshape(-1)].reshape(16, 16, heads).permute(2, 0, 1)
    o = (torch.softmax((q * (C // heads) ** -0.5) @ k.transpose(-2, -1) + bias, -1) @ v).transpose(1, 2).reshape(-1, 16, C)
    o = o.reshape(B, H // 4, W // 4, 4, 4, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H * W, C)
    x1 = x + F.linear(o, p["attn.proj.weight"], p["attn.proj.bias"])
    h = F.gelu(F.linear(F.layer_norm(x1, (C,), p["norm2.weight"], p["norm2.bias"]), p["mlp.linear1.0.weight"], p["mlp.linear1.0.bias"]))
    h = F.gelu(F.conv2d(h.reshape(B, H, W, 4 * C).permute(0, 3, 1, 2), p["mlp.dwconv.0.weight"], p["mlp.dwconv.0.bias"], padding=1, groups=4 * C))
    want = x1 + F.linear(h.permute(0, 2, 3, 1).reshape(B, H * W, 4 * C), p["mlp.linear2.0.weight"], p["mlp.linear2.0.bias"])
    got = SM.block4(x, p, "", heads, H, W)
    assert (got - want).abs().max().item() < 1e-12


# ---- the fixtures --------------------------------------------------------------------------------------------------------------------------------
FIXTURES = ["model_tiny_128", "model_tiny32_128", "model_win4_B_64", "model_win4_B_256", "model_win4_tiny_64", "model_win4_tiny32_64",
            "crossmod_model_tiny32_128", "crossmod_model_tiny32_128x256", "ffn_model_tiny32_128", "ffn_model_tiny32_128x256",
            "convproj_model_tiny32_128", "convproj_model_tiny32_128x256", "chans_model_tiny32_128_d1x1", "chans_model_tiny32_128_d4x3",
            "chans_model_tiny32_128_d4x4", "chans_model_tiny32_128_d6x3", "chans_model_tiny32_128x256_d6x3", "model_hd64_tiny64_128",
            "model_hd64_tiny64_128_b2", "model_hd64_tiny64_128x256"]


def fixture_cfg(g) -> spec.UformerConfig:
    cfg = spec.arch_config(str(g["arch"]), img_size=int(g["img_size"]))
    kw = {k: g[k].item() for k in ("token_mlp", "token_projection", "cross_modulator", "dd_in", "in_chans") if k in g}
    return dataclasses.replace(cfg, **kw)


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_forward_reproduces_the_fixture(golden, name):
    g = golden(name)
    cfg = fixture_cfg(g)
    H, W = (int(g["HW"]),) * 2 if "HW" in g else (int(g["H"]), int(g["W"]))
    sd = spec.synth_state_dict(cfg, int(g["seed"]))
    x = spec.synth_input(int(g["B"]), H, W, int(g["in_seed"]), channels=cfg.dd_in)
    with torch.no_grad():
        y = SM.forward_cfg(cfg, sd, x)
    err = (y.float() - t(g["y"])).abs().max().item()
    print(f"{name}: {err:.2e}")
    assert y.dtype == torch.float64 and err < FIXTURE_TOL, err


def test_reference_grads_reproduce_the_64x64_gradient_fixture(golden):
    """grad_model_tiny32_64: the reference's autograd under its Charbonnier loss at img_size 64 (two signed projections, a 256-element gather or
    the full tensor, 64x64 blocks), at tests/test_oracle_golden.py's gradient bound (2e-4, as tests/test_hd64.py holds its own)."""
    g = golden("grad_model_tiny32_64")
    form = SM.Form(32, 64)
    sd = spec.synth_state_dict(form.cfg(), 1234)
    x, target = spec.synth_input(2, 64, 64, 1234), spec.synth_input(2, 64, 64, 1235)
    y, loss, dx, grads = SM.reference_grads(form, sd, x, target)
    rtol = 2e-4
    assert abs(loss - float(g["loss"])) < 1e-6
    assert SM.grad_rel(dx, t(g["dx"])) <= rtol
    names = [str(n) for n in g["param_names"]]
    assert sorted(names) == sorted(grads)
    for i, n in enumerate(names):
        gr = grads[n].float()
        l2, mx = float(g["norms"][i, 0]), float(g["norms"][i, 1])
        for k in range(2):
            assert abs(float((gr.double() * proj_vector(n, k, gr.shape).double()).sum()) - float(g["proj"][i, k])) / max(l2, 1e-30) <= rtol, (n, k)
        got, want = (gr, t(g["full." + n])) if "full." + n in g else (gr.reshape(-1)[gather_index(n, gr.numel(), 256)], t(g["gather." + n]))
        assert (got - want).abs().max().item() <= rtol * max(mx, 1e-30), n


# ---- gate strength and bf16 sanity, row by row ---------------------------------------------------------------------------------------------------
def rounded_params(sd, dt):
    return {k: (v.to(SM.DTYPES[dt]).double() if v.is_floating_point() else v) for k, v in sd.items()}


def half_gate(dt):
    return (SM.BF16_TOL if dt == "bf16" else SM.F32_TOL) / 2


def half_gate_psnr(dt):
    """the PSNR part of the bf16 gate at half its rms error: 60 dB + 20 log10(2) = 66.02 dB; f32 and f16 have no PSNR part"""
    return SM.BF16_PSNR + 20 * math.log10(2) if dt == "bf16" else 0.0


@pytest.mark.parametrize("name", SM.INFER_ROWS)
def test_inference_row_reference_faults_and_bf16_sanity(name):
    row = SM.parse_infer(name)
    form = SM.form_of(row)
    sd, x, mask, _ = SM.row_inputs(name, row)
    n = 1 if row["B"] == 1 else 2
    t0 = time.time()
    with torch.no_grad():
        ref = SM.reference_forward(form, sd, x[:n], mask)
    dt = time.time() - t0
    print(f"{name}: reference of {n} image(s) {dt:.1f} s on {torch.get_num_threads()} threads")
    assert torch.isfinite(ref).all() and tuple(ref.shape) == (n, form.in_chans) + SM.geometry(row)
    assert torch.get_num_threads() < 16 or dt <= BUDGET_S, dt
    ok, err, ps = SM.output_gate(ref.float(), ref, torch.float32)
    assert ok and err < 1e-6                                                   # the cast alone is far inside the gate
    if n == 2:
        assert not torch.equal(ref[0], ref[1])
    with torch.no_grad():
        for fault in SM.FAULTS:
            if not SM.fault_applies(fault, form, mask is not None):
                continue
            bad = SM.reference_forward(form, sd, x[:1], mask, fault=fault)
            ok, err, _ = SM.output_gate(bad.float(), ref[:1], torch.float32)
            print(f"  fault {fault}: {err:.3e} against the f32 gate {SM.F32_TOL:.0e} ({err / SM.F32_TOL:.0f} x)")
            assert not ok, (name, fault, err)
        rb = SM.reference_forward(form, rounded_params(sd, row["dt"]), x[:1], mask)
    err = (rb - ref[:1]).abs().max().item()
    print(f"  {row['dt']}-rounded parameters: {err:.3e} (half the {row['dt']} gate: {half_gate(row['dt']):.0e}), PSNR {O.psnr(rb, ref[:1]):.1f} dB")
    assert err <= half_gate(row["dt"]) and O.psnr(rb, ref[:1]) >= half_gate_psnr(row["dt"]), (err, O.psnr(rb, ref[:1]))


@pytest.mark.parametrize("name", SM.TRAIN_ROWS[::2])
def test_training_configuration_reference_faults_and_bf16_sanity(name):
    """one reference per kept / ckpt pair (they share everything else)"""
    row = SM.parse_train(name)
    form = SM.form_of(row)
    sd, x2, _, t2 = SM.row_inputs(name, row)
    x, target = SM.batch_of(x2, row["B"]), SM.batch_of(t2, row["B"])
    t0 = time.time()
    y, loss, dx, grads = SM.reference_grads(form, sd, x, target)
    dt = time.time() - t0
    print(f"{name}: forward + autograd at B = {row['B']} {dt:.1f} s on {torch.get_num_threads()} threads, loss {loss:.4f}")
    assert torch.get_num_threads() < 16 or dt <= BUDGET_S, dt
    assert abs(loss - float(O.charbonnier_loss(y, target.double()))) < 1e-12
    assert sorted(grads) == sorted(k for k, v in sd.items() if v.is_floating_point())
    dead = [k for k, v in grads.items() if not v.abs().max().item() > 0 and not k.endswith(("norm_cross.weight", "norm_cross.bias"))]
    assert not dead, dead                                                      # every parameter reaches the loss
    for fault in SM.GRAD_FAULTS:
        if fault == "dx_image_order" and row["B"] == 1:
            continue
        bdx, bg, which = SM.faulted_grads(fault, dx, grads)
        rels = {n_: SM.grad_rel(bdx, dx) if n_ == "dx" else SM.grad_rel(bg[n_], grads[n_]) for n_ in which}
        print(f"  fault {fault}: " + ", ".join(f"{k} {v:.2f}" for k, v in rels.items()) + f" against the widest gradient gate {max(SM.GRAD_RTOL.values())}")
        assert all(v > max(SM.GRAD_RTOL.values()) for v in rels.values()), (name, fault, rels)
    with torch.no_grad():
        rb = SM.reference_forward(form, rounded_params(sd, row["dt"]), x[:1])
    err = (rb - y[:1]).abs().max().item()
    print(f"  {row['dt']}-rounded parameters: {err:.3e} (half the {row['dt']} gate: {half_gate(row['dt']):.0e})")
    assert err <= half_gate(row["dt"]) and O.psnr(rb, y[:1]) >= half_gate_psnr(row["dt"]), (err, O.psnr(rb, y[:1]))
