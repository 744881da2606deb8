"""GPU: models whose image channel counts are not 3 -> 3 (``Uformer(in_chans=..., dd_in=...)``): the head kernels at 1..4 output planes and the
stem kernels at 1..8 input planes on exact integer lattices (tests/exact_lattice.py's method: every f32 sum is exact, so the comparison is
``torch.equal``), both forms of each; their backward; the C-channel patch loader; whole models against the reference's own outputs and gradients
(tests/golden/chans_*.npz, tests/golden/make_golden_chans.py).  Tolerances are the project's own, defined where the 3 -> 3 models are tested."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_cases as E
import exact_lattice as X
import rect_composition as R
from gradproj import proj_vector
from oracle import uformer_oracle as O
from oracle import uformer_oracle_bwd as OB
from test_gpu_bwd import BF16_Y_TOL, F16_LOSS_SCALE, GRAD_RTOL_BF16, GRAD_RTOL_F16, pick, rel
from test_gpu_model import BF16_PSNR, BF16_TOL, F32_TOL
from uformer_amd import spec

pytestmark = pytest.mark.gpu

MODES = [torch.float32, torch.bfloat16, torch.float16]
TAG = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
PAIRS = [(6, 3), (1, 1), (4, 4), (4, 3)]          # (dd_in, in_chans)
SHAPES = [(2, 5, 19), (1, 9, 140)]                # odd and under one tile in both forms / across a tile boundary of the second forms
PM1, PM2 = (-1, 1), (-2, -1, 1, 2)
GRAD_RTOL_F32 = 2e-4


def t(a):
    return torch.from_numpy(np.asarray(a))


def tag_of(dd_in, in_chans):
    return f"d{dd_in}x{in_chans}"


def chans_cfg(dd_in, in_chans, arch="tiny32", img_size=128):
    return dataclasses.replace(spec.arch_config(arch, img_size=img_size), dd_in=dd_in, in_chans=in_chans)


def build(cfg, sd, dtype, **kw):
    from uformer_amd import model
    m = model.Uformer(img_size=cfg.img_size, in_chans=cfg.in_chans, dd_in=cfg.dd_in, embed_dim=cfg.embed_dim, depths=list(cfg.depths),
                      num_heads=list(cfg.num_heads), modulator=cfg.modulator, compute_dtype=dtype, **kw)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def okw(cfg):
    return dict(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in)


def f32(x64):
    y = x64.float()
    assert torch.equal(y.double(), x64), "the reference is not a float32 value: the lattice bound is wrong"
    return y


def lib():
    from uformer_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------------------
# head: uf_output_proj_c_fwd, exact
# ---------------------------------------------------------------------------------------------------------------------------------------
def head_case(B, H, W, C2, Cout):
    """token rows and image on {+-1, +-2} (the image in quarters), weights on {+-1}, bias on {+-1, +-2}: |partial sums| <= 9 C2 * 2 + 2 + 2 < 2^24 quarters"""
    x = X.lattice((B, C2, H, W), PM2, 24 + C2 + W)
    w, b = X.lattice((Cout, C2, 3, 3), PM1, 25 + C2 + Cout), X.lattice((Cout,), PM2, 26 + Cout)
    img = X.lattice((B, Cout, H, W), PM2, 21 + H + Cout, k=2)
    X.check_accumulation(9 * C2, PM2, PM1, addend_steps=4 * 4)
    head = F.conv2d(x, w, b, padding=1)
    return x, w, b, img, head


@pytest.mark.parametrize("variant", [None, "head=1"], ids=["default", "first_form"])
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("C2", [16, 32, 64, 128])
@pytest.mark.parametrize("Cout", [1, 2, 3, 4])
def test_head_exact(monkeypatch, Cout, C2, B, H, W, variant):
    from uformer_amd import ops, packing
    if variant is None:
        monkeypatch.delenv("UF_VARIANT", raising=False)
    else:
        monkeypatch.setenv("UF_VARIANT", variant)
    x, w, b, img, head = head_case(B, H, W, C2, Cout)
    rows = X.to_rows(x).float().contiguous().cuda()            # (B = 1: the permuted view keeps its strides through float() and cuda())
    wp, bp = packing.pack_output_proj(w.float()).cuda(), b.float().cuda()
    got = ops.output_proj(rows, wp, bp, B, H, W)
    assert tuple(got.shape) == (B, Cout, H, W) and torch.equal(got.cpu(), f32(head))
    im = img.float().cuda()
    got = ops.output_proj(rows, wp, bp, B, H, W, img=im)
    assert torch.equal(got.cpu(), f32(head + img))
    if Cout == 3:                # the 3-plane entry point is this one's Cout = 3 case, bit for bit
        from uformer_amd import _lib
        old = torch.empty_like(got)
        _lib.check(lib().uf_output_proj_fwd(rows.data_ptr(), C2, wp.data_ptr(), bp.data_ptr(), im.data_ptr(), old.data_ptr(), B, H, W, C2, 1, stream()),
                   "uf_output_proj_fwd")
        assert torch.equal(old, got)


# ---------------------------------------------------------------------------------------------------------------------------------------
# stem: uf_input_proj_fwd, exact, first form against second form
# ---------------------------------------------------------------------------------------------------------------------------------------
STEM2_CIN = (1, 2, 3, 4, 6)       # the channel counts the LDS-staged form is built for (E 16 and 32)


def stem_case(B, H, W, Cin, Ew):
    img = X.lattice((B, Cin, H, W), PM2, 21 + H + Cin, k=2)
    w, b = X.lattice((Ew, Cin, 3, 3), PM2, 22 + Ew + Cin), X.lattice((Ew,), PM1, 23 + Ew)
    X.check_accumulation(9 * Cin, PM2, PM2, addend_steps=4)            # in steps of 1/4
    return img, w, b, X.leaky_f32(F.conv2d(img, w, b, padding=1))


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("Ew", [16, 32, 64])
@pytest.mark.parametrize("Cin", [1, 2, 4, 6, 8])
def test_stem_exact_both_forms(monkeypatch, Cin, Ew, B, H, W):
    from uformer_amd import ops, packing
    img, w, b, ref = stem_case(B, H, W, Cin, Ew)
    w27, bias, im = packing.pack_input_proj(w.float()).cuda(), b.float().cuda(), img.float().cuda()
    want = X.to_rows(ref).float()
    monkeypatch.setenv("UF_VARIANT", "stem=1")
    first = ops.input_proj(im, w27, bias)
    monkeypatch.delenv("UF_VARIANT")
    second = ops.input_proj(im, w27, bias)          # the LDS-staged form where it is built and routed, else the first form again
    assert torch.equal(first.cpu(), want)
    assert torch.equal(second.cpu(), want) and torch.equal(first, second)


@pytest.mark.parametrize("Cin", STEM2_CIN)
@pytest.mark.parametrize("Ew", [16, 32])
def test_stem_second_form_is_bit_identical_on_real_valued_input(monkeypatch, Cin, Ew):
    """Not a lattice: random f32 values, where a different order of the same products would show.  UF_VARIANT="stem=2" asks for the second form
    wherever it is built, whatever the default route is."""
    from uformer_amd import ops
    gen = torch.Generator().manual_seed(7 + Cin)
    img = torch.randn(2, Cin, 9, 140, generator=gen).cuda()
    w27, bias = torch.randn(Cin * 9, Ew, generator=gen).cuda(), torch.randn(Ew, generator=gen).cuda()
    monkeypatch.setenv("UF_VARIANT", "stem=1")
    first = ops.input_proj(img, w27, bias)
    monkeypatch.setenv("UF_VARIANT", "stem=2")
    second = ops.input_proj(img, w27, bias)
    assert torch.equal(first, second)


# ---------------------------------------------------------------------------------------------------------------------------------------
# poisoned buffers, ld larger than the width
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_head_in_a_poisoned_buffer():
    from uformer_amd import _lib, packing
    B, H, W, C2, Cout = 2, 5, 19, 32, 4
    x, w, b, img, head = head_case(B, H, W, C2, Cout)
    xin = E.PoisonedView(B * H * W, C2, mode="strided", device="cuda").fill(X.to_rows(x).float())
    out = E.PoisonedView(B * Cout * H, W, mode="guard", device="cuda")
    wp, bp, im = packing.pack_output_proj(w.float()).cuda(), b.float().cuda(), img.float().cuda()
    _lib.check(lib().uf_output_proj_c_fwd(xin.ptr(), xin.ld, wp.data_ptr(), bp.data_ptr(), im.data_ptr(), out.ptr(), B, H, W, C2, Cout, 1, stream()),
               "uf_output_proj_c_fwd")
    torch.cuda.synchronize()
    assert torch.equal(out.live().reshape(B, Cout, H, W).cpu(), f32(head + img))
    assert out.guard_intact() and xin.guard_intact()


def test_stem_in_a_poisoned_buffer():
    from uformer_amd import _lib, packing
    B, H, W, Cin, Ew = 2, 5, 19, 6, 32
    img, w, b, ref = stem_case(B, H, W, Cin, Ew)
    out = E.PoisonedView(B * H * W, Ew, mode="cat", device="cuda")             # the right half of a concat buffer, as the encoder runs
    im = E.PoisonedView(B * Cin * H, W, mode="guard", device="cuda").fill(img.float())
    w27, bias = packing.pack_input_proj(w.float()).cuda(), b.float().cuda()
    _lib.check(lib().uf_input_proj_fwd(im.ptr(), w27.data_ptr(), bias.data_ptr(), out.ptr(), out.ld, B, Cin, H, W, Ew, stream()), "uf_input_proj_fwd")
    torch.cuda.synchronize()
    assert torch.equal(out.live().cpu(), X.to_rows(ref).float())
    assert out.guard_intact() and im.guard_intact()


# ---------------------------------------------------------------------------------------------------------------------------------------
# backward of the two convolutions
# ---------------------------------------------------------------------------------------------------------------------------------------
def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("B,H,W", [(2, 8, 16), (2, 5, 19)])
@pytest.mark.parametrize("Cout", [16, 32])
@pytest.mark.parametrize("Cin", [1, 4, 6, 8])
def test_stem_backward_vs_oracle(Cin, Cout, B, H, W):
    from uformer_amd import ops
    x = torch.randn(B, Cin, H, W, generator=g(80 + Cin))
    w, b = torch.randn(Cout, Cin, 3, 3, generator=g(81)) * 0.2, torch.randn(Cout, generator=g(82)) * 0.1
    dy = torch.randn(B, Cout, H, W, generator=g(83))
    # OB.input_proj_bwd on a map that need not be square: LeakyReLU(0.01)' from the pre-activation, then the dense convolution's closed form
    pre = F.conv2d(x, w, b, padding=1)
    ref_dx, ref_dW, ref_db = OB.conv2d_bwd(x, w, dy * torch.where(pre >= 0, torch.ones_like(pre), torch.full_like(pre, 0.01)), 1, 1)
    act = X.to_rows(F.leaky_relu(pre, 0.01)).contiguous().cuda()
    dx, dW, db = ops.conv3x3_bwd(x.cuda(), X.to_rows(dy).contiguous().cuda(), w.cuda(), B, H, W, nchw=True, act_out=act, slope=0.01)
    errs = (rel(dx, ref_dx), rel(dW, ref_dW), rel(db, ref_db))
    print("stem backward", Cin, Cout, (B, H, W), errs)
    assert max(errs) < 2e-4, errs


@pytest.mark.parametrize("B,H,W", [(2, 8, 16), (2, 5, 19)])
@pytest.mark.parametrize("Cout", [1, 2, 4])
def test_head_backward_vs_oracle(Cout, B, H, W):
    from uformer_amd import ops
    Cin = 32
    x = torch.randn(B, Cin, H, W, generator=g(90 + Cout))
    w = torch.randn(Cout, Cin, 3, 3, generator=g(91)) * 0.2
    dy = torch.randn(B, Cout, H, W, generator=g(93))
    ref_dx, ref_dW, ref_db = OB.conv2d_bwd(x, w, dy, 1, 1)              # OB.output_proj_bwd on a map that need not be square
    dx, dW, db = ops.conv3x3_bwd(X.to_rows(x).contiguous().cuda(), X.to_rows(dy).contiguous().cuda(), w.cuda(), B, H, W)
    errs = (rel(dx, X.to_rows(ref_dx)), rel(dW, ref_dW), rel(db, ref_db))
    print("head backward", Cout, (B, H, W), errs)
    assert max(errs) < 2e-4, errs


@pytest.mark.parametrize("Cin", [32, 64])
@pytest.mark.parametrize("Cout", [1, 2, 3, 4])
def test_dx_walk_against_the_generic_dx_kernel(Cout, Cin):
    """W a multiple of 16 and a 16-byte aligned dx take conv3x3_dx_walk_kernel<Cout, 16>; the same call with dx moved by one float takes the generic
    kernel.  Both compute fmaf chains over the same 9 Cout products per element in different orders."""
    from uformer_amd import _lib
    B, H, W = 2, 8, 32
    n = B * H * W
    rows, dy = torch.randn(n, Cin, generator=g(70)).cuda(), torch.randn(n, Cout, generator=g(71)).cuda()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g(72)) * 0.2).cuda()
    L = lib()
    nb = L.uf_conv3x3_bwd_workspace_bytes(B, H, W, Cin, Cout)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dW, db = torch.empty_like(w), torch.empty(Cout, device="cuda")
    buf = torch.zeros(n * Cin + 4, device="cuda")
    out = []
    for off in (0, 1):
        dx = buf[off:off + n * Cin]
        assert (dx.data_ptr() % 16 == 0) == (off == 0)
        _lib.check(L.uf_conv3x3_bwd(rows.data_ptr(), 0, dy.data_ptr(), None, 0.01, w.data_ptr(), dx.data_ptr(), dW.data_ptr(), db.data_ptr(), B, H, W, Cin, Cout,
                                    ws.data_ptr(), nb, stream()), "uf_conv3x3_bwd")
        out.append(dx.clone())
    err = rel(out[0], out[1].cpu())
    print("dx walk vs generic", Cout, Cin, err)
    assert err < 2e-6, err


# ---------------------------------------------------------------------------------------------------------------------------------------
# patch loader
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 4, 6])
def test_crop_augment_c_channels(C):
    from uformer_amd import data, ops
    N, H, W, ps = 3, 40, 56, 24
    u8_hwc = torch.randint(0, 256, (N, H, W, C), generator=g(3 + C), dtype=torch.uint8)
    f_chw = (u8_hwc.float() / 255.0).permute(0, 3, 1, 2).contiguous()
    meta = torch.tensor([[i % N, (7 * i) % (H - ps), (11 * i) % (W - ps), i % 8] for i in range(16)], dtype=torch.int32)     # all eight transforms, twice
    ref = torch.stack([O.crop_augment(f_chw[i], r, c, ps, k) for i, r, c, k in meta.tolist()])
    m = meta.cuda()
    assert torch.equal(ops.crop_augment(u8_hwc.cuda(), m, ps, hwc=True).cpu(), ref)
    assert torch.equal(ops.crop_augment(u8_hwc.permute(0, 3, 1, 2).contiguous().cuda(), m, ps, hwc=False).cpu(), ref)
    assert torch.equal(ops.crop_augment(f_chw.cuda(), m, ps, hwc=False).cpu(), ref)
    assert torch.equal(ops.crop_augment(f_chw.permute(0, 2, 3, 1).contiguous().cuda(), m, ps, hwc=True).cpu(), ref)
    rgb = torch.randint(0, 256, (N, H, W, 3), generator=g(9), dtype=torch.uint8)
    target, inp = data.GpuPatchLoader(rgb.cuda(), u8_hwc.cuda(), ps).batch(8)          # a target of 3 planes beside an input of C
    assert tuple(target.shape) == (8, 3, ps, ps) and tuple(inp.shape) == (8, C, ps, ps)


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole models, forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def compare(name, y, ref, dtype):
    """tests/test_gpu_model.py's ``compare``"""
    y = y.float().cpu()
    err = (y - ref).abs().max().item()
    ps = O.psnr(y, ref)
    print(f"{name}: max abs err {err:.3e}, PSNR {ps:.1f} dB")
    assert torch.isfinite(y).all()
    if dtype in (torch.float32, torch.float16):
        assert err <= F32_TOL, f"{name}: {err:.3e} > {F32_TOL}"
    else:
        assert err <= BF16_TOL and ps >= BF16_PSNR, f"{name}: err {err:.3e} psnr {ps:.1f}"


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("dd_in,in_chans", PAIRS)
def test_model_forward_vs_reference(golden, dd_in, in_chans, dtype):
    gd = golden("chans_model_tiny32_128_" + tag_of(dd_in, in_chans))
    cfg = chans_cfg(dd_in, in_chans)
    m = build(cfg, spec.synth_state_dict(cfg, int(gd["seed"])), dtype).eval()
    x = spec.synth_input(int(gd["B"]), 128, 128, int(gd["in_seed"]), channels=dd_in).cuda()
    with torch.no_grad():
        y = m(x)
    assert tuple(y.shape) == (2, in_chans, 128, 128)
    compare(f"chans_{tag_of(dd_in, in_chans)}_{TAG[dtype]}", y, t(gd["y"]), dtype)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_model_forward_rect(golden, dtype):
    gd = golden("chans_model_tiny32_128x256_d6x3")
    cfg = chans_cfg(6, 3)
    m = build(cfg, spec.synth_state_dict(cfg, int(gd["seed"])), dtype).eval()
    with torch.no_grad():
        y = m(spec.synth_input(1, 128, 256, int(gd["in_seed"]), channels=6).cuda())
    compare(f"chans_d6x3_128x256_{TAG[dtype]}", y, t(gd["y"]), dtype)


@pytest.mark.parametrize("dd_in,in_chans", [(6, 3), (4, 4)])
def test_graphed_and_pipelined_forward_are_bit_identical(dd_in, in_chans):
    from uformer_amd import infer
    cfg = chans_cfg(dd_in, in_chans)
    m = build(cfg, spec.synth_state_dict(cfg, 1234), torch.bfloat16).eval()
    x = spec.synth_input(2, 128, 128, 1234, channels=dd_in).cuda()
    with torch.no_grad():
        y = m(x)
    gf = infer.GraphedForward(m, x)
    assert torch.equal(gf(x), y)
    pf = infer.PipelinedForward(m, depth=2)
    outs = list(pf.map([x, x.flip(0), x]))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], y) and torch.equal(outs[2], y) and torch.equal(outs[1], y.flip(0))
    # eight images: the library cuts the batch over two streams, whose output offsets use in_chans
    x8 = torch.cat([x, x.flip(0), x, x.flip(0)])
    with torch.no_grad():
        y8 = m(x8)
    assert torch.equal(y8, torch.cat([y, y.flip(0), y, y.flip(0)]))


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_mask_argument_on_the_6_to_3_model(dtype):
    cfg = chans_cfg(6, 3)
    sd = spec.synth_state_dict(cfg, 1234)
    x = spec.synth_input(1, 128, 128, 77, channels=6)
    mask = (torch.rand(1, 1, 128, 128, generator=g(78)) > 0.7).float()
    with torch.no_grad():
        ref = R.uformer_forward(x, sd, mask=mask, **okw(cfg))
        y = build(cfg, sd, dtype).eval()(x.cuda(), mask=mask.cuda())
    compare(f"chans_d6x3_mask_{TAG[dtype]}", y, ref, dtype)


@pytest.mark.parametrize("variant", ["ffn", "conv", "cross", "embed64"])
def test_block_variants_combine_with_the_channel_counts(variant):
    """The stem and the head are independent of the blocks: token_mlp='ffn', token_projection='conv', cross_modulator=True and embed_dim 64 (the stem's
    first form at E = 64, the head at C2 = 128) on a 6 -> 3 and a 4 -> 4 model, f32, against the CPU compositions the 3 -> 3 variants are tested with."""
    import convproj_composition as CC
    import crossmod_composition as XC
    import ffn_composition as FC
    dd_in, in_chans = (4, 4) if variant in ("conv", "embed64") else (6, 3)
    base = chans_cfg(dd_in, in_chans, arch="tiny64" if variant == "embed64" else "tiny32")
    cfg, fwd = {"ffn": (dataclasses.replace(base, token_mlp="ffn"), FC.uformer_forward), "conv": (dataclasses.replace(base, token_projection="conv"), CC.uformer_forward),
                "cross": (dataclasses.replace(base, cross_modulator=True), XC.uformer_forward), "embed64": (base, O.uformer_forward)}[variant]
    sd = spec.synth_state_dict(cfg, 1234)
    x = spec.synth_input(1, 128, 128, 91, channels=dd_in)
    m = build(cfg, sd, torch.float32, token_mlp=cfg.token_mlp, token_projection=cfg.token_projection, cross_modulator=cfg.cross_modulator).eval()
    with torch.no_grad():
        ref = fwd(x, sd, **okw(cfg))
        y = m(x.cuda())
    assert tuple(y.shape) == (1, in_chans, 128, 128)
    compare(f"chans_{variant}_{tag_of(dd_in, in_chans)}_f32", y, ref, torch.float32)


@pytest.mark.parametrize("canvas", ["square", "rect"])
def test_restore_4_to_4_on_a_100x70_input(canvas):
    from uformer_amd import infer
    cfg = chans_cfg(4, 4)
    sd = spec.synth_state_dict(cfg, 1234)
    img = spec.synth_input(1, 100, 70, 55, channels=4)
    padded = torch.zeros(1, 4, 128, 128)                     # both canvases are 128 x 128 here; the image is centred on each axis
    padded[:, :, 14:114, 29:99] = img
    with torch.no_grad():
        ref = O.uformer_forward(padded, sd, **okw(cfg))[:, :, 14:114, 29:99].clamp(0, 1)
        got = infer.restore(build(cfg, sd, torch.float32).eval(), img.cuda(), canvas=canvas)
    assert tuple(got.shape) == (1, 4, 100, 70)
    err = (got.cpu() - ref).abs().max().item()
    print("restore 4->4", canvas, err)
    assert err <= F32_TOL


def test_restore_tiled_allocates_in_chans_planes():
    from uformer_amd import infer
    cfg = chans_cfg(6, 3)
    m = build(cfg, spec.synth_state_dict(cfg, 1234), torch.bfloat16).eval()
    img = spec.synth_input(1, 128, 200, 56, channels=6).cuda()
    out = infer.restore_tiled(m, img, tile=128, min_overlap=32)
    assert tuple(out.shape) == (1, 3, 128, 200) and torch.isfinite(out).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole models, training
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_grads(gd, name, loss, y, dx, grads, dtype):
    """loss, restored images, d loss / d input (centre crop and pooled map) and every parameter gradient of a chans_grad fixture: two signed random
    projections per parameter (tolerance rtol * ||g_ref||_2, tests/fixture_checks.py's rule) and the tensors stored in full (rtol * max |g_ref|)."""
    rtol = pick(dtype, GRAD_RTOL_F32, GRAD_RTOL_BF16, GRAD_RTOL_F16)
    y_tol = BF16_Y_TOL if dtype == torch.bfloat16 else 1e-3
    worst = {"loss": abs(loss - float(gd["loss"])), "y": (y.float().cpu() - t(gd["y"])).abs().max().item()}
    dx = dx.float().cpu()
    dmax = float(gd["dx_absmax"])
    worst["dx_crop"] = (dx[:, :, 32:96, 32:96] - t(gd["dx_crop"])).abs().max().item() / dmax
    worst["dx_pooled"] = (F.avg_pool2d(dx, 16) - t(gd["dx_pooled16"])).abs().max().item() / max(t(gd["dx_pooled16"]).abs().max().item(), dmax / 16)
    names = [str(n) for n in gd["param_names"]]
    assert sorted(names) == sorted(grads), "parameter set differs from the reference's named_parameters()"
    worst["proj"], worst["full"] = (0.0, ""), (0.0, "")
    for i, n in enumerate(names):
        l2, mx = float(gd["norms"][i, 0]), float(gd["norms"][i, 1])
        gr = grads[n]
        assert gr is not None or l2 == 0.0, n
        if gr is None:
            continue
        gr = gr.detach().float().cpu()
        for k in range(2):
            dev = abs(float((gr.double() * proj_vector(n, k, gr.shape).double()).sum()) - float(gd["proj"][i, k])) / max(l2, 1e-30)
            worst["proj"] = max(worst["proj"], (dev, n))
        if "full." + n in gd:
            worst["full"] = max(worst["full"], ((gr - t(gd["full." + n])).abs().max().item() / max(mx, 1e-30), n))
    print(f"{name}: {worst}")
    assert worst["loss"] <= pick(dtype, 1e-5, 2e-3) and worst["y"] <= y_tol, worst
    assert worst["dx_crop"] <= rtol and worst["dx_pooled"] <= rtol, worst
    assert worst["proj"][0] <= rtol and worst["full"][0] <= rtol, worst
    return worst


def grad_setup(golden, dd_in, in_chans):
    gd = golden("chans_grad_tiny_128_" + tag_of(dd_in, in_chans))
    cfg = chans_cfg(dd_in, in_chans, arch="tiny")
    sd = spec.synth_state_dict(cfg, int(gd["seed"]))
    x = spec.synth_input(2, 128, 128, int(gd["in_seed"]), channels=dd_in).cuda()
    target = spec.synth_input(2, 128, 128, int(gd["target_seed"]), channels=in_chans).cuda()
    dref = t(gd["y"]).cuda() - target
    dy_ref = dref / torch.sqrt(dref * dref + 1e-6) / dref.numel()           # CharbonnierLoss' gradient at the REFERENCE's output (sign-like: it must not
    return gd, cfg, sd, x, target, dy_ref                                   # inherit the forward error of the path under test, tests/test_gpu_bwd.py)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("recompute", [False, True], ids=["kept", "recompute"])
@pytest.mark.parametrize("dd_in,in_chans", [(6, 3), (4, 4)])
def test_tape_vs_reference_autograd(golden, dd_in, in_chans, recompute, dtype):
    import warnings
    from uformer_amd import train
    gd, cfg, sd, x, target, dy_ref = grad_setup(golden, dd_in, in_chans)
    sd = {k: v.cuda() for k, v in sd.items()}
    ls = F16_LOSS_SCALE if dtype == torch.float16 else 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # 'tiny' is head_dim 16: the recompute form says that every block keeps its intermediates
        y, dimg, grads = train.uformer_forward_backward(x, sd, dy_ref, cfg=cfg, dtype=dtype, drop_scales=t(gd["masks"]).cuda(), recompute=recompute, loss_scale=ls)
    assert tuple(y.shape) == (2, in_chans, 128, 128) and tuple(dimg.shape) == (2, dd_in, 128, 128)
    d = y - target
    loss = torch.mean(torch.sqrt(d * d + 1e-6)).item()
    check_grads(gd, f"tape_{tag_of(dd_in, in_chans)}_{'recompute' if recompute else 'kept'}_{TAG[dtype]}", loss, y, dimg, grads, dtype)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("dd_in,in_chans", [(6, 3), (4, 4)])
def test_module_autograd_vs_reference_autograd(golden, dd_in, in_chans, dtype):
    gd, cfg, sd, x, target, dy_ref = grad_setup(golden, dd_in, in_chans)
    m = build(cfg, sd, dtype, drop_path_rate=0.3).train()
    assert np.allclose(m.drop_path_rates(), list(gd["drop_rates"]), atol=1e-6)
    m._drop_scales_override = t(gd["masks"]).cuda()
    x = x.requires_grad_(True)
    y = m(x)
    d = y - target
    loss = torch.mean(torch.sqrt(d * d + 1e-6))
    ls = F16_LOSS_SCALE if dtype == torch.float16 else 1.0
    if dtype != torch.float32:
        y.backward(dy_ref * ls)
    else:
        loss.backward()
    grads = {n: (None if p_.grad is None else p_.grad / ls) for n, p_ in m.named_parameters()}
    check_grads(gd, f"module_{tag_of(dd_in, in_chans)}_{TAG[dtype]}", loss.item(), y.detach(), x.grad / ls, grads, dtype)
    # no input gradient is computed unless the caller asks for it
    m.zero_grad()
    y2 = m(x.detach())
    y2.backward(dy_ref * ls)
    assert torch.equal(y2, y) and m.input_proj.proj[0].weight.grad is not None


@pytest.mark.parametrize("dd_in,in_chans", [(6, 3), (4, 4)])
def test_use_checkpoint_equals_the_plain_path(golden, dd_in, in_chans):
    """As tests/test_gpu_bwd.py::test_use_checkpoint_takes_the_recompute_form asserts it: the recompute form is taken, and its gradients are those of the
    kept-intermediates form of the same model on the same DropPath masks to bf16 rounding."""
    import warnings
    from uformer_amd import train
    gd, cfg, sd, x, target, dy_ref = grad_setup(golden, dd_in, in_chans)
    grads = {}
    for ckpt in (False, True):
        m = build(cfg, sd, torch.bfloat16, drop_path_rate=0.3, use_checkpoint=ckpt).train()
        m._drop_scales_override = t(gd["masks"]).cuda()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            d = m(x) - target
            torch.mean(torch.sqrt(d * d + 1e-6)).backward()
        assert train.UformerFunction.last_recompute is ckpt
        grads[ckpt] = {n: p_.grad.float().cpu() for n, p_ in m.named_parameters() if p_.grad is not None}
    assert grads[True].keys() == grads[False].keys()
    worst = max((rel(grads[True][n].cuda(), grads[False][n]), n) for n in grads[True] if grads[False][n].abs().max() > 0)
    print("use_checkpoint vs plain", worst)
    assert worst[0] < 6e-2, worst
