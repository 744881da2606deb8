"""GPU: rectangular inputs (H != W) through the whole model -- the fused forward, the batch split over two streams, the autograd tape,
the mask path, restore(canvas="rect") and its pad / crop kernels, HIP-graph replay and the pipelined forward -- against the
rectangle-general CPU composition (tests/rect_composition.py) and against the transposed problem.

Gates as tests/test_gpu_model.py (outputs: f32 / f16 <= 1e-3, bf16 <= 4e-3 and >= 60 dB) and tests/test_gpu_bwd.py (gradients:
max |g - g_ref| / max |g_ref| <= 2e-3 f32, 6e-2 bf16, 1e-2 f16)."""
import json
import os

import pytest
import torch

import rect_composition as R
from oracle import uformer_oracle as O
from uformer_amd import spec

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL, BF16_PSNR = 1e-3, 4e-3, 60.0
GRAD_RTOL = {torch.float32: 2e-3, torch.bfloat16: 6e-2, torch.float16: 1e-2}
MODES = [torch.float32, torch.bfloat16, torch.float16]
TAG = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
REPORT = {}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_report():
    """the measured errors go to $UF_REPORT_DIR/parity_rect.json when that variable names a directory"""
    yield
    out = os.environ.get("UF_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_rect.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def compare(name, y, ref, dtype):
    y = y.float().cpu()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    err = (y - ref).abs().max().item()
    ps = O.psnr(y, ref)
    REPORT[name] = {"max_abs_err": err, "psnr_db": ps}
    assert torch.isfinite(y).all()
    if dtype in (torch.float32, torch.float16):
        assert err <= F32_TOL, f"{name}: {err:.3e} > {F32_TOL}"
    else:
        assert err <= BF16_TOL and ps >= BF16_PSNR, f"{name}: err {err:.3e} psnr {ps:.1f}"


def build(cfg, sd, dtype, **kw):
    from uformer_amd import model
    m = model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                      modulator=cfg.modulator, dd_in=cfg.dd_in, compute_dtype=dtype, **kw).eval()
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def composition(cfg, sd, x, mask=None):
    with torch.no_grad():
        return R.uformer_forward(x, sd, img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                                 dd_in=cfg.dd_in, mask=mask)


def tiny_ref(ctor, H, W, B=2):
    key = ("tiny32", ctor, H, W, B)
    if key not in _REF:
        cfg = spec.arch_config("tiny32", img_size=ctor)
        sd = spec.synth_state_dict(cfg, 1234)
        x = spec.synth_input(B, H, W, 4321)
        _REF[key] = (cfg, sd, x, composition(cfg, sd, x))
    return _REF[key]


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("hw", [(128, 256), (256, 128), (384, 128)])
@pytest.mark.parametrize("ctor", [128, 256])
def test_tiny_forward_vs_composition(ctor, hw, dtype):
    """ctor 256 at 128 x 256: the bottleneck is 8 x 16 with shift 4 (one window tall; 256 x 128: one window wide)."""
    cfg, sd, x, ref = tiny_ref(ctor, *hw)
    m = build(cfg, sd, dtype)
    with torch.no_grad():
        y = m(x.cuda())
    compare(f"tiny32_c{ctor}_{hw[0]}x{hw[1]}_{TAG[dtype]}", y, ref, dtype)


@pytest.mark.parametrize("dtype", MODES)
def test_uformer_B_on_a_768x1280_canvas(dtype):
    key = ("B", 768, 1280)
    if key not in _REF:
        cfg = spec.arch_config("Uformer_B", img_size=128)
        sd = spec.synth_state_dict(cfg, 99)
        x = spec.synth_input(1, 768, 1280, 98)
        _REF[key] = (cfg, sd, x, composition(cfg, sd, x))
    cfg, sd, x, ref = _REF[key]
    m = build(cfg, sd, dtype)
    with torch.no_grad():
        y = m(x.cuda())
    compare(f"B_c128_768x1280_{TAG[dtype]}", y, ref, dtype)


def test_transpose_equivariance_f32():
    """f32: uformer(x^T; weights^T)^T == uformer(x; weights) at 128 x 256 / 256 x 128 (ctor 256: a one-window-tall and a one-window-wide
    bottleneck with shift).  Needs no reference: a kernel that confuses H and W fails it."""
    cfg = spec.arch_config("tiny32", img_size=256)
    sd = spec.synth_state_dict(cfg, 1234)
    x = spec.synth_input(2, 128, 256, 55).cuda()
    with torch.no_grad():
        y = build(cfg, sd, torch.float32)(x)
        yt = build(cfg, R.transpose_state_dict(sd), torch.float32)(x.transpose(-1, -2).contiguous())
    err = (yt.transpose(-1, -2) - y).abs().max().item()
    REPORT["transpose_f32"] = err
    assert err <= 1e-5, err


def test_rect_batch_split_is_bit_identical_per_image():
    """B = 8 runs as two parts on two streams; every image equals the same image run alone, and repeated calls are bit-identical."""
    cfg = spec.arch_config("tiny32", img_size=128)
    sd = spec.synth_state_dict(cfg, 1234)
    m = build(cfg, sd, torch.bfloat16)
    x = spec.synth_input(8, 128, 384, 66).cuda()
    with torch.no_grad():
        y = m(x)
        y2 = m(x)
        torch.cuda.synchronize()
        assert torch.equal(y, y2)
        for i in range(8):
            assert torch.equal(m(x[i:i + 1]), y[i:i + 1]), i


@pytest.mark.parametrize("dtype,recompute", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True), (torch.float16, True)])
def test_autograd_vs_torch_autograd_through_the_composition(dtype, recompute):
    """eval() with parameters that require grad: the tape runs (DropPath off).  recompute=True (use_checkpoint) takes the fused block
    forward / backward of the training path; False the kept-intermediates form.  Input gradient and every parameter gradient against
    torch autograd through the CPU composition."""
    cfg = spec.arch_config("tiny32", img_size=256)
    sd = spec.synth_state_dict(cfg, 1234)
    m = build(cfg, sd, dtype, use_checkpoint=recompute)
    x = spec.synth_input(2, 128, 256, 71)
    dy = torch.randn(2, 3, 128, 256, generator=torch.Generator().manual_seed(72))
    xg = x.cuda().requires_grad_(True)
    y = m(xg)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    p = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    yr = R.uformer_forward(xr, p, img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in)
    yr.backward(dy)
    tag = f"grad_{TAG[dtype]}_{'recompute' if recompute else 'kept'}"
    compare(tag + "_y", y.detach(), yr.detach(), dtype)
    rtol = GRAD_RTOL[dtype]
    worst = {}

    def dev(got, ref):
        return (got.float().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)

    worst["x"] = dev(xg.grad, xr.grad)
    n = 0
    for name, prm in m.named_parameters():
        ref = p[name].grad
        assert prm.grad is not None, name
        worst[name] = dev(prm.grad, ref)
        n += 1
    REPORT[tag] = max(worst.values())
    assert n == len([k for k, v in sd.items() if v.is_floating_point()])
    bad = {k: v for k, v in worst.items() if not v <= rtol}
    assert not bad, (rtol, bad)


def test_mask_path_vs_composition():
    cfg = spec.arch_config("tiny32", img_size=256)
    sd = spec.synth_state_dict(cfg, 1234)
    x = spec.synth_input(1, 128, 256, 81)
    mask = (torch.rand(1, 1, 128, 256, generator=torch.Generator().manual_seed(82)) > 0.5).float()
    ref = composition(cfg, sd, x, mask)
    for dtype in MODES:
        m = build(cfg, sd, dtype)
        with torch.no_grad():
            y = m(x.cuda(), mask.cuda())
        compare(f"mask_128x256_{TAG[dtype]}", y, ref, dtype)


def test_canvas_kernels_bit_exact_vs_torch_slicing():
    from uformer_amd import ops
    g = torch.Generator().manual_seed(90)
    for (B, C, h, w, Xh, Xw) in ((2, 3, 37, 50, 64, 128), (1, 3, 720, 1280, 768, 1280), (3, 1, 128, 9, 128, 16), (1, 3, 100, 100, 256, 256)):
        img = torch.rand(B, C, h, w, generator=g) * 1.4 - 0.2
        canvas, mask = ops.expand_canvas(img.cuda(), Xh, Xw)
        ref = torch.zeros(B, C, Xh, Xw)
        rm = torch.zeros(B, 1, Xh, Xw)
        y0, x0 = (Xh - h) // 2, (Xw - w) // 2
        ref[:, :, y0:y0 + h, x0:x0 + w] = img
        rm[:, :, y0:y0 + h, x0:x0 + w] = 1
        assert torch.equal(canvas.cpu(), ref) and torch.equal(mask.cpu(), rm)
        c2, m2 = ops.expand_canvas(img.cuda(), Xh, Xw, with_mask=False)
        assert m2 is None and torch.equal(c2, canvas)
        big = (torch.rand(B, C, Xh, Xw, generator=g) * 1.4 - 0.2)
        for clamp in (False, True):
            crop = big[:, :, y0:y0 + h, x0:x0 + w]
            assert torch.equal(ops.crop_clamp_canvas(big.cuda(), h, w, clamp).cpu(), crop.clamp(0, 1) if clamp else crop)
        if Xh == Xw:   # the square entry points are the same placement
            s, sm = ops.expand2square(img.cuda(), float(Xh))
            assert torch.equal(s, canvas) and torch.equal(sm, mask)
            assert torch.equal(ops.crop_clamp(big.cuda(), h, w, True), ops.crop_clamp_canvas(big.cuda(), h, w, True))


def test_restore_rect_equals_square_where_the_canvases_coincide():
    from uformer_amd import infer
    cfg = spec.arch_config("tiny32", img_size=128)
    m = build(cfg, spec.synth_state_dict(cfg, 1234), torch.bfloat16)
    img = torch.rand(2, 3, 200, 136, generator=torch.Generator().manual_seed(91)).cuda()
    a = infer.restore(m, img)
    b = infer.restore(m, img, canvas="rect")
    assert a.shape == (2, 3, 200, 136) and torch.equal(a, b)


@pytest.mark.parametrize("dtype", MODES)
def test_restore_rect_720p_vs_composition(dtype):
    from uformer_amd import infer
    key = ("720p",)
    if key not in _REF:
        cfg = spec.arch_config("tiny32", img_size=128)
        sd = spec.synth_state_dict(cfg, 1234)
        img = torch.rand(1, 3, 720, 1280, generator=torch.Generator().manual_seed(92))
        canvas = torch.zeros(1, 3, 768, 1280)
        canvas[:, :, 24:744, :] = img
        _REF[key] = (cfg, sd, img, composition(cfg, sd, canvas)[:, :, 24:744, :].clamp(0, 1))
    cfg, sd, img, ref = _REF[key]
    m = build(cfg, sd, dtype)
    y = infer.restore(m, img.cuda(), canvas="rect")
    compare(f"restore_rect_720p_{TAG[dtype]}", y, ref, dtype)


def test_graphed_forward_replays_a_rectangular_shape():
    from uformer_amd import infer
    cfg = spec.arch_config("tiny32", img_size=128)
    m = build(cfg, spec.synth_state_dict(cfg, 1234), torch.bfloat16)
    x = spec.synth_input(2, 128, 256, 93).cuda()
    x2 = spec.synth_input(2, 128, 256, 94).cuda()
    gf = infer.GraphedForward(m, x)
    with torch.no_grad():
        e1, e2 = m(x), m(x2)
    r1 = gf(x).clone()
    r2 = gf(x2).clone()
    torch.cuda.synchronize()
    assert torch.equal(r1, e1) and torch.equal(r2, e2)


def test_pipelined_forward_on_rectangular_batches():
    from uformer_amd import infer
    cfg = spec.arch_config("tiny32", img_size=128)
    m = build(cfg, spec.synth_state_dict(cfg, 1234), torch.bfloat16)
    xs = [spec.synth_input(2, 128, 384, 95 + i).cuda() for i in range(3)] + [spec.synth_input(8, 256, 128, 98).cuda()]
    with torch.no_grad():
        eager = [m(x) for x in xs]
    outs = list(infer.PipelinedForward(m, depth=2).map(xs))
    torch.cuda.synchronize()
    assert len(outs) == len(eager)
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)


def test_width_not_a_multiple_of_128_is_an_error_naming_W():
    from uformer_amd._lib import UformerHipError
    cfg = spec.arch_config("tiny32", img_size=128)
    m = build(cfg, spec.synth_state_dict(cfg, 1234), torch.bfloat16)
    with torch.no_grad(), pytest.raises(UformerHipError, match="W=200"):
        m(torch.zeros(1, 3, 256, 200, device="cuda"))
