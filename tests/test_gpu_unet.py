"""GPU: the UNet baseline (get_arch('UNet')) on the implicit-GEMM convolutions.

* uf_conv3x3_fwd against F.conv2d in f32 for every (Cin, Cout) pair UNet(dim=32) uses, each epilogue (bias, LeakyReLU, + conv11 rows,
  input gradient), a strided destination and aux, batches 1 and 3; the 2-byte operand types on one pair; uf_conv4s2_fwd (Cout = Cin and
  Cout != Cin) and uf_conv1x1_fwd;
* whole-model forwards against the reference's outputs (tests/golden/model_unet_*.npz), f32 (measured: 1.2e-7 on all three, gate 1e-6);
* bf16 / f16 against the fp64 restatement (tests/unet_composition.py), no worse than PyTorch's autocast forward of the same dtype
  (measured at dim 32, 2 x 128 x 96: bf16 1.0e-3 against autocast's 3.3e-3, f16 1.25e-4 against 4.1e-4);
* the same with the weights scaled x2, where the bottleneck reaches the output (the test checks that it does; measured: bf16 4.3e-2
  against autocast's 7.9e-2, f16 5.5e-3 against 2.1e-2, on outputs of magnitude 5);
* f32 at dims 64 and 128 against the restatement (measured: 1.2e-7 both, gate 1e-6);
* rectangular input, batch independence (bit for bit), eval() under no_grad, infer.restore against the restatement on the
  reference's square canvas."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from unet_composition import unet_forward
from uformer_amd import _lib, infer, model, packing, spec

pytestmark = pytest.mark.gpu

DT = {torch.float32: _lib.UF_F32, torch.bfloat16: _lib.UF_BF16, torch.float16: _lib.UF_F16}
# (Cin, Cout) of every 3x3 conv of UNet(dim=32) after ConvBlock1.block.0 (which runs on uf_input_proj_fwd)
PAIRS = sorted({(32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 256),
                (256, 128), (128, 64), (64, 32)})


def g(seed):
    return torch.Generator().manual_seed(seed)


def rows(x, ld=None):
    """(B,C,H,W) -> f32 token rows (B*H*W, ld) with the channels in columns [0, C)."""
    B, C, H, W = x.shape
    r = torch.zeros(B * H * W, ld or C, device="cuda")
    r[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    return r


def unrows(r, B, H, W, C, off=0):
    return r[:, off:off + C].reshape(B, H, W, C).permute(0, 3, 1, 2)


def run_conv3x3(x, w, b, dtype, epi=1, aux=None, ld_o=None, o_off=0, out=None, accumulate=0, w_pk=None):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    xr = rows(x, Cin + 4)                       # a strided source
    wp = packing.pack_conv(w, dtype) if w_pk is None else w_pk
    ld = ld_o or Cout
    if out is None:
        out = torch.full((B * H * W, ld + o_off), 7.0, device="cuda")
    ar = rows(aux, Cout + 8) if aux is not None else None
    _lib.check(_lib.load().uf_conv3x3_fwd(xr.data_ptr(), xr.shape[1], wp.data_ptr(), b.data_ptr() if b is not None else None,
                                          ar.data_ptr() if ar is not None else None, ar.shape[1] if ar is not None else 0,
                                          out[:, o_off:].data_ptr(), out.shape[1], B, H, W, Cin, Cout, epi, accumulate, DT[dtype],
                                          torch.cuda.current_stream().cuda_stream), "uf_conv3x3_fwd")
    torch.cuda.synchronize()
    return out


def rand_conv(Cin, Cout, k, seed):
    w = (torch.randn(Cout, Cin, k, k, generator=g(seed)) * (1.0 / (Cin * k * k) ** 0.5)).cuda()
    b = (0.1 * torch.randn(Cout, generator=g(seed + 1))).cuda()
    return w, b


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_conv3x3_f32_every_pair(cin, cout):
    H, W = (12, 20) if cin <= 128 else (6, 10)
    for B in (1, 3):
        x = torch.randn(B, cin, H, W, generator=g(cin + cout + B)).cuda()
        w, b = rand_conv(cin, cout, 3, cin * 7 + cout)
        ref = F.leaky_relu(F.conv2d(x, w, b, padding=1), 0.01)
        out = run_conv3x3(x, w, b, torch.float32)
        err = (unrows(out, B, H, W, cout) - ref).abs().max().item()
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (cin, cout, B, err)


@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_epilogues_and_strided_destination(B):
    cin, cout, H, W = 64, 96, 17, 23            # partial tiles in both directions; Cout not a multiple of 64
    x = torch.randn(B, cin, H, W, generator=g(1)).cuda()
    w, b = rand_conv(cin, cout, 3, 2)
    r = torch.randn(B, cout, H, W, generator=g(3)).cuda()
    conv = F.conv2d(x, w, b, padding=1)
    # (0) bias only, into columns [32, 32 + Cout) of rows of 2 Cout + 32: the rest stays untouched
    out = run_conv3x3(x, w, b, torch.float32, epi=0, ld_o=2 * cout, o_off=32)
    assert (unrows(out, B, H, W, cout, 32) - conv).abs().max().item() < 1e-4
    assert torch.all(out[:, :32] == 7.0) and torch.all(out[:, 32 + cout:] == 7.0)
    # (b) LeakyReLU + the conv11 rows
    out = run_conv3x3(x, w, b, torch.float32, epi=2, aux=r, ld_o=2 * cout, o_off=cout)
    assert (unrows(out, B, H, W, cout, cout) - (F.leaky_relu(conv, 0.01) + r)).abs().max().item() < 1e-4
    assert torch.all(out[:, :cout] == 7.0)
    # (c) input gradient of a 3x3 conv (cout -> cin) through a LeakyReLU: dy = conv_transpose of the gradient, times LeakyReLU'(a)
    dy = torch.randn(B, cout, H, W, generator=g(4)).cuda()
    a = torch.randn(B, cin, H, W, generator=g(5)).cuda()
    w2, _ = rand_conv(cin, cout, 3, 6)          # forward: cin -> cout, so the gradient flows cout -> cin
    ref = F.conv_transpose2d(dy, w2, padding=1) * torch.where(a > 0, 1.0, 0.01)
    wt = packing.pack_conv_dgrad(w2, torch.float32)
    got = run_conv3x3(dy, torch.empty(cin, cout, 3, 3, device="cuda"), None, torch.float32, epi=3, aux=a, w_pk=wt)
    assert (unrows(got, B, H, W, cin) - ref).abs().max().item() < 1e-4
    prev = torch.randn(B * H * W, cin, generator=g(7)).cuda()
    got = run_conv3x3(dy, torch.empty(cin, cout, 3, 3, device="cuda"), None, torch.float32, epi=3, aux=a, w_pk=wt,
                      out=prev.clone(), accumulate=1)
    assert (unrows(got - prev, B, H, W, cin) - ref).abs().max().item() < 1e-4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv3x3_half_operands(dtype):
    cin, cout, B, H, W = 128, 256, 2, 16, 16
    x = torch.randn(B, cin, H, W, generator=g(11)).cuda()
    w, b = rand_conv(cin, cout, 3, 12)
    ref = F.leaky_relu(F.conv2d(x.to(dtype).float(), w.to(dtype).float(), b, padding=1), 0.01)
    out = run_conv3x3(x, w, b, dtype)
    assert (unrows(out, B, H, W, cout) - ref).abs().max().item() < 1e-3 * ref.abs().max().item()


def run_simple(fn, x, w, b, dtype, k, Ho, Wo):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    xr = rows(x)
    wp = packing.pack_conv(w, dtype)
    out = torch.full((B * Ho * Wo, Cout + 16), 7.0, device="cuda")
    _lib.check(getattr(_lib.load(), fn)(xr.data_ptr(), Cin, wp.data_ptr(), b.data_ptr(), out.data_ptr(), Cout + 16, B, H, W, Cin, Cout,
                                         DT[dtype], torch.cuda.current_stream().cuda_stream), fn)
    torch.cuda.synchronize()
    assert torch.all(out[:, Cout:] == 7.0)
    return unrows(out, B, Ho, Wo, Cout)


@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 64), (256, 256), (16, 16), (64, 32)])
@pytest.mark.parametrize("B", [1, 3])
def test_conv4s2(cin, cout, B):
    x = torch.randn(B, cin, 24, 40, generator=g(cin + B)).cuda()
    w, b = rand_conv(cin, cout, 4, cout)
    ref = F.conv2d(x, w, b, stride=2, padding=1)
    got = run_simple("uf_conv4s2_fwd", x, w, b, torch.float32, 4, 12, 20)
    assert (got - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("cin,cout", [(32, 64), (512, 256), (16, 32)])
def test_conv1x1(cin, cout):
    x = torch.randn(2, cin, 10, 14, generator=g(cin)).cuda()
    w, b = rand_conv(cin, cout, 1, cout)
    got = run_simple("uf_conv1x1_fwd", x, w, b, torch.float32, 1, 10, 14)
    assert (got - F.conv2d(x, w, b)).abs().max().item() < 2e-5 * max(1.0, got.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------------
def make(dim, dtype, seed=1234):
    m = model.UNet(dim=dim, compute_dtype=dtype).eval()
    m.load_state_dict(spec.synth_unet_state_dict(dim, seed), strict=True)
    return m.cuda()


@pytest.mark.parametrize("tag", ["d32_64", "d32_96x64", "d16_128"])
def test_model_f32_matches_reference(golden, tag):
    gd = golden("model_unet_" + tag)
    m = make(int(gd["dim"]), torch.float32, int(gd["seed"]))
    x = spec.synth_input(int(gd["B"]), int(gd["H"]), int(gd["W"]), int(gd["in_seed"])).cuda()
    with torch.no_grad():
        y = m(x)
    err = (y.cpu() - torch.from_numpy(gd["y"])).abs().max().item()
    print(f"UNet {tag} f32: max|hip - reference| = {err:.3e}")
    assert err <= 1e-6


def hot(sd, scale):
    """The synthetic weights scaled up: at scale 1 the deep levels barely reach the output (zeroing ConvBlock5 of d32 at 64x64 moves it
    by 4e-5), at scale 2 the bottleneck moves it by O(1), so an error there shows at the 2-byte types' error level."""
    return {k: (v * scale if k.endswith("weight") else v) for k, v in sd.items()}


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_model_half_no_worse_than_autocast(dtype, scale):
    dim, B, H, W = 32, 2, 128, 96
    sd = hot(spec.synth_unet_state_dict(dim, 99), scale)
    x = spec.synth_input(B, H, W, 98)
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        ref = unet_forward(x.double(), sd64).float()
        if scale > 1:   # the test must see the bottleneck: without ConvBlock5 the output moves far beyond the errors gated below
            cut = unet_forward(x.double(), {k: (torch.zeros_like(v) if k.startswith("ConvBlock5.") else v) for k, v in sd64.items()}).float()
            assert (cut - ref).abs().max().item() > 0.1
        m = model.UNet(dim=dim, compute_dtype=dtype).eval()
        m.load_state_dict(sd, strict=True)
        y = m.cuda()(x.cuda()).cpu()
        sdc = {k: v.cuda() for k, v in sd.items()}
        with torch.autocast("cuda", dtype=dtype):
            yv = unet_forward(x.cuda().contiguous(memory_format=torch.channels_last), sdc).float().cpu()
    err, err_v = (y - ref).abs().max().item(), (yv - ref).abs().max().item()
    print(f"UNet dim 32 weights x{scale} {dtype}: max|hip - fp64| = {err:.3e}, max|autocast - fp64| = {err_v:.3e}, "
          f"max|out| = {ref.abs().max().item():.3e}")
    assert err <= err_v


@pytest.mark.parametrize("dim", [64, 128])
def test_model_f32_wider_dims(dim):
    sd = spec.synth_unet_state_dict(dim, 5)
    x = spec.synth_input(1, 32, 48, 6)
    with torch.no_grad():
        ref = unet_forward(x.double(), {k: v.double() for k, v in sd.items()}).float()
        y = make(dim, torch.float32, 5)(x.cuda()).cpu()
    err = (y - ref).abs().max().item()
    print(f"UNet dim {dim} f32: max|hip - fp64| = {err:.3e}")
    assert err <= 1e-6


def test_restore_against_restatement():
    """infer.restore on an f32 model against the restatement run on the reference's square canvas (test/test_sidd.py:79-92, 106-109)."""
    m = make(16, torch.float32)
    sd = {k: v.double() for k, v in spec.synth_unet_state_dict(16, 1234).items()}
    h, w = 70, 100
    img = spec.synth_input(1, h, w, 6)
    X = 128
    canvas = torch.zeros(1, 3, X, X, dtype=torch.float64)
    y0, x0 = (X - h) // 2, (X - w) // 2
    canvas[:, :, y0:y0 + h, x0:x0 + w] = img.double()
    with torch.no_grad():
        ref = unet_forward(canvas, sd)[:, :, y0:y0 + h, x0:x0 + w].clamp(0, 1).float()
        out = infer.restore(m, img.cuda()).cpu()
    assert out.shape == img.shape
    assert (out - ref).abs().max().item() <= 1e-6


def test_rect_batch_and_grad_mode():
    m = make(16, torch.bfloat16)
    x = spec.synth_input(4, 48, 80, 5).cuda()
    with torch.no_grad():
        y = m(x)
        ys = torch.cat([m(x[i:i + 1]) for i in range(4)])
    assert y.shape == (4, 3, 48, 80) and torch.isfinite(y).all()
    assert torch.equal(y, ys)
    with torch.no_grad():
        assert m(x).grad_fn is None
    with pytest.raises(NotImplementedError):
        m.train()(x)


def test_flops_and_errors():
    m = make(16, torch.float32)
    with torch.no_grad():
        with pytest.raises(_lib.UformerHipError, match="multiples of 16"):
            m(torch.zeros(1, 3, 64, 56, device="cuda"))
    assert m.flops(256, 256) > 0
