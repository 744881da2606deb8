"""GPU: models built for 64x64 patches (img_size 64 = get_arch(..., train_ps=64)), whose bottleneck runs on 4x4 windows.

* the 4x4-window kernels (uf_window4_attention_fwd / _bwd, uf_rpb4_table_grad, uf_window4_partition / _reverse) against a torch
  composition of the same ops, in f32 / bf16 / f16, head_dim 16 and 32, one window and many;
* a standalone LeWinTransformerBlock(dim, (4, 4), heads): inference and autograd against torch autograd through the composition;
* whole-model forwards against the reference's outputs (tests/golden/model_win4_*.npz; gates of tests/test_gpu_model.py), all parameter
  gradients of tiny32 against the reference's autograd (tests/golden/grad_model_tiny32_64.npz; tolerances of tests/test_gpu_bwd.py), in
  the kept form and with use_checkpoint=True;
* a rectangular 64 x 192 input (inference == autograd forward, batch split bit-identical, the 192 x 64 transpose), and one AdamW step at
  train_ps 64, batch 32, bf16."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gradproj import gather_index, proj_vector
from oracle import uformer_oracle as O
from uformer_amd import model, ops, packing, spec

pytestmark = pytest.mark.gpu

MODES = [torch.float32, torch.bfloat16, torch.float16]
TAG = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
KTOL = {torch.float32: 2e-4, torch.bfloat16: 2.5e-2, torch.float16: 2.5e-2 / 4}     # kernel tolerances of tests/test_gpu_bwd.py
F32_TOL, BF16_TOL, BF16_PSNR = 1e-3, 4e-3, 60.0                                      # whole-model gates of tests/test_gpu_model.py
GRAD_RTOL = {torch.float32: 2e-3, torch.bfloat16: 6e-2, torch.float16: 1e-2}        # whole-model gradient gates of tests/test_gpu_bwd.py
F16_LOSS_SCALE = 65536.0


def g(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().max().item() / max(1e-12, b.float().abs().max().item())


# ------------------------------------------------------------------------------------------------------------------------
# torch composition of a 4x4-window block (model.py:452-546, :908-989 at win 4, shift 0, no modulator)
# ------------------------------------------------------------------------------------------------------------------------
def partition4(x, B, H, W):
    """raster rows (B*H*W, C) -> window rows (B*nW, 16, C), model.py:704-715"""
    C = x.shape[-1]
    return x.reshape(B, H // 4, 4, W // 4, 4, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 16, C)


def reverse4(w, B, H, W):
    C = w.shape[-1]
    return w.reshape(B, H // 4, W // 4, 4, 4, C).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, C)


def attn4_ref(qkv, table, B, H, W, heads):
    C = qkv.shape[1] // 3
    hd = C // heads
    win = partition4(qkv, B, H, W)
    q, k, v = (win[..., i * C:(i + 1) * C].reshape(-1, 16, heads, hd).transpose(1, 2) for i in range(3))
    bias = table[spec.relative_position_index(4).reshape(-1).to(table.device)].reshape(16, 16, heads).permute(2, 0, 1)
    a = torch.softmax((q * hd ** -0.5) @ k.transpose(-2, -1) + bias.unsqueeze(0), -1)
    return reverse4((a @ v).transpose(1, 2).reshape(-1, 16, C), B, H, W)


def block4_ref(x, p, heads, H, W):
    B, L, C = x.shape
    xn = F.layer_norm(x, (C,), p["norm1.weight"], p["norm1.bias"])
    qkv = torch.cat([F.linear(xn, p["attn.qkv.to_q.weight"], p["attn.qkv.to_q.bias"]), F.linear(xn, p["attn.qkv.to_kv.weight"], p["attn.qkv.to_kv.bias"])], -1)
    o = attn4_ref(qkv.reshape(B * L, 3 * C), p["attn.relative_position_bias_table"], B, H, W, heads)
    x1 = x + F.linear(o, p["attn.proj.weight"], p["attn.proj.bias"]).reshape(B, L, C)
    h = F.gelu(F.linear(F.layer_norm(x1, (C,), p["norm2.weight"], p["norm2.bias"]), p["mlp.linear1.0.weight"], p["mlp.linear1.0.bias"]))
    h = h.reshape(B, H, W, 4 * C).permute(0, 3, 1, 2)
    h = F.gelu(F.conv2d(h, p["mlp.dwconv.0.weight"], p["mlp.dwconv.0.bias"], padding=1, groups=4 * C))
    return x1 + F.linear(h.permute(0, 2, 3, 1).reshape(B, L, 4 * C), p["mlp.linear2.0.weight"], p["mlp.linear2.0.bias"])


SHAPES = [(1, 4, 4), (2, 8, 12), (3, 16, 16)]               # one window; 12 windows of a rectangle; 48
HEADS = [(64, 2), (96, 6), (512, 16)]                       # head_dim 32; head_dim 16 with a partial group of heads; the Uformer-B bottleneck


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("C,heads", HEADS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_window4_attention_forward_and_backward_vs_torch(dtype, C, heads, B, H, W):
    M = B * H * W
    qkv = (torch.randn(M, 3 * C, generator=g(1)) * 0.7).to(dtype)
    table = torch.randn(49, heads, generator=g(2)) * 0.5
    do = torch.randn(M, C, generator=g(3)).to(dtype)
    tab4 = packing.pack_rpb_table4(table, spec.relative_position_index(4)).cuda()
    o = ops.window4_attention(qkv.cuda(), tab4, B, H, W, heads)
    dqkv, dscore = ops.window4_attention_bwd(qkv.cuda(), tab4, do.cuda(), B, H, W, heads)
    dtab = ops.rpb4_table_grad(dscore)
    qf = qkv.float().requires_grad_(True)
    tf = table.clone().requires_grad_(True)
    ref = attn4_ref(qf, tf, B, H, W, heads)
    ref.backward(do.float())
    assert o.dtype == dtype and dqkv.dtype == dtype
    assert rel(o, ref.detach()) < KTOL[dtype]
    assert rel(dqkv, qf.grad) < KTOL[dtype]
    assert rel(dtab, tf.grad) < KTOL[dtype]
    assert torch.equal(ops.rpb4_table_grad(dscore), dtab)                   # fixed-order sums: deterministic


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_window4_partition_and_reverse_bit_exact(dtype, B, H, W):
    x = torch.randn(B, H, W, 24, generator=g(4)).to(dtype)
    want = partition4(x.reshape(-1, 24), B, H, W).reshape(-1, 4, 4, 24)
    got = model.window_partition(x.cuda(), 4)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(model.window_reverse(got, 4, H, W).cpu(), x)


def randomized_block(C, heads, seed):
    blk = model.LeWinTransformerBlock(C, (4, 4), heads)
    gg = g(seed)
    with torch.no_grad():
        for n, p_ in blk.named_parameters():
            r = torch.randn(p_.shape, generator=gg)
            p_.copy_(1 + 0.1 * r if n.endswith("norm1.weight") or n.endswith("norm2.weight") else
                     (0.3 * r if "relative_position" in n else (0.1 * r if n.endswith("bias") else r / max(1, p_[0].numel()) ** 0.5)))
    return blk


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("C,heads", [(64, 2), (256, 16)])
def test_standalone_block_inference_and_autograd_vs_torch(dtype, C, heads):
    B, H, W = 2, 8, 12
    blk = randomized_block(C, heads, 5 + C)
    p = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in blk.state_dict().items()}
    x = torch.randn(B, H * W, C, generator=g(6))
    gy = torch.randn(B, H * W, C, generator=g(7))
    xr = x.clone().requires_grad_(True)
    ref = block4_ref(xr, p, heads, H, W)
    ref.backward(gy)
    blk = blk.cuda().eval()
    tol = {torch.float32: 1e-4, torch.bfloat16: 2.5e-2, torch.float16: 2.5e-2 / 4}[dtype]
    with torch.no_grad():
        y_inf = blk(x.cuda(), compute_dtype=dtype, hw=(H, W))
    assert rel(y_inf - x.cuda(), (ref - x).detach()) < tol
    xg = x.cuda().requires_grad_(True)
    y = blk(xg, compute_dtype=dtype, hw=(H, W))
    assert y.grad_fn is not None
    assert rel(y - xg, (ref - x).detach()) < tol
    y.backward(gy.cuda())
    gtol = {torch.float32: 2e-3, torch.bfloat16: 6e-2, torch.float16: 1e-2}[dtype]
    assert rel(xg.grad, xr.grad) < gtol
    for n, p_ in blk.named_parameters():
        assert p_.grad is not None, n
        assert rel(p_.grad, p[n].grad) < gtol, (n, rel(p_.grad, p[n].grad))


# ------------------------------------------------------------------------------------------------------------------------
# whole models
# ------------------------------------------------------------------------------------------------------------------------
def build(arch, dtype, seed=1234, **kw):
    cfg = spec.arch_config(arch, img_size=64)
    m = model.Uformer(img_size=64, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), modulator=cfg.modulator,
                      dd_in=cfg.dd_in, compute_dtype=dtype, **kw).eval()
    m.load_state_dict(spec.synth_state_dict(cfg, seed), strict=True)
    return m.cuda()


def compare(name, y, ref, dtype):
    y = y.float().cpu()
    assert y.shape == ref.shape and torch.isfinite(y).all()
    err = (y - ref).abs().max().item()
    if dtype in (torch.float32, torch.float16):
        assert err <= F32_TOL, f"{name}: {err:.3e} > {F32_TOL}"
    else:
        ps = O.psnr(y, ref)
        assert err <= BF16_TOL and ps >= BF16_PSNR, f"{name}: err {err:.3e} psnr {ps:.1f}"


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("tag", ["B_64", "B_256", "tiny_64", "tiny32_64"])
def test_model_win4_golden(golden, tag, dtype):
    """Uformer_B at 64x64 (batch 2) and 256x256 (batch 1: train_denoise.py's validation patches, a 16x16 bottleneck of sixteen windows),
    tiny (head_dim 16) and tiny32 at 64x64, all built with img_size 64, against the reference's outputs."""
    gd = golden("model_win4_" + tag)
    cfg = spec.arch_config(str(gd["arch"]), img_size=64)
    sd = spec.synth_state_dict(cfg, int(gd["seed"]))
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].numpy().tobytes())
    assert h.hexdigest() == str(gd["sd_sha256"])
    x = spec.synth_input(int(gd["B"]), int(gd["H"]), int(gd["W"]), int(gd["in_seed"]))
    m = build(str(gd["arch"]), dtype, int(gd["seed"]))
    with torch.no_grad():
        y = m(x.cuda())
    compare(f"{tag}_{TAG[dtype]}", y, torch.from_numpy(gd["y"]), dtype)


def check_param_grads(gd, grads, rtol):
    """every parameter gradient against the fixture's probes: two signed projections (rtol x ||g_ref||), a seeded 256-element gather or
    the full tensor and a few 64x64 blocks (rtol x max |g_ref|)"""
    names = [str(n) for n in gd["param_names"]]
    assert sorted(names) == sorted(grads), "parameter set differs from the reference's named_parameters()"
    worst = (0.0, "")
    for i, n in enumerate(names):
        gr = grads[n].detach().float().cpu()
        l2, mx = float(gd["norms"][i, 0]), float(gd["norms"][i, 1])
        for k in range(2):
            dev = abs(float((gr.double() * proj_vector(n, k, gr.shape).double()).sum()) - float(gd["proj"][i, k])) / max(l2, 1e-30)
            assert dev <= rtol, f"{n}: projection {k} off by {dev:.3e} x ||g||"
            worst = max(worst, (dev, n))
        if "full." + n in gd:
            got, want = gr, torch.from_numpy(gd["full." + n])
        else:
            got, want = gr.reshape(-1)[gather_index(n, gr.numel(), 256)], torch.from_numpy(gd["gather." + n])
        dev = (got - want).abs().max().item() / max(mx, 1e-30)
        assert dev <= rtol, f"{n}: elements off by {dev:.3e} x max|g|"
        if "block64." + n in gd:
            dev = (gr.reshape(gr.shape[0], -1)[:64, :64] - torch.from_numpy(gd["block64." + n])).abs().max().item() / max(mx, 1e-30)
            assert dev <= rtol, f"{n}: 64x64 block off by {dev:.3e} x max|g|"
    return worst


@pytest.mark.parametrize("dtype,ckpt", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True), (torch.float16, False),
                                        (torch.float16, True)])
def test_tiny32_gradients_vs_reference_autograd(golden, dtype, ckpt):
    """All 299 parameter gradients of tiny32 (img_size 64, 64x64, batch 2; both bottleneck relative-position tables in full) and d loss / d x
    under the reference's Charbonnier loss, through the module's autograd path, kept form and use_checkpoint=True."""
    gd = golden("grad_model_tiny32_64")
    y_ref = torch.from_numpy(golden("model_win4_tiny32_64")["y"])
    target = spec.synth_input(2, 64, 64, 1235)
    d = (y_ref - target).double()
    assert abs(float(torch.sqrt(d * d + 1e-6).mean()) - float(gd["loss"])) < 1e-6
    dy = (d / torch.sqrt(d * d + 1e-6) / d.numel()).float()                  # d loss / d y at the reference output (losses.py:41-52)
    m = build("tiny32", dtype, use_checkpoint=ckpt)
    x = spec.synth_input(2, 64, 64, 1234).cuda().requires_grad_(True)
    y = m(x)
    ls = F16_LOSS_SCALE if dtype == torch.float16 else 1.0
    y.backward(dy.cuda() * ls)
    compare(f"tiny32_64_autograd_{TAG[dtype]}", y.detach(), y_ref, dtype)
    rtol = GRAD_RTOL[dtype]
    assert rel(x.grad / ls, torch.from_numpy(gd["dx"])) < rtol
    check_param_grads(gd, {n: p_.grad / ls for n, p_ in m.named_parameters()}, rtol)


def test_rectangular_64x192_three_ways():
    m = build("tiny32", torch.float32)
    x = spec.synth_input(3, 64, 192, 77).cuda()
    with torch.no_grad():
        y = m(x)
    y_ag = m(x.clone().requires_grad_(True))                                 # grad mode: the autograd tape
    assert y_ag.grad_fn is not None
    assert (y_ag.detach() - y).abs().max().item() <= 1e-5
    mb = build("tiny32", torch.bfloat16)
    x8 = spec.synth_input(8, 64, 192, 78).cuda()
    with torch.no_grad():
        y8 = mb(x8)                                                           # two parts on two streams
        for i in range(8):
            assert torch.equal(mb(x8[i:i + 1]), y8[i:i + 1]), i
        yt = m(x.transpose(-1, -2).contiguous())
    assert tuple(yt.shape) == (3, 3, 192, 64) and torch.isfinite(yt).all()


def test_adamw_step_at_train_ps_64_batch_32_bf16():
    from uformer_amd import losses, optim
    torch.manual_seed(1234)
    m = model.get_arch("Uformer_B", train_ps=64, compute_dtype=torch.bfloat16)
    m.load_state_dict(spec.synth_state_dict(spec.arch_config("Uformer_B", img_size=64), 1234), strict=True)
    m = m.cuda().train()
    opt = optim.AdamW(m.parameters(), lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    x = spec.synth_input(32, 64, 64, 11).cuda()
    target = spec.synth_input(32, 64, 64, 12).cuda()
    tables = [b.attn.relative_position_bias_table for b in m.conv.blocks]
    before = [t.detach().clone() for t in tables]
    opt.zero_grad(set_to_none=True)
    loss = losses.CharbonnierLoss()(m(x), target)
    loss.backward()
    assert torch.isfinite(loss).item()
    for n, p_ in m.named_parameters():
        assert p_.grad is not None and torch.isfinite(p_.grad).all(), n
    assert all(t.grad.abs().sum().item() > 0 for t in tables)
    opt.step()
    torch.cuda.synchronize()
    assert all(not torch.equal(t.detach(), b) for t, b in zip(tables, before))
