"""GPU: ``token_mlp='ffn'`` -- the fused feed-forward kernel ``uf_ffn_fwd`` and the models built on it.

Gates (none derived from what the code produces):
  * uf_ffn_fwd, f32 operands: 2e-4 x max(1, |ref|) against an fp64 evaluation of the formula (the per-op f32 gate of tests/test_gpu_ops.py);
  * uf_ffn_fwd, bf16 / f16: error against fp64 <= 1.5 x the error of the UNFUSED composition of existing entry points on the same inputs
    (uf_ln_linear_gelu_fwd writing h, then uf_linear_residual_fwd: the same rounding points -- LN output, GELU output -- in another f32
    summation order, which is all the 1.5 allows for);
  * blocks: the per-op gates of tests/test_gpu_ops.py (``check``: 2e-4 / 2.5e-2 / 2.5e-2 / 8, x max(1, |ref|));
  * whole models: the gates of tests/test_gpu_model.py (``compare``: 1e-3 for f32 and f16; 4e-3 and 60 dB for bf16);
  * train-mode forward and gradients: the whole-model rule of tests/test_gpu_bwd.py (GRAD_RTOL: 2e-3 / 6e-2 / 1e-2 relative), on the probes of tests/gradproj.py.
"""
import json
import os

import numpy as np
import pytest
import torch

import ffn_composition as FC
from gradproj import gather_index, proj_vector
from oracle import uformer_oracle as O
from uformer_amd import _lib, losses, model, ops, optim, spec

pytestmark = pytest.mark.gpu

MODES = [torch.float32, torch.bfloat16, torch.float16]
TAG = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
OP_TOL = {torch.float32: 2e-4, torch.bfloat16: 2.5e-2, torch.float16: 2.5e-2 / 8}       # tests/test_gpu_ops.py: F32_TOL, BF16_REL, F16_REL
F32_TOL, BF16_TOL, BF16_PSNR = 1e-3, 4e-3, 60.0                                          # tests/test_gpu_model.py
GRAD_RTOL = {torch.float32: 2e-3, torch.bfloat16: 6e-2, torch.float16: 1e-2}             # tests/test_gpu_bwd.py (whole-model gradient gates)
F16_LOSS_SCALE = 65536.0
WIDTHS = [16, 32, 64, 128, 256, 512]
PARITY = {}


def t(a):
    return torch.from_numpy(np.asarray(a))


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("UF_FFN_PARITY_OUT")       # profiles/ffn_parity.json is this dump (UF_FFN_PARITY_OUT=<path> pytest tests/test_gpu_ffn.py -m gpu)
    if out and PARITY:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)


def ffn_inputs(C, M, seed):
    x = torch.randn(M, C, generator=gen(seed)) * 1.5 + 0.3
    p = dict(gamma=1 + 0.1 * torch.randn(C, generator=gen(seed + 1)), beta=0.1 * torch.randn(C, generator=gen(seed + 2)),
             w1=torch.randn(4 * C, C, generator=gen(seed + 3)) / C ** 0.5, b1=0.1 * torch.randn(4 * C, generator=gen(seed + 4)),
             w2=torch.randn(C, 4 * C, generator=gen(seed + 5)) / (4 * C) ** 0.5, b2=0.1 * torch.randn(C, generator=gen(seed + 6)))
    return x, p


def ffn_fp64(x, p, scale=None, hw=64):
    x = x.double()
    C = x.shape[1]
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    z = (x - mu) / torch.sqrt(var + 1e-5) * p["gamma"].double() + p["beta"].double()
    a = z @ p["w1"].double().t() + p["b1"].double()
    h = 0.5 * a * (1 + torch.erf(a / 2 ** 0.5))
    br = h @ p["w2"].double().t() + p["b2"].double()
    s = 1.0 if scale is None else scale.double().repeat_interleave(hw)[:, None]
    return x + s * br


def run_fused(x, p, dtype, B, ld=None, scale=None):
    """uf_ffn_fwd on a buffer of row stride ld whose pad columns and over-allocated tail are NaN; returns (rows [M, C], whole buffer)."""
    M, C = x.shape
    ld = ld or C
    buf = torch.full((M + 8, ld), float("nan"))
    buf[:M, :C] = x
    buf = buf.cuda()
    d = {k: v.cuda() for k, v in p.items()}
    view = buf[:M]
    ops.ffn(view, d["gamma"], d["beta"], d["w1"].to(dtype), d["b1"], d["w2"].to(dtype), d["b2"], None if scale is None else scale.cuda(), B, C=C)
    torch.cuda.synchronize()
    return buf[:M, :C].cpu(), buf.cpu()


def run_unfused(x, p, dtype, B, scale=None):
    """The same formula from existing entry points: LN2 + fc1 + GELU GEMM writing h, then the linear-with-residual GEMM."""
    M, C = x.shape
    d = {k: v.cuda() for k, v in p.items()}
    h = ops.ln_linear_gelu(x.cuda(), d["gamma"], d["beta"], d["w1"].to(dtype), d["b1"])
    hw = M // B
    y = ops.linear_residual(h, d["w2"].to(dtype), d["b2"], x.cuda(), None if scale is None else scale.cuda(), B, 8, hw // 8)
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", MODES)
def test_ffn_kernel_vs_fp64(dtype, C):
    """M = 64 (one 8x8 map) and M = 192 (B = 3: an odd number of 64-row tiles), ld = C and ld = C + 8 with NaN in the pad columns and after
    the last row, which must come back untouched."""
    worst_f = worst_u = 0.0
    for M, B in ((64, 1), (192, 3)):
        x, p = ffn_inputs(C, M, 1000 + C + M)
        ref = ffn_fp64(x, p)
        eu = None
        if dtype != torch.float32:
            eu = (run_unfused(x, p, dtype, B).double() - ref).abs().max().item()
        for ld in (C, C + 8):
            y, buf = run_fused(x, p, dtype, B, ld)
            assert torch.isnan(buf[M:]).all(), "rows after the last were written"
            assert ld == C or torch.isnan(buf[:M, C:]).all(), "pad columns were written"
            assert torch.isfinite(y).all()
            ef = (y.double() - ref).abs().max().item()
            print(f"uf_ffn_fwd {TAG[dtype]} C={C} M={M} ld={ld}: fused err {ef:.3e}" + ("" if eu is None else f", unfused err {eu:.3e}"))
            if dtype == torch.float32:
                assert ef <= OP_TOL[dtype] * max(1.0, ref.abs().max().item()), (C, M, ld, ef)
            else:
                assert ef <= 1.5 * eu, (C, M, ld, ef, eu)
                worst_u = max(worst_u, eu)
            worst_f = max(worst_f, ef)
    PARITY[f"C{C}[{TAG[dtype]}]"] = {"fused_max_abs_err_vs_fp64": worst_f, **({} if dtype == torch.float32 else {"unfused_max_abs_err_vs_fp64": worst_u})}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ffn_droppath_scales(dtype):
    C, M, B = 64, 192, 3
    x, p = ffn_inputs(C, M, 77)
    scale = torch.tensor([0.0, 1 / 0.7, 1.0])
    y, _ = run_fused(x, p, dtype, B, scale=scale)
    assert torch.equal(y[:64], x[:64])                                  # a dropped image is bit-equal to its input
    y1, _ = run_fused(x, p, dtype, B)
    assert torch.equal(y[128:], y1[128:])                               # scale 1 = no scale
    yo, _ = run_fused(x, p, dtype, B, scale=torch.ones(3))
    assert torch.equal(yo, y1)                                          # NULL is bit-equal to all-ones
    ref = ffn_fp64(x, p, scale)
    tol = OP_TOL[dtype] * max(1.0, ref.abs().max().item())
    assert (y.double() - ref).abs().max().item() <= tol


@pytest.mark.parametrize("C", [32, 256])
def test_ffn_deterministic_and_batch_invariant(C):
    x, p = ffn_inputs(C, 192, 5 + C)
    a, _ = run_fused(x, p, torch.bfloat16, 3, C + 8)
    b, _ = run_fused(x, p, torch.bfloat16, 3, C + 8)
    assert torch.equal(a, b)
    parts = torch.cat([run_fused(x[i * 64:(i + 1) * 64], p, torch.bfloat16, 1)[0] for i in range(3)])
    assert torch.equal(a, parts)                                        # a batch of 3 = three batches of 1


def op_check(name, got, ref, dtype):
    got = got.detach().float().cpu()
    err = (got - ref).abs().max().item()
    tol = OP_TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"{name}[{TAG[dtype]}]: err {err:.3e} (tol {tol:.3e})")
    assert torch.isfinite(got).all() and err <= tol, (name, err, tol)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("tag", ["a", "b"])
def test_ffn_block_vs_reference(golden, dtype, tag):
    g = golden("ffn_lewin_block_" + tag)
    C, heads, shift = int(g["C"]), int(g["heads"]), int(g["shift"])
    blk = model.LeWinTransformerBlock(C, (16, 16), heads, win_size=8, shift_size=shift, token_mlp="ffn", modulator=(tag == "a"))
    blk.load_state_dict({k[2:]: t(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    blk = blk.cuda().eval()
    with torch.no_grad():
        op_check(f"ffn_lewin_block_{tag}", blk(t(g["x"]).cuda(), None, dtype), t(g["y"]), dtype)


def ffn_cfg():
    import dataclasses
    return dataclasses.replace(spec.arch_config("tiny32", img_size=128), token_mlp="ffn")


def build(cfg, dtype, seed=1234, **kw):
    m = model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                      modulator=cfg.modulator, dd_in=cfg.dd_in, token_mlp=cfg.token_mlp, compute_dtype=dtype, **kw)
    m.load_state_dict(spec.synth_state_dict(cfg, seed), strict=True)
    return m.cuda()


def model_compare(name, y, ref, dtype):
    y = y.float().cpu()
    err = (y - ref).abs().max().item()
    ps = O.psnr(y, ref)
    print(f"{name}[{TAG[dtype]}]: err {err:.3e} psnr {ps:.1f} dB")
    assert torch.isfinite(y).all()
    if dtype in (torch.float32, torch.float16):
        assert err <= F32_TOL, (name, err)
    else:
        assert err <= BF16_TOL and ps >= BF16_PSNR, (name, err, ps)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("tag", ["128", "128x256"])
def test_ffn_model_vs_reference(golden, dtype, tag):
    g = golden("ffn_model_tiny32_" + tag)
    m = build(ffn_cfg(), dtype, int(g["seed"])).eval()
    x = spec.synth_input(int(g["B"]), int(g["H"]), int(g["W"]), int(g["in_seed"]))
    with torch.no_grad():
        y = m(x.cuda())
        model_compare("ffn_model_tiny32_" + tag, y, t(g["y"]), dtype)
        assert torch.equal(y, m._forward_blockwise(x.cuda(), None))     # module by module = the one-call forward, bit for bit


def test_ffn_mask_inference_and_graph_replay():
    from uformer_amd import infer
    cfg = ffn_cfg()
    sd = spec.synth_state_dict(cfg, 11)
    m = build(cfg, torch.float32, 11).eval()
    x = spec.synth_input(1, 128, 128, 12)
    mask = (torch.rand(1, 1, 128, 128, generator=gen(5)) > 0.3).float()
    with torch.no_grad():
        y = m(x.cuda(), mask.cuda())
        ref = FC.uformer_forward(x, sd, img_size=128, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, mask=mask)
        model_compare("ffn_usermask", y, ref, torch.float32)
        mb = build(cfg, torch.bfloat16, 31).eval()
        xs = [spec.synth_input(2, 128, 128, 60 + i).cuda() for i in range(2)]
        gf = infer.GraphedForward(mb, xs[0])
        for xx in xs:
            assert torch.equal(gf(xx), mb(xx))


def check_param_grads(gd, grads, rtol):
    """tests/test_gpu_hd64.py's probe check: two signed projections (rtol x ||g_ref||), a seeded 256-element gather or the full tensor
    (rtol x max |g_ref|)"""
    names = [str(n) for n in gd["param_names"]]
    assert sorted(names) == sorted(grads), sorted(set(names) ^ set(grads))
    worst = (0.0, "")
    for i, n in enumerate(names):
        gr = grads[n].detach().float().cpu()
        l2, mx = float(gd["norms"][i, 0]), float(gd["norms"][i, 1])
        for k in range(2):
            dev = abs(float((gr.double() * proj_vector(n, k, gr.shape).double()).sum()) - float(gd["proj"][i, k])) / max(l2, 1e-30)
            worst = max(worst, (dev, n + f" projection {k}"))
        if "full." + n in gd:
            got, want = gr, t(gd["full." + n])
        else:
            got, want = gr.reshape(-1)[gather_index(n, gr.numel(), 256)], t(gd["gather." + n])
        worst = max(worst, ((got - want).abs().max().item() / max(mx, 1e-30), n + " elements"))
    return worst


@pytest.mark.parametrize("ckpt", [False, True])
@pytest.mark.parametrize("dtype", MODES)
def test_ffn_train_mode_gradients_vs_reference_autograd(golden, dtype, ckpt):
    """train() mode with the DropPath masks the reference drew, Charbonnier loss: kept-intermediates form and use_checkpoint=True."""
    gd = golden("ffn_grad_tiny32_128")
    cfg = ffn_cfg()
    m = build(cfg, dtype, drop_path_rate=float(gd["drop_path_rate"]), use_checkpoint=ckpt).train()
    m._drop_scales_override = t(gd["masks"]).cuda()
    x = spec.synth_input(2, 128, 128, 4321).cuda().requires_grad_(True)
    target = spec.synth_input(2, 128, 128, 4322)
    y_ref = t(gd["y"])
    d = (y_ref - target).double()
    assert abs(float(torch.sqrt(d * d + 1e-6).mean()) - float(gd["loss"])) < 1e-6
    dy = (d / torch.sqrt(d * d + 1e-6) / d.numel()).float()              # d loss / d y at the reference output (losses.py:41-52)
    y = m(x)
    # the train-mode forward at the rule tests/test_gpu_bwd.py applies to its train-mode fixture (test_module_train_mode_loss_backward_with_droppath:
    # relative to max |y_ref|, pick(dtype, 1e-5, 1e-2)): a kept branch is scaled by 1 / keep = 2 here, so the eval-mode image gates do not apply
    ey = (y.detach().float().cpu() - y_ref).abs().max().item() / y_ref.abs().max().item()
    print(f"ffn_train_forward_ckpt{int(ckpt)}[{TAG[dtype]}]: rel err {ey:.3e}")
    assert ey < {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 1e-2 / 4}[dtype], ey
    ls = F16_LOSS_SCALE if dtype == torch.float16 else 1.0
    y.backward(dy.cuda() * ls)
    rtol = GRAD_RTOL[dtype]
    dx = (x.grad / ls).float().cpu()
    l2, mx = float(gd["dx_norms"][0]), float(gd["dx_norms"][1])
    for k in range(2):
        assert abs(float((dx.double() * proj_vector("dx", k, dx.shape).double()).sum()) - float(gd["dx_proj"][k])) / l2 <= rtol
    assert (dx.reshape(-1)[gather_index("dx", dx.numel(), 4096)] - t(gd["dx_gather"])).abs().max().item() / mx <= rtol
    grads = {n: (p_.grad / ls if p_.grad is not None else torch.zeros_like(p_)) for n, p_ in m.named_parameters()}
    worst = check_param_grads(gd, grads, rtol)
    print(TAG[dtype], "ckpt", ckpt, "worst", worst)
    assert worst[0] <= rtol, worst
    assert any(n.endswith("mlp.fc1.weight") for n in grads) and any(n.endswith("mlp.fc2.bias") for n in grads)


@pytest.mark.parametrize("dtype", MODES)
def test_ffn_adamw_step(dtype):
    torch.manual_seed(5)
    m = build(ffn_cfg(), dtype).train()
    assert "conv.blocks.0.mlp.fc1.weight" in dict(m.named_parameters())
    opt = optim.AdamW(m.parameters(), lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    before = {n: p_.detach().clone() for n, p_ in m.named_parameters()}
    opt.zero_grad(set_to_none=True)
    loss = losses.CharbonnierLoss()(m(spec.synth_input(2, 128, 128, 11).cuda()), spec.synth_input(2, 128, 128, 12).cuda())
    if dtype == torch.float16:
        scaler = optim.GradScaler()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        assert scaler.steps_taken() == 1
    else:
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
    for n, p_ in m.named_parameters():
        assert torch.isfinite(p_).all(), n
    for n in ("conv.blocks.0.mlp.fc1.weight", "encoderlayer_0.blocks.0.mlp.fc2.weight", "decoderlayer_3.blocks.0.mlp.fc1.bias"):
        assert not torch.equal(dict(m.named_parameters())[n], before[n]), n


def kernel_names(m, x):
    import ctypes
    lib = _lib.load()
    lib.uf_timing_enable(1)
    try:
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()
    finally:
        lib.uf_timing_enable(0)
    buf = ctypes.create_string_buffer(1 << 20)
    lib.uf_timing_report(buf, len(buf))
    return [k["kernel"] for k in json.loads(buf.value.decode())]


def test_leff_models_never_reach_the_ffn_kernel():
    x = spec.synth_input(1, 128, 128, 3).cuda()
    leff = spec.arch_config("tiny32", img_size=128)
    ml = model.Uformer(img_size=128, embed_dim=32, depths=list(leff.depths), num_heads=list(leff.num_heads), modulator=True, compute_dtype=torch.bfloat16)
    ml.load_state_dict(spec.synth_state_dict(leff, 1234), strict=True)
    names = kernel_names(ml.cuda().eval(), x)
    assert names and not any(n.startswith("ffn_") for n in names), names
    names = kernel_names(build(ffn_cfg(), torch.bfloat16).eval(), x)
    assert any(n.startswith("ffn_") for n in names) and not any(n.startswith("leff2") for n in names), names
