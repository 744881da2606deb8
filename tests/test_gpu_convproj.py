"""GPU: ``token_projection='conv'`` -- the ConvProjection producer ``uf_ln_convqkv_fwd`` and the models built on it (inference).

Gates (none derived from what the code produces):
  * exact lattice: ``torch.equal`` against an fp64 evaluation on a dyadic lattice every value of which (xw, P, the outputs) is exactly
    representable in bf16, so all three operand types must return the same bits;
  * uf_ln_convqkv_fwd against an fp64 evaluation of the formula: the per-op gates of tests/test_gpu_ops.py (``OP_TOL``: 2e-4 / 2.5e-2 / 2.5e-2 / 8,
    x max(1, max |ref|)), as tests/test_gpu_ffn.py uses them;
  * blocks: the same per-op gates against the reference's own block outputs;
  * whole models: the gates of tests/test_gpu_model.py (1e-3 for f32 and f16; 4e-3 and 60 dB for bf16)."""
import dataclasses
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convproj_composition as CC
from oracle import uformer_oracle as O
from uformer_amd import _lib, model, ops, spec

pytestmark = pytest.mark.gpu

MODES = [torch.float32, torch.bfloat16, torch.float16]
TAG = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
OP_TOL = {torch.float32: 2e-4, torch.bfloat16: 2.5e-2, torch.float16: 2.5e-2 / 8}       # tests/test_gpu_ops.py: F32_TOL, BF16_REL, F16_REL
F32_TOL, BF16_TOL, BF16_PSNR = 1e-3, 4e-3, 60.0                                          # tests/test_gpu_model.py
WIDTHS = [16, 32, 64, 128, 256, 512]
HEADS = {16: 1, 32: 1, 64: 4, 128: 2, 256: 8, 512: 16}                                   # head_dim 16, 32, 16, 64, 32, 32


def t(a):
    return torch.from_numpy(np.asarray(a))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def conv_qkv_fp64(x, p, heads, B, H, W, shift, normed=None):
    """The formula of include/uformer_hip.h in fp64: LN1 -> roll -> partition -> + modulator, then per window and third the depthwise 3x3
    (F.conv2d, zero padding 1 on the 8x8 window image) + bias, ReLU, pointwise + bias.  Returns q (scaled), k (nW, heads, 64, hd) and
    v^T (nW, heads, hd, 64).  ``normed``: the LayerNorm's output given directly (the lattice test)."""
    C = x.shape[1]
    hd = C // heads
    if normed is None:
        xd = x.double()
        mu = xd.mean(-1, keepdim=True)
        var = ((xd - mu) ** 2).mean(-1, keepdim=True)
        normed = (xd - mu) / torch.sqrt(var + 1e-5) * p["gamma"].double() + p["beta"].double()
    y = normed.double().reshape(B, H, W, C)
    if shift:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    xw = O.window_partition(y, 8).reshape(-1, 64, C)
    if p.get("modulator") is not None:
        xw = xw + p["modulator"].double()
    img = xw.transpose(1, 2).reshape(-1, C, 8, 8)
    outs = []
    for j in range(3):
        wdw = p["dw9"][j].double().t().reshape(C, 1, 3, 3)                            # (9, C) tap-major -> (C, 1, ky, kx)
        pj = F.relu(F.conv2d(img, wdw, p["bdw"][j].double(), padding=1, groups=C))
        oj = torch.einsum("bchw,nc->bnhw", pj, p["wpw"][j * C:(j + 1) * C].double()) + p["bpw"][j * C:(j + 1) * C].double().reshape(1, C, 1, 1)
        outs.append(oj.reshape(-1, heads, hd, 64))                                    # 'b (h d) l w -> b h d (l w)'
    return outs[0].transpose(2, 3) * hd ** -0.5, outs[1].transpose(2, 3), outs[2]


def run_kernel(x, p, dtype, heads, B, H, W, shift=0, ld=None):
    """uf_ln_convqkv_fwd on a buffer of row stride ld whose pad columns and over-allocated tail are NaN."""
    M, C = x.shape
    ld = ld or C
    buf = torch.full((M + 8, ld), float("nan"))
    buf[:M, :C] = x
    d = {k: (None if v is None else v.cuda()) for k, v in p.items()}
    q, k, vt = ops.ln_conv_qkv(buf.cuda()[:M], d["gamma"], d["beta"], d["dw9"], d["bdw"], d["wpw"].to(dtype), d["bpw"], heads, B=B, H=H, W=W, shift=shift,
                               modulator=d.get("modulator"), C=C)
    torch.cuda.synchronize()
    return q.cpu(), k.cpu(), vt.cpu()


# ---------------------------------------------------------------------------------------------------------------------------------------
# exact lattice
# ---------------------------------------------------------------------------------------------------------------------------------------
def lattice_params(C, seed):
    """norm1.weight = 0, so xw = norm1.bias + modulator whatever x is: integers in [-2, 2] that differ strongly from one window position to the
    next (the four windows of the map share them -- with a zero LayerNorm weight nothing of x reaches xw).  The nine taps of a channel are the
    nine DISTINCT multiples of 1/2 in [-2, 2] (there are only five integers there) in an order of their own per channel and per third, so they are
    asymmetric under every flip or transposition; depthwise biases in {-1, 0, 1}; every pointwise row has three entries of +-1, the rest 0.
    Bounds: |xw| <= 2, |P| <= 10 * 2 + 1 = 21 in halves, |out| <= 3 * 21 + 1 = 64 in halves, q scaled by 1/4 or 1/8: eighths or sixteenths
    below 2^8 units -- everything is exact in bf16's 8 significant bits, and in f32 accumulation."""
    g = gen(seed)
    beta = torch.randint(-1, 2, (C,), generator=g).float()
    mod = torch.randint(-1, 2, (64, C), generator=g).float()
    taps = torch.arange(-4, 5).float() / 2
    dw9 = torch.stack([torch.stack([taps[torch.randperm(9, generator=g)] for _ in range(C)], 1) for _ in range(3)])          # (3, 9, C)
    bdw = torch.randint(-1, 2, (3, C), generator=g).float()
    wpw = torch.zeros(3 * C, C)
    for n in range(3 * C):
        cols = torch.randperm(C, generator=g)[:3]
        wpw[n, cols] = (torch.randint(0, 2, (3,), generator=g) * 2 - 1).float()
    bpw = torch.randint(-1, 2, (3 * C,), generator=g).float()
    return dict(gamma=torch.zeros(C), beta=beta, modulator=mod, dw9=dw9, bdw=bdw, wpw=wpw, bpw=bpw)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("C", [16, 64, 32])
@pytest.mark.parametrize("dtype", MODES)
def test_convqkv_exact_on_a_lattice(dtype, C, shift):
    """B = 1, H = W = 16 (four windows), 1 head: head_dim 16 and 64 scale q by a power of two, so q, k and v^T are compared with torch.equal;
    at head_dim 32 (scale 2^-2.5) k and v^T only.  A tap that crosses the window border reads a lattice value where the formula has zero
    padding, a swapped ky / kx or another third's taps or pointwise rows pick another of the nine distinct values: each changes the result."""
    p = lattice_params(C, 900 + C)
    x = torch.randn(256, C, generator=gen(7 + C)) * 3 + 1
    normed = p["beta"].expand(256, C)
    ref = conv_qkv_fp64(x, p, 1, 1, 16, 16, shift, normed=normed)
    for name, r in zip(("q", "k", "vt"), ref):
        assert (name == "q" and C == 32) or torch.equal(r.to(torch.bfloat16).double(), r), "the lattice must be exact in bf16"
        assert r.abs().max().item() >= 2 and (r != 0).float().mean().item() > 0.5                 # not a degenerate case
    got = run_kernel(x, p, dtype, 1, 1, 16, 16, shift)
    for name, a, r in zip(("q", "k", "vt"), got, ref):
        if name == "q" and C == 32:
            continue
        assert a.dtype == dtype and torch.equal(a.double(), r), (name, TAG[dtype], C, shift, (a.double() - r).abs().max().item())


def test_lattice_detects_the_faults_it_is_built_for():
    """The lattice reference itself moves under each fault named above (evaluated on the CPU: a test of the test's inputs)."""
    C = 16
    p = lattice_params(C, 900 + C)
    normed = p["beta"].expand(256, C)
    ref = conv_qkv_fp64(torch.zeros(256, C), p, 1, 1, 16, 16, 0, normed=normed)
    swapped = dict(p, dw9=p["dw9"].reshape(3, 3, 3, C).transpose(1, 2).reshape(3, 9, C))             # ky <-> kx
    rolled = dict(p, dw9=p["dw9"].roll(1, 0))                                                         # another third's taps
    wrong_w = dict(p, wpw=p["wpw"].roll(C, 0))                                                        # another third's pointwise rows
    for bad in (swapped, rolled, wrong_w):
        out = conv_qkv_fp64(torch.zeros(256, C), bad, 1, 1, 16, 16, 0, normed=normed)
        assert all(not torch.equal(a, b) for a, b in zip(out, ref))


def test_fp64_formula_is_the_pinned_composition():
    """conv_qkv_fp64 (this file's reference) against tests/convproj_composition.py, which tests/test_convproj.py pins to the reference (CPU only)."""
    C, heads = 32, 2
    x, p = conv_inputs(C, 256, 1)
    sd = {}
    for j, n in enumerate("qkv"):
        sd[f"to_{n}.depthwise.weight"] = p["dw9"][j].t().reshape(C, 1, 3, 3).double()
        sd[f"to_{n}.depthwise.bias"] = p["bdw"][j].double()
        sd[f"to_{n}.pointwise.weight"] = p["wpw"][j * C:(j + 1) * C].reshape(C, C, 1, 1).double()
        sd[f"to_{n}.pointwise.bias"] = p["bpw"][j * C:(j + 1) * C].double()
    xw = O.window_partition(torch.roll(O.layer_norm(x.double(), p["gamma"].double(), p["beta"].double()).reshape(1, 16, 16, C), (-4, -4), (1, 2)), 8)
    q, k, v = CC.conv_projection(xw.reshape(-1, 64, C) + p["modulator"].double(), sd, "", heads)
    rq, rk, rvt = conv_qkv_fp64(x, p, heads, 1, 16, 16, 4)
    assert (q * (C // heads) ** -0.5 - rq).abs().max() < 1e-12 and (k - rk).abs().max() < 1e-12 and (v.transpose(2, 3) - rvt).abs().max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------------
# against the fp64 formula
# ---------------------------------------------------------------------------------------------------------------------------------------
def conv_inputs(C, M, seed, modulator=True):
    x = torch.randn(M, C, generator=gen(seed)) * 1.5 + 0.3
    return x, dict(gamma=1 + 0.1 * torch.randn(C, generator=gen(seed + 1)), beta=0.1 * torch.randn(C, generator=gen(seed + 2)),
                   modulator=0.5 * torch.randn(64, C, generator=gen(seed + 3)) if modulator else None,
                   dw9=0.3 * torch.randn(3, 9, C, generator=gen(seed + 4)), bdw=0.1 * torch.randn(3, C, generator=gen(seed + 5)),
                   wpw=torch.randn(3 * C, C, generator=gen(seed + 6)) / C ** 0.5, bpw=0.1 * torch.randn(3 * C, generator=gen(seed + 7)))


def check_qkv(name, got, ref, dtype):
    for part, a, r in zip(("q", "k", "vt"), got, ref):
        assert a.shape == r.shape and torch.isfinite(a).all(), (name, part)
        err = (a.double() - r).abs().max().item()
        tol = OP_TOL[dtype] * max(1.0, r.abs().max().item())
        print(f"{name} {part}[{TAG[dtype]}]: err {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (name, part, err, tol)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", MODES)
def test_convqkv_kernel_vs_fp64(dtype, C):
    """M = 64 (one 8x8 map) and B = 3 maps of 8x8, ld = C and ld = C + 8 with NaN in the pad columns and after the last row of x: the outputs must be
    finite (no NaN read into them).  Beyond the cases the gate names: a 16x16 map with shift 4 (four windows, rolled gather) and no modulator."""
    heads = HEADS[C]
    for B in (1, 3):
        x, p = conv_inputs(C, 64 * B, 2000 + C + B)
        ref = conv_qkv_fp64(x, p, heads, B, 8, 8, 0)
        for ld in (C, C + 8):
            check_qkv(f"uf_ln_convqkv_fwd C={C} B={B} ld={ld}", run_kernel(x, p, dtype, heads, B, 8, 8, 0, ld), ref, dtype)
    x, p = conv_inputs(C, 256, 3000 + C, modulator=False)
    check_qkv(f"uf_ln_convqkv_fwd C={C} 16x16 shift 4", run_kernel(x, p, dtype, heads, 1, 16, 16, 4, C + 8), conv_qkv_fp64(x, p, heads, 1, 16, 16, 4), dtype)


@pytest.mark.parametrize("dtype,C", [(torch.bfloat16, 32), (torch.bfloat16, 256), (torch.float32, 512)])
def test_convqkv_deterministic_and_batch_invariant(dtype, C):
    x, p = conv_inputs(C, 192, 5 + C)
    a = run_kernel(x, p, dtype, HEADS[C], 3, 8, 8, 0, C + 8)
    b = run_kernel(x, p, dtype, HEADS[C], 3, 8, 8, 0, C + 8)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    parts = [run_kernel(x[i * 64:(i + 1) * 64], p, dtype, HEADS[C], 1, 8, 8, 0) for i in range(3)]
    for i in range(3):
        assert torch.equal(a[i], torch.cat([pt[i] for pt in parts]))                    # a batch of 3 = three batches of 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# blocks and models
# ---------------------------------------------------------------------------------------------------------------------------------------
def op_check(name, got, ref, dtype):
    got = got.detach().float().cpu()
    err = (got - ref).abs().max().item()
    tol = OP_TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"{name}[{TAG[dtype]}]: err {err:.3e} (tol {tol:.3e})")
    assert torch.isfinite(got).all() and err <= tol, (name, err, tol)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("tag", ["a", "b"])
def test_convproj_block_vs_reference(golden, dtype, tag):
    g = golden("convproj_lewin_block_" + tag)
    C, heads, shift = int(g["C"]), int(g["heads"]), int(g["shift"])
    blk = model.LeWinTransformerBlock(C, (16, 16), heads, win_size=8, shift_size=shift, token_projection="conv", modulator=(tag == "a"))
    blk.load_state_dict({k[2:]: t(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    blk = blk.cuda().eval()
    with torch.no_grad():
        op_check(f"convproj_lewin_block_{tag}", blk(t(g["x"]).cuda(), None, dtype), t(g["y"]), dtype)


def conv_cfg(**kw):
    return dataclasses.replace(spec.arch_config("tiny32", img_size=128), token_projection="conv", **kw)


def build(cfg, dtype, seed=1234, **kw):
    m = model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                      modulator=cfg.modulator, dd_in=cfg.dd_in, token_mlp=cfg.token_mlp, token_projection=cfg.token_projection, compute_dtype=dtype, **kw)
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
def test_convproj_model_vs_reference(golden, dtype, tag):
    g = golden("convproj_model_tiny32_" + tag)
    m = build(conv_cfg(), dtype, int(g["seed"])).eval()
    x = spec.synth_input(int(g["B"]), int(g["H"]), int(g["W"]), int(g["in_seed"]))
    with torch.no_grad():
        model_compare("convproj_model_tiny32_" + tag, m(x.cuda()), t(g["y"]), dtype)


def test_convproj_model_paths_are_bit_equal():
    """The mask path (module by module; an all-zero mask adds 0 to every logit), a GraphedForward replay, a PipelinedForward run and infer.restore's
    padded canvas against the plain one-call forward of the same model; a real mask against the composition."""
    from uformer_amd import infer
    cfg = conv_cfg()
    m = build(cfg, torch.bfloat16, 31).eval()
    xs = [spec.synth_input(2, 128, 128, 60 + i).cuda() for i in range(2)]
    with torch.no_grad():
        plain = [m(xx).clone() for xx in xs]
        assert torch.equal(m(xs[0], torch.zeros(2, 1, 128, 128, device="cuda")), plain[0])
        gf = infer.GraphedForward(m, xs[0])
        for xx, y in zip(xs, plain):
            assert torch.equal(gf(xx), y)
        pf = infer.PipelinedForward(m, depth=2)
        for y, want in zip(pf.map(xs), plain):
            assert torch.equal(y, want)
        r = infer.restore(m, xs[0][:1, :, :100, :90])
        assert r.shape == (1, 3, 100, 90) and torch.isfinite(r).all()
        mf = build(cfg, torch.float32, 11).eval()
        x = spec.synth_input(1, 128, 128, 12)
        mask = (torch.rand(1, 1, 128, 128, generator=gen(5)) > 0.3).float()
        ref = CC.uformer_forward(x, spec.synth_state_dict(cfg, 11), img_size=128, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, mask=mask)
        model_compare("convproj_usermask", mf(x.cuda(), mask.cuda()), ref, torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_projection_with_ffn(dtype):
    cfg = conv_cfg(token_mlp="ffn")
    m = build(cfg, dtype, 21).eval()
    x = spec.synth_input(1, 128, 128, 22)
    with torch.no_grad():
        ref = CC.uformer_forward(x, spec.synth_state_dict(cfg, 21), img_size=128, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads)
        model_compare("convproj_with_ffn", m(x.cuda()), ref, dtype)


def kernel_names(m, x):
    import ctypes
    lib = _lib.load()
    lib.uf_timing_enable(1)
    try:
        with torch.no_grad():
            y = m(x)
        torch.cuda.synchronize()
    finally:
        lib.uf_timing_enable(0)
    buf = ctypes.create_string_buffer(1 << 20)
    lib.uf_timing_report(buf, len(buf))
    return [k["kernel"] for k in json.loads(buf.value.decode())], y


def test_linear_models_never_reach_the_conv_kernel():
    x = spec.synth_input(1, 128, 128, 3).cuda()
    lin = spec.arch_config("tiny32", img_size=128)
    ml = model.Uformer(img_size=128, embed_dim=32, depths=list(lin.depths), num_heads=list(lin.num_heads), modulator=True, compute_dtype=torch.bfloat16)
    ml.load_state_dict(spec.synth_state_dict(lin, 1234), strict=True)
    ml = ml.cuda().eval()
    names, y_timed = kernel_names(ml, x)
    assert names and not any(n.startswith("ln_convqkv") for n in names) and any(n.startswith("attn_block") for n in names), names
    pk = ml._get_packed(x.device)
    assert all(b.qkv_dw9 is None and b.qkv_bdw is None for b in pk.blocks)               # the new fields of every block are NULL ...
    with torch.no_grad():
        assert torch.equal(ml(x), y_timed)                                                # ... and the forward is the same bits, timed or not
    names, _ = kernel_names(build(conv_cfg(), torch.bfloat16).eval(), x)
    assert any(n.startswith("ln_convqkv") for n in names), names
    assert not any(n.startswith("attn_block") or n.startswith("ln_gemm_bf16_qkv") for n in names), names
