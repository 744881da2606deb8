"""GPU: ``cross_modulator=True`` -- the cross-modulator attention kernel ``uf_cross_attn_fwd`` and the models built on it (inference).

Gates (none derived from what the code produces):
  * uf_cross_attn_fwd against a float64 evaluation of the formula: the per-op gates of tests/test_gpu_convproj.py (``OP_TOL``: 2e-4 / 2.5e-2 /
    2.5e-2 / 8, x max(1, max |ref|));
  * blocks: the same per-op gates against the reference's own block outputs;
  * whole models: the gates of tests/test_gpu_model.py (1e-3 for f32 and f16; 4e-3 and 60 dB for bf16);
  * paths (mask argument with an all-zero mask, graph replay, pipelined, two-part batch): bit-equal to the one-call forward."""
import dataclasses
import json

import numpy as np
import pytest
import torch

import crossmod_composition as XC
from oracle import uformer_oracle as O
from uformer_amd import _lib, model, ops, spec

pytestmark = pytest.mark.gpu

MODES = [torch.float32, torch.bfloat16, torch.float16]
TAG = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
OP_TOL = {torch.float32: 2e-4, torch.bfloat16: 2.5e-2, torch.float16: 2.5e-2 / 8}       # tests/test_gpu_convproj.py (tests/test_gpu_ops.py: F32_TOL, BF16_REL, F16_REL)
F32_TOL, BF16_TOL, BF16_PSNR = 1e-3, 4e-3, 60.0                                          # tests/test_gpu_model.py
WIDTHS = [16, 32, 64, 128, 256, 512]
HEADS = {16: 1, 32: 1, 64: 4, 128: 4, 256: 8, 512: 32}                                   # head_dim 16, 32, 16, 32, 32, 16


def t(a):
    return torch.from_numpy(np.asarray(a))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cross_fp64(x, p, heads):
    """The formula of include/uformer_hip.h in fp64: x + proj(softmax((x Wq^T + bq) hd^-0.5 K_h^T) V_h), K | V = to_kv(emb)."""
    x = x.double()
    C = x.shape[1]
    hd = C // heads
    q = ((x @ p["wq"].double().t() + p["bq"].double()) * hd ** -0.5).reshape(-1, heads, hd).transpose(0, 1)
    kv = p["emb"].double() @ p["wkv"].double().t() + p["bkv"].double()
    k = kv[:, :C].reshape(64, heads, hd).transpose(0, 1)
    v = kv[:, C:].reshape(64, heads, hd).transpose(0, 1)
    o = (torch.softmax(q @ k.transpose(1, 2), -1) @ v).transpose(0, 1).reshape(-1, C)
    return x + o @ p["wp"].double().t() + p["bp"].double()


@pytest.fixture(scope="module")
def cases():
    """inputs and the float64 reference of every width, computed once and shared (M = 512: the first 256 / 64 rows serve the smaller runs, every
    row being independent)"""
    out = {}
    for C in WIDTHS:
        s = 4000 + C
        p = dict(wq=torch.randn(C, C, generator=gen(s)) / C ** 0.5, bq=0.1 * torch.randn(C, generator=gen(s + 1)), emb=0.5 * torch.randn(64, C, generator=gen(s + 2)),
                 wkv=torch.randn(2 * C, C, generator=gen(s + 3)) / C ** 0.5 * 2, bkv=0.1 * torch.randn(2 * C, generator=gen(s + 4)),
                 wp=torch.randn(C, C, generator=gen(s + 5)) / C ** 0.5, bp=0.1 * torch.randn(C, generator=gen(s + 6)))
        x = torch.randn(512, C, generator=gen(s + 7)) * 1.5 + 0.3
        out[C] = (x, p, cross_fp64(x, p, HEADS[C]))
    return out


def run_kernel(x, p, dtype, heads, ld=None, poison=float("nan")):
    """uf_cross_attn_fwd in place on rows of stride ld inside a buffer whose pad columns and 8 extra rows are poisoned; returns the whole buffer.
    k and v^T are what packing.pack_cross makes: to_kv(emb) in f32, rounded to the operand type."""
    M, C = x.shape
    hd = C // heads
    ld = ld or C
    buf = torch.full((M + 8, ld), poison)
    buf[:M, :C] = x
    buf = buf.cuda()
    kv = torch.nn.functional.linear(p["emb"], p["wkv"], p["bkv"])
    k = kv[:, :C].reshape(64, heads, hd).permute(1, 0, 2).to(dtype).contiguous().cuda()
    vt = kv[:, C:].reshape(64, heads, hd).permute(1, 2, 0).to(dtype).contiguous().cuda()
    ops.cross_attn(buf[:M], p["wq"].to(dtype).cuda(), p["bq"].cuda(), k, vt, p["wp"].to(dtype).cuda(), p["bp"].cuda(), C=C)
    torch.cuda.synchronize()
    return buf.cpu()


def op_check(name, got, ref, dtype):
    got = got.detach().float().cpu()
    err = (got.double() - ref.double()).abs().max().item()
    tol = OP_TOL[dtype] * max(1.0, ref.abs().max().item())
    print(f"{name}[{TAG[dtype]}]: err {err:.3e} (tol {tol:.3e})")
    assert torch.isfinite(got).all() and err <= tol, (name, err, tol)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", MODES)
def test_cross_attn_kernel_vs_fp64(cases, dtype, C):
    """M = 256: four tiles (eight for f32 at C = 512)."""
    x, p, ref = cases[C]
    buf = run_kernel(x[:256], p, dtype, HEADS[C])
    op_check(f"uf_cross_attn_fwd C={C}", buf[:256], ref[:256], dtype)
    assert torch.isnan(buf[256:]).all()


@pytest.mark.parametrize("dtype", MODES)
def test_cross_attn_kernel_inside_a_concat_buffer(cases, dtype):
    """ld = 2C inside a poisoned buffer, which must come back intact outside the written columns."""
    C = 64
    x, p, ref = cases[C]
    buf = run_kernel(x[:256], p, dtype, HEADS[C], ld=2 * C, poison=-12345.0)
    op_check(f"uf_cross_attn_fwd C={C} ld={2 * C}", buf[:256, :C], ref[:256], dtype)
    assert bool((buf[:256, C:] == -12345.0).all()) and bool((buf[256:] == -12345.0).all())


@pytest.mark.parametrize("dtype,C", [(torch.bfloat16, 32), (torch.bfloat16, 512), (torch.float32, 512)])
def test_cross_attn_deterministic_and_batch_invariant(cases, dtype, C):
    x, p, _ = cases[C]
    a = run_kernel(x, p, dtype, HEADS[C], ld=C + 8, poison=0.0)
    b = run_kernel(x, p, dtype, HEADS[C], ld=C + 8, poison=0.0)
    assert torch.equal(a, b)                                                                  # bit-reproducible across two calls
    for r0 in (0, 192, 448):                                                                  # M = 64 against the same rows inside M = 512
        one = run_kernel(x[r0:r0 + 64], p, dtype, HEADS[C], poison=0.0)
        assert torch.equal(one[:64], a[r0:r0 + 64, :C])


# ---------------------------------------------------------------------------------------------------------------------------------------
# blocks and models
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("tag", ["a", "b"])
def test_crossmod_block_vs_reference(golden, dtype, tag):
    g = golden("crossmod_lewin_block_" + tag)
    C, heads, shift = int(g["C"]), int(g["heads"]), int(g["shift"])
    blk = model.LeWinTransformerBlock(C, (16, 16), heads, win_size=8, shift_size=shift, modulator=(tag == "a"), cross_modulator=True)
    blk.load_state_dict({k[2:]: t(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    blk = blk.cuda().eval()
    with torch.no_grad():
        y = blk(t(g["x"]).cuda(), None, dtype)
        op_check(f"crossmod_lewin_block_{tag}", y, t(g["y"]), dtype)
        assert torch.equal(blk(t(g["x"]).cuda(), None, dtype), y)


def cross_cfg(**kw):
    return dataclasses.replace(spec.arch_config("tiny32", img_size=128), cross_modulator=True, **kw)


def build(cfg, dtype, seed=1234, **kw):
    m = model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                      modulator=cfg.modulator, dd_in=cfg.dd_in, token_mlp=cfg.token_mlp, token_projection=cfg.token_projection,
                      cross_modulator=cfg.cross_modulator, compute_dtype=dtype, **kw)
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
def test_crossmod_model_vs_reference(golden, dtype, tag):
    g = golden("crossmod_model_tiny32_" + tag)
    m = build(cross_cfg(), dtype, int(g["seed"])).eval()
    x = spec.synth_input(int(g["B"]), int(g["H"]), int(g["W"]), int(g["in_seed"]))
    with torch.no_grad():
        model_compare("crossmod_model_tiny32_" + tag, m(x.cuda()), t(g["y"]), dtype)


def test_crossmod_model_paths_are_bit_equal():
    """A GraphedForward replay, a PipelinedForward run, the two-part batch 8 and the mask path (module by module; an all-zero mask adds 0 to every
    logit) against the plain one-call forward of the same model; infer.restore on both canvases; a real mask against the composition.

    The mask path is bit-equal where a block's window attention takes the same route with and without a mask: token_projection='conv' (always the
    three-launch route), the model tests/test_gpu_convproj.py makes this check on.  There the cross kernel is the only part of a decoder block that
    the one-call forward (rows of the concat buffer) and the block-by-block forward (uf_cross_attn_fwd, then uf_lewin_block_fwd) could run differently.
    A 'linear' model's window attention leaves its fused kernel under a mask (with or without the cross-modulator), so its zero-mask forward is held
    to the whole-model gate instead."""
    from uformer_amd import infer
    cfg = cross_cfg()
    m = build(cfg, torch.bfloat16, 31).eval()
    xs = [spec.synth_input(2, 128, 128, 60 + i).cuda() for i in range(2)]
    zero = torch.zeros(2, 1, 128, 128, device="cuda")
    with torch.no_grad():
        plain = [m(xx).clone() for xx in xs]
        assert torch.equal(m(xs[1]), plain[1]) and not torch.equal(plain[0], plain[1])
        gf = infer.GraphedForward(m, xs[0])
        for xx, y in zip(xs, plain):
            assert torch.equal(gf(xx), y)
        pf = infer.PipelinedForward(m, depth=2)
        for y, want in zip(pf.map(xs), plain):
            assert torch.equal(y, want)
        x8 = torch.cat([xs[0], xs[1], xs[1], xs[0]], 0)                                       # B = 8: two half-batch parts on two streams
        assert torch.equal(m(x8), torch.cat([plain[0], plain[1], plain[1], plain[0]], 0))
        model_compare("crossmod_zero_mask", m(xs[0], zero), plain[0].cpu(), torch.bfloat16)
        mc = build(cross_cfg(token_projection="conv"), torch.bfloat16, 31).eval()
        assert torch.equal(mc(xs[0], zero), mc(xs[0]))
        for canvas in ("square", "rect"):                                                     # 100 x 200 -> 256 x 256 or 128 x 256
            r = infer.restore(m, torch.cat([xs[0], xs[1]], 3)[:1, :, :100, :200], canvas=canvas)
            assert r.shape == (1, 3, 100, 200) and torch.isfinite(r).all()
        mf = build(cfg, torch.float32, 11).eval()
        x = spec.synth_input(1, 128, 128, 12)
        mask = (torch.rand(1, 1, 128, 128, generator=gen(5)) > 0.3).float()
        ref = XC.uformer_forward(x, spec.synth_state_dict(cfg, 11), img_size=128, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, mask=mask)
        model_compare("crossmod_usermask", mf(x.cuda(), mask.cuda()), ref, torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kw", [dict(token_mlp="ffn"), dict(token_projection="conv")], ids=["ffn", "conv"])
def test_cross_modulator_with_the_other_ablations(kw, dtype):
    cfg = cross_cfg(**kw)
    m = build(cfg, dtype, 21).eval()
    x = spec.synth_input(1, 128, 128, 22)
    with torch.no_grad():
        ref = XC.uformer_forward(x, spec.synth_state_dict(cfg, 21), img_size=128, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads)
        model_compare("crossmod_with_" + "_".join(kw.values()), m(x.cuda()), ref, dtype)


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


def test_models_without_the_flag_never_reach_the_cross_kernel():
    x = spec.synth_input(1, 128, 128, 3).cuda()
    lin = spec.arch_config("tiny32", img_size=128)
    ml = model.Uformer(img_size=128, embed_dim=32, depths=list(lin.depths), num_heads=list(lin.num_heads), modulator=True, compute_dtype=torch.bfloat16)
    ml.load_state_dict(spec.synth_state_dict(lin, 1234), strict=True)
    ml = ml.cuda().eval()
    names, y_timed = kernel_names(ml, x)
    assert names and not any(n.startswith("cross_attn") for n in names) and any(n.startswith("attn_block") for n in names), names
    pk = ml._get_packed(x.device)
    assert pk.cross is None and not pk.desc.cross                                             # the appended field is NULL ...
    with torch.no_grad():
        assert torch.equal(ml(x), y_timed)                                                    # ... and the forward is the same bits, timed or not
    cfg = cross_cfg()
    names, _ = kernel_names(build(cfg, torch.bfloat16).eval(), x)
    assert sum(n.startswith("cross_attn") for n in names) >= 4, names                         # one kernel class per decoder stage
    assert any(n.startswith("attn_block") for n in names), names                              # the window attention keeps its fused kernel
