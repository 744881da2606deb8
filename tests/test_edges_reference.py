"""CPU checks that keep the gates of tests/test_gpu_edges.py honest: every generator gives finite float64 references with the
property its class names, every emulation with its switches off IS the reference, and no emulation's error exceeds the rounding
unit of its type times the class's condition number -- a broken emulation would otherwise silently loosen a GPU gate."""
import math

import pytest
import torch

import edge_cases as E

TYPES = [E.F32, E.BF16, E.F16]
EPS32 = torch.finfo(torch.float32).eps


def test_poisoned_view_round_trips():
    for dtype in TYPES:
        for mode in ("guard", "strided", "cat", "cat_left"):
            p = E.PoisonedView(12, 32, dtype, mode)
            assert p.view.shape == (12, 32) and p.view.data_ptr() % 16 == 0 and p.ld % 4 == 0
            assert p.guard_intact() and torch.isnan(p.live().float()).all()
            src = torch.randn(12, 32).to(dtype)
            p.fill(src)
            assert torch.equal(p.live(), src) and p.guard_intact()
            p.view[3, 5] = 2.0                                              # the view aliases the buffer
            assert float(p.buf[E.GUARD_ROWS // 2 + 3, p.col + 5]) == 2.0 and p.guard_intact()
            # a planted write just outside the view, on every side, is found
            for r, c in ((E.GUARD_ROWS // 2 - 1, p.col), (E.GUARD_ROWS // 2 + 12, p.col + 31)) + \
                    (((E.GUARD_ROWS // 2, p.col - 1),) if p.col else ()) + (((E.GUARD_ROWS // 2 + 11, p.col + 32),) if p.ld > p.col + 32 else ()):
                keep = p.bits[r, c].item()
                p.buf[r, c] = 1.0
                assert not p.guard_intact(), (mode, r, c)
                p.bits[r, c] = keep
                assert p.guard_intact()
    plain = E.PoisonedView(4, 16, E.F32, "plain")
    assert plain.buf.shape == (4, 16) and plain.guard_intact()
    ws, guard = E.poisoned_bytes(256, 64, 0xFF, "cpu")
    assert ws.numel() == 320 and bool((ws[:256] == 0xFF).all()) and bool((guard == 0xA5).all())
    assert torch.isnan(ws[:256].view(torch.float32)).all() and torch.isnan(ws[:256].view(torch.bfloat16).float()).all() and torch.isnan(ws[:256].view(torch.float16).float()).all()


@pytest.mark.parametrize("C", E.LN_CS)
@pytest.mark.parametrize("cls", E.LN_CLASSES)
def test_layernorm_classes(cls, C):
    x = E.ln_rows(cls, C)
    gamma, beta = E.ln_affine(C)
    ref = E.ln_ref(x, gamma, beta)
    assert x.shape == (E.LN_ROWS, C) and torch.isfinite(ref).all()
    xd = x.double()
    if cls == "constant":
        assert bool((xd.var(-1, unbiased=False) == 0).all())
        assert torch.equal(ref, beta.double().expand_as(ref))            # variance 0: the output is beta
    if cls == "mean1e3_std1":
        assert float((xd.mean(-1).abs() / xd.std(-1)).min()) > 500
    if cls == "mean100_std1e-2":
        assert float((xd.mean(-1).abs() / xd.std(-1)).min()) > 5000
    if cls == "outlier1e4":
        assert bool(((xd == 1e4).sum(-1) == 1).all())
    if cls == "tiny1e-6":
        assert float(xd.var(-1, unbiased=False).max()) < 1e-5 * 1e-5      # eps dominates the variance
    assert float(E.row_err(E.ln_emu(x, gamma, beta, None), ref).max()) <= 1e-6
    if cls == "constant":                                                # the emulation keeps the property too: only the output rounding is left
        assert torch.equal(E.ln_emu(x, gamma, beta, E.F32), beta.expand_as(ref))
    cond = E.ln_condition(x)
    for dtype in TYPES:
        err = float(E.row_err(E.ln_emu(x, gamma, beta, dtype), ref).max())
        # one output rounding (unit of T, relative to the row's largest value) + float32 statistics: the mean and the centred
        # values carry a few eps32 of max|x|, amplified by rstd = the condition number
        bound = (0 if dtype == E.F32 else 1.01 * E.unit(dtype)) + 4 * EPS32 * (cond + 2)
        assert math.isfinite(err) and err <= bound, (cls, C, dtype, err, bound)


@pytest.mark.parametrize("C", E.LN_CS)
@pytest.mark.parametrize("cls", E.LN_CLASSES)
def test_layernorm_backward_classes(cls, C):
    x = E.ln_rows(cls, C)
    gamma, _ = E.ln_affine(C)
    dy = torch.randn(E.LN_ROWS, C, generator=torch.Generator().manual_seed(C))
    ref = E.ln_bwd_ref(x, gamma, dy)
    emu = E.ln_bwd_ref(x, gamma, dy, torch.float32)
    cond = E.ln_condition(x)
    for r, e in zip(ref, emu):
        assert torch.isfinite(r).all() and torch.isfinite(e).all()
    err = float(E.row_err(emu[0], ref[0]).max())
    # xhat carries eps32 * cond * log2(C); dx subtracts two projections of size ~|g dy| sqrt(C) from it
    assert err <= 8 * EPS32 * (cond + 2) * C ** 0.5, (cls, C, err)


@pytest.mark.parametrize("cls", E.GELU_CLASSES)
def test_gelu_classes(cls):
    for dtype in TYPES:
        x = E.gelu_grid(cls, dtype)
        assert x.shape == (64, E.GELU_ROW) and torch.isfinite(x).all() and torch.equal(x, x.to(dtype).float())
        lim = 40 if cls == "wide40" else 4
        assert float(x.abs().amax(-1).min()) >= 0.9 * lim                  # every row spans the range
        assert bool((x == 0).any()) and bool(((x == 0) & torch.signbit(x)).any())
        assert bool(((x < -8.4) & (x > -8.6)).any()) and bool(((x > -8.4 - 1e-6) & (x < -8.2)).any())
        if cls == "wide40":
            big = float(torch.tensor(65504.0).to(dtype))                    # the largest finite f16 value, snapped to T (bf16: 65536)
            assert bool((x == big).any()) and bool((x == -big).any())
        ref, gref = E.gelu_ref(x, dtype), E.gelu_grad_ref(x, dtype)
        assert torch.isfinite(ref).all() and torch.isfinite(gref).all()
        # the derivative formula is the derivative of the forward formula (central differences in float64)
        xs = x.double()[x.abs() < 30]
        h = 1e-6
        fd = (E.gelu_ref(xs + h, dtype) - E.gelu_ref(xs - h, dtype)) / (2 * h)
        assert float((fd - E.gelu_grad_ref(xs, dtype)).abs().max()) < 1e-7
        # sigmoid form against erf form: the distance uf_common.h states (4.8e-4 for GELU, 8.7e-4 for GELU')
        core = x[x.abs() < 100]
        assert float((E.gelu_ref(core, E.BF16) - E.gelu_ref(core, E.F32)).abs().max()) <= 4.8e-4
        assert float((E.gelu_grad_ref(core, E.BF16) - E.gelu_grad_ref(core, E.F32)).abs().max()) <= 8.7e-4
        dy = torch.ones_like(x)
        err = float(E.row_err(E.gelu_emu(x, dtype), ref).max())
        gerr = float(E.row_err(E.gelu_grad_emu(x, dy, dtype), gref).max())
        # float32 evaluation: u = x (A + B x^2) carries 3 eps32 |u|, 2^u turns that into a relative error ln2 |u| 3 eps32 where the
        # sigmoid is not yet saturated (|u| < 32); the erf form's cancellation 1 + erf for x < 0 costs up to eps32 / (1 + erf) until GELU underflows
        # relative to a row's largest value the condition number is 1: one output rounding + a few eps32 of evaluation
        bound = (0 if dtype == E.F32 else 1.01 * E.unit(dtype)) + 4 * EPS32
        assert math.isfinite(err) and err <= bound, (cls, dtype, err, bound)
        assert math.isfinite(gerr) and gerr <= bound, (cls, dtype, gerr, bound)
    x = E.gelu_grid(cls, E.BF16)
    assert float(E.row_err(E.gelu_emu(x, None), E.gelu_ref(x, E.BF16)).max()) <= 1e-6
    assert float(E.row_err(E.gelu_grad_emu(x, torch.ones_like(x), None), E.gelu_grad_ref(x, E.BF16)).max()) <= 1e-6


@pytest.mark.parametrize("heads,hd", [(1, 16), (4, 16), (1, 32), (4, 32), (1, 64), (4, 64)])
@pytest.mark.parametrize("cls", E.ATT_CLASSES)
def test_attention_classes(cls, heads, hd):
    for dtype in TYPES:
        case = E.attention_case(cls, heads, hd, dtype)
        assert float(case["q"].float().abs().max()) <= 64 and float(case["k"].float().abs().max()) <= 64
        s = E.attention_logits(case)
        p = torch.softmax(s, -1)
        ref = E.attention_ref(case)
        assert torch.isfinite(ref).all() and ref.shape == (E.ATT_NW * 64, heads * hd)
        if cls == "one_hot":
            assert float(p.amax(-1).min()) > 1 - 1e-9
        if cls == "uniform":
            assert torch.equal(p, torch.full_like(p, 1 / 64))
        if cls == "bias30":
            assert bool((case["bias"].abs() == 30).all())
        if cls == "shift_user_mask":
            both = E.shift_mask(E.ATT_H, E.ATT_W, 4).unsqueeze(1) + case["mask"].double().unsqueeze(1)
            assert float(both.min()) == -200 and case["shift"] == 4     # some pairs carry both masks, added
            assert bool(((both == 0).sum(-1) > 0).all())
        if cls == "masked_keys_win":
            masked = case["mask"][0, 0] != 0
            assert float((s[..., masked].amin(-1) - s[..., ~masked].amax(-1)).min()) >= 55
            assert float(p[..., ~masked].sum(-1).max()) < 1e-20
        assert float(E.row_err(E.attention_emu(case, None), ref).max()) <= 1e-6
        err = float(E.row_err(E.attention_emu(case, dtype), ref).max())
        cond = E.attention_condition(case)
        # p and o rounded to T (a row of p.v inherits at most sqrt-ish of 64 independent roundings: bounded by 2 units), float32 logits
        # ... times the cancellation of the row's product: sum_j p_j |v_j| over the largest |o| of the row
        vabs = case["vt"].double().transpose(-1, -2).abs()
        kappa = float(((p @ vabs).amax(-1) / (p @ case["vt"].double().transpose(-1, -2)).abs().amax(-1)).max())
        bound = ((0 if dtype == E.F32 else 2 * E.unit(dtype)) + 2 * EPS32 * (cond + 1)) * kappa
        assert math.isfinite(err) and err <= bound, (cls, dtype, err, bound)


@pytest.mark.parametrize("cls", E.ATT4_CLASSES)
def test_attention4_classes(cls):
    for dtype in TYPES:
        case = E.attention4_case(cls, 2, 32, dtype)
        assert case["qkv"].shape == (64, 192) and float(case["qkv"].float().abs().max()) <= 64
        ref, p = E.attention4_ref(case)
        assert torch.isfinite(ref).all()
        if cls == "one_hot":
            assert float(p.amax(-1).min()) > 1 - 1e-9
        if cls == "uniform":
            assert torch.equal(p, torch.full_like(p, 1 / 16))
        if cls == "bias30":
            assert bool((case["rpb4"].abs() == 30).all())
        assert float(E.row_err(E.attention4_emu(case, None), ref).max()) <= 1e-6
        err = float(E.row_err(E.attention4_emu(case, dtype), ref).max())
        bound = (0 if dtype == E.F32 else 2 * E.unit(dtype)) + 2 * EPS32 * (1 + float(p.amax(-1).log().abs().max()) + 60 * 64)   # eps32 |logit|, |q.k| <= 60 * 64
        assert math.isfinite(err) and err <= bound, (cls, dtype, err)


@pytest.mark.parametrize("heads,hd", [(1, 16), (4, 16), (1, 32), (4, 32), (1, 64), (4, 64)])
@pytest.mark.parametrize("cls", E.ATT_CLASSES)
def test_attention_backward_classes(cls, heads, hd):
    do = torch.randn(E.ATT_NW * 64, heads * hd, generator=torch.Generator().manual_seed(hd))
    for dtype in TYPES:
        case = E.attention_case(cls, heads, hd, dtype)
        ref = E.attention_bwd(case, do.to(dtype), None)
        emu = E.attention_bwd(case, do.to(dtype), dtype)
        off = E.attention_bwd(case, do.to(dtype), E.F32, dt=torch.float64)     # the emulation's own path (exp2, kernel-order sums), no rounding
        conds, amps = E.attention_bwd_condition(case, do.to(dtype))
        sub = 2.0 ** -25 if dtype == E.F16 else 0.0                          # half a step of f16's subnormal grid
        smax = float(E.attention_logits(case).abs().max())
        for name, r_, e_, o_, c_, a_ in zip(("dq", "dk", "dv", "dbias"), ref, emu, off, conds, amps):
            assert torch.isfinite(r_).all() and torch.isfinite(e_).all()
            assert float(E.row_err(o_, r_).max()) <= 1e-6 * float(c_.max()), (name, cls)
            # per row: (operand + output roundings of T, float32 logits / exp / sums) x the row's condition number
            per_row = ((0 if dtype == E.F32 or name == "dbias" else 3 * E.unit(dtype)) + 16 * EPS32 * (2 + smax)) * c_ + sub * a_
            err = E.row_err(e_, r_)
            assert bool((err <= per_row).all()), (name, cls, dtype, float((err / per_row).max()))
        # the reference is autograd's gradient (float64) of sum(o * dO)
        q = case["q"].double().requires_grad_(True)
        k = case["k"].double().requires_grad_(True)
        v = case["vt"].double().transpose(-1, -2).contiguous().requires_grad_(True)
        bias = case["bias"].double().requires_grad_(True)
        s = q @ k.transpose(-1, -2) + bias.unsqueeze(0)
        if case["shift"]:
            s = s + E.shift_mask(E.ATT_H, E.ATT_W, case["shift"]).unsqueeze(1)
        if case["mask"] is not None:
            s = s + case["mask"].double().unsqueeze(1)
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(E.ATT_NW * 64, -1)
        (o * do.to(dtype).double()).sum().backward()
        for r_, a_ in zip(ref, (q.grad, k.grad, v.grad, bias.grad)):
            assert float((r_ - a_).abs().max()) <= 1e-9 * max(1.0, float(a_.abs().max()))


@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("cls", E.LN_CLASSES)
def test_block_on_layernorm_classes(cls, C):
    """the whole-block reference and emulation of test_lewin_block_hard_layernorm_rows (CPU weights: the same module class, no GPU)"""
    from oracle import uformer_oracle as O
    from uformer_amd import spec
    heads = max(1, C // 32)
    g = torch.Generator().manual_seed(C)
    hid = 4 * C
    sd = {"norm1.weight": 1 + 0.1 * torch.randn(C, generator=g), "norm1.bias": 0.1 * torch.randn(C, generator=g),
          "norm2.weight": 1 + 0.1 * torch.randn(C, generator=g), "norm2.bias": 0.1 * torch.randn(C, generator=g),
          "modulator.weight": 0.1 * torch.randn(64, C, generator=g),
          "attn.relative_position_bias_table": 0.1 * torch.randn(225, heads, generator=g), "attn.relative_position_index": spec.relative_position_index(8),
          "attn.qkv.to_q.weight": torch.randn(C, C, generator=g) / C ** 0.5, "attn.qkv.to_q.bias": 0.1 * torch.randn(C, generator=g),
          "attn.qkv.to_kv.weight": torch.randn(2 * C, C, generator=g) / C ** 0.5, "attn.qkv.to_kv.bias": 0.1 * torch.randn(2 * C, generator=g),
          "attn.proj.weight": torch.randn(C, C, generator=g) / C ** 0.5, "attn.proj.bias": 0.1 * torch.randn(C, generator=g),
          "mlp.linear1.0.weight": torch.randn(hid, C, generator=g) / C ** 0.5, "mlp.linear1.0.bias": 0.1 * torch.randn(hid, generator=g),
          "mlp.dwconv.0.weight": torch.randn(hid, 1, 3, 3, generator=g) / 3, "mlp.dwconv.0.bias": 0.1 * torch.randn(hid, generator=g),
          "mlp.linear2.0.weight": torch.randn(C, hid, generator=g) / hid ** 0.5, "mlp.linear2.0.bias": 0.1 * torch.randn(C, generator=g)}
    x = E.ln_rows(cls, C).reshape(2, 64, C)
    cond = E.ln_condition(x.reshape(-1, C))
    for dtype in TYPES:
        p = E.block_params(sd, dtype)
        ref = E.block_ref(x, p, heads, dtype)
        assert torch.isfinite(ref).all()
        if dtype == E.F32:                                              # switches off: the float64 oracle block itself
            prefix = {"blk." + k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}
            ora = O.lewin_block(x.double(), prefix, "blk.", heads, 0)
            assert float(E.row_err(E.block_emu(x, p, heads, None).reshape(-1, C), ora.reshape(-1, C)).max()) <= 1e-6
        err = float(E.row_err(E.block_emu(x, p, heads, dtype).reshape(-1, C), ref.reshape(-1, C)).max())
        # the two branches relative to the row's largest output value; nine rounding points of T along them; float32 LayerNorm statistics
        branch = float(((ref - x.double()).abs().amax(-1) / ref.abs().amax(-1)).max())
        bound = (0 if dtype == E.F32 else 16 * E.unit(dtype)) * max(branch, 1e-3) + 64 * EPS32 * (cond + 2)
        assert math.isfinite(err) and err <= bound, (cls, C, dtype, err, bound)
