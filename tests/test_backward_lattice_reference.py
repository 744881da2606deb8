"""CPU: the constructions of tests/backward_lattice.py -- every condition on the references alone, a float32 emulation of every formula against its
reference to the bit, the references under the faults an exact gate must see, and which of those faults the present gates of tests/test_gpu_bwd.py let
through on Gaussian inputs.  No GPU; tests/test_gpu_backward_exact.py runs the same cases through the kernels."""
import math

import pytest
import torch

import backward_lattice as L
import exact_lattice as X
from exact_lattice import BF16, F32, MODES, TAG

def bits_equal(a, b):
    return a.dtype == b.dtype and torch.equal(X._bits(a), X._bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# conditions (asserted by the builders) and float32 emulations
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.ATTN_BWD_CASES, ids=str)
def test_attention_conditions_and_f32_emulation(case):
    """the builder asserts: winners and their lead (>= MARGIN), P the lattice value, P and dS T values, every contraction below 2^24 steps, dot live on at
    least half the rows, dq = dk = 0 under one-hot (asserted equal to zero), dq live under tie where the winners' k rows differ, the sign structure of "uniform".  Then the float32 emulation
    of the kernels' softmax algebra equals the float64 reference rounded once, in every type."""
    c = L.attn_bwd_case(*case)
    for dtype in MODES:
        e = L.attn_bwd_emulate_f32(c, dtype)
        for key in ("dq", "dk", "dvt", "dbias"):
            t = F32 if key == "dbias" else dtype
            assert bits_equal(e[key].to(t), c["ref"][key].to(t)), (case, TAG[dtype], key)
        # the reference with the operand roundings of the 2-byte kernels is the unrounded one: P and dS are T values
        r = L.attn_bwd_eval(c, dtype)
        assert all(torch.equal(r[k], c["ref"][k]) for k in ("dq", "dk", "dvt", "dbias"))
    assert torch.equal(L.rpb_table_grad64(c["ref"]["dbias"]).sum(0), c["ref"]["dbias"].sum((1, 2)))
    hd, C = case[4], case[3] * case[4]
    assert torch.equal(c["dqkv"][:, C:2 * C], L.merge_heads(c["ref"]["dk"])) and c["dqkv"].shape == (c["n"] * 64, 3 * C)
    if hd != 32:                                                   # the query scale is a power of two at head widths 16 and 64
        assert torch.equal(c["dqkv"][:, :C], L.merge_heads(c["ref"]["dq"]) * hd ** -0.5)


def test_attention_case_list_reaches_every_launch_form():
    seen = {(hd, kind, shift, masked) for (_, _, _, _, hd, shift, kind, masked) in L.ATTN_BWD_CASES}
    for hd in (16, 32, 64):
        for kind in L.KINDS:
            assert (hd, kind, 0, False) in seen and (hd, kind, 4, False) in seen
        assert (hd, "uniform", 0, True) in seen and (hd, "onehot", 0, True) in seen
    assert {c[3] for c in L.ATTN_BWD_CASES} >= {1, 2, 4, 16}
    chunked = [c for c in L.ATTN_BWD_CASES if c[0] * (c[1] // 8) * (c[2] // 8) > 1024 // c[3]]
    assert len(chunked) == 2 and all(c[3] == 16 for c in chunked), "a workgroup must walk several windows of a chunk"


@pytest.mark.parametrize("case", L.ATTN4_BWD_CASES, ids=str)
def test_attention4_conditions_and_f32_emulation(case):
    c = L.attn4_bwd_case(*case)
    e = L.attn4_bwd_emulate_f32(c)
    r = c["ref"]
    assert bits_equal(e["dS"], r["dS"].float()) and bits_equal(e["dv"], r["dv"].float())
    assert bits_equal(e["dq"], L.scaled_f32(r["dq"], c["scale"])) and bits_equal(e["dk"], L.scaled_f32(r["dk"], c["scale"]))
    assert torch.equal(c["dtable"].sum(0), r["dS"].sum((0, 2, 3)))


@pytest.mark.parametrize("C,rows", L.LN_PLAIN_CASES)
def test_layernorm_conditions_and_f32_emulation(C, rows):
    """eps disappears in float32(a^2 + eps) for every amplitude (asserted by the builder, with s1 and s2 live); the float32 emulation WITH eps equals the
    float64 lattice reference (rstd := 1 / a) to the bit; that reference differs from the float64 formula with eps by under 1e-7 relative"""
    c = L.ln_bwd_case(C, rows)
    r, e = L.ln_bwd_eval(c), L.ln_bwd_emulate_f32(c)
    for key in r:
        assert bits_equal(e[key], r[key].float()) and torch.equal(r[key].float().double(), r[key]), key
    if rows < 1000:
        x = c["x"].clone().requires_grad_(True)
        gm = c["gamma"].clone().requires_grad_(True)
        bt = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.layer_norm(x, (C,), gm, bt, 1e-5).backward(c["dy"])
        for got, want in ((r["dx"], x.grad), (r["dgamma"], gm.grad), (r["dbeta"], bt.grad)):
            assert float((got - want).abs().max()) <= 1e-7 * float(want.abs().max())
    assert not all(torch.tensor(float(a * a) + 1e-5, dtype=F32) == a * a for a in (8.0,)), "a = 8 must fail the eps condition (it is why the amplitudes start at 16)"


@pytest.mark.parametrize("C", L.LN_WIDTHS)
def test_layernorm_fused_configs(C):
    configs = list(enumerate(L.LN_FUSED_CONFIGS)) + ([(100, L.LN_FUSED_BIG[1])] if C == L.LN_FUSED_BIG[0] else [])
    for ci, (B, H, W, windowed, shift, add, dy_f32, cast, cast_shift, scaled) in configs:
        c = L.ln_bwd_case(C, B * H * W, seed=ci)
        tok = X.window_tokens(B, H, W, shift) if windowed else None
        spec = None if cast is None else (L.cast_rows(B, H, W, cast == "window", cast_shift), L.drops(B) if scaled else None, H * W)
        r = L.ln_bwd_eval(c, tok, add, spec, BF16)
        e = L.ln_bwd_emulate_f32(c, tok, add)
        for key in e:
            assert bits_equal(e[key], r[key].float()), (C, ci, key)
        if cast is not None:
            assert bool(r["cast"].any()) and torch.equal(r["cast"].to(BF16).double(), r["cast"])
            if scaled:                                             # image 0 is dropped (scale 0), image 1 doubled
                dest = spec[0]
                assert not bool(r["cast"][dest[:H * W]].any()) and torch.equal(r["cast"][dest[H * W:2 * H * W]], (2 * r["dx"][H * W:2 * H * W]).to(BF16).double())
    Cb, (Bb, Hb, Wb) = L.LN_FUSED_BIG[0], L.LN_FUSED_BIG[1][:3]
    assert Bb * Hb * Wb > L.LN_GRID * L.rows_per_workgroup(Cb), "the large configuration must take a second trip of the grid-stride loop"
    rows = {L.rows_per_workgroup(C) for C in L.LN_WIDTHS}
    assert rows == {64, 32, 16, 8, 4} and all(130 % r for r in rows if r > 2)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_gelu_grad_classes_and_f32_emulation(dtype):
    """GELU' of the three classes: the documented derivative rounds to 1, 1/2, 0 (asserted by gelu_grad_lattice); the float32 emulation of gelu_grad_t times
    a gradient, stored as T, is the lattice product -- except bf16 at a <= -15, where the clamp's residue stays inside rule (b)"""
    for n in L.GELU_BWD_N:
        c = L.gelu_bwd_case(n, dtype)
        got = L.nz((c["dy"].float() * L.gelu_grad_kernel_f32(c["pre"].float(), dtype)).to(dtype))
        neg = c["pre"] <= L.NEG_MAX
        if dtype == BF16:
            assert bool(((got.double() - c["dx"]).abs()[neg] <= L.gelu_residue_bound(c["dy"], c["pre"])[neg]).all()) and bool((got.double()[neg] != 0).any())
            assert float(neg.double().mean()) <= L.RULE_B_CAP
            got = torch.where(neg, c["dx"].to(dtype), got)
        assert bits_equal(got, c["dx"].to(dtype)), n
    assert float(L.gelu_residue_bound(torch.tensor(2048.0), torch.tensor(-64.0))) < 2.0 ** -24 * 0.5


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_gelu_family_cases(dtype):
    for (M, N, K, _) in L.LINEAR_DGELU_CASES[:4]:
        c = L.linear_dgelu_case(M, N, K, dtype)
        assert bool(c["out"].any()) and torch.equal(c["out"].to(dtype).double(), c["out"])
    for case in L.DW_BWD_CASES:
        d = L.dw_bwd_case(*case, dtype)
        assert min(L.check_classes(d["pre"], dtype)) >= 0.2                      # all three classes in every type
        assert torch.equal(d["dbias"], d["dc"].sum((0, 1, 2)))
        # where a tap gradient is 0 the bf16 kernel may leave the clamp's residue: far below half the lattice step of a non-zero entry (1)
        assert float(L.dw9_residue_bound(d).max()) < 2.0 ** -24


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C", L.LEFF_BWD_CASES[:4] + L.LEFF_BWD_CASES[-1:])
def test_leff_half_conditions(dtype, B, H, W, C):
    """the builder asserts the classes of a1 and c (each at least a fifth), the exactness of every float32 intermediate of the chain and that no output is zero"""
    for dropped in (False, True):
        c = L.leff_bwd_case(B, H, W, C, dtype, dropped)
        assert set(c["refs"]) == {"dx1", "norm2_w", "norm2_b", "w1", "b1", "wdw", "bdw", "w2", "b2"}
        if dropped and B == 3:                                     # image 0 is dropped: only the residual path reaches its rows
            assert torch.equal(c["refs"]["dx1"][:H * W], c["dy"][:H * W])


def attn_half_subset(dtype):
    return [c for c in L.attn_half_cases(dtype) if c[3] in (32, 128, 512)]


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_attention_half_conditions(dtype):
    """the builder asserts: the op-level forward reproduces the block's saturated o, every float32 intermediate of the chain is exact, dS = 0 and dq = dk = 0 under
    one-hot, dk = 0 and dq live under Wq = 0, no other output zero, and (2-byte types) that dxn reaches dx through LayerNorm 1.  The summation bound of the q rows is
    far below the values it holds"""
    for case in attn_half_subset(dtype):
        for dropped in (False, True):
            c = L.attn_half_bwd_case(*case, dtype, dropped)
            C = case[3]
            assert ("modulator" in c["refs"]) == case[6]
            if case[5] == "onehot":
                assert not c["bounds"] and not bool(c["refs"]["wqkv"][:2 * C].any()) and bool(c["refs"]["wqkv"][2 * C:].any())
            else:
                bw = c["bounds"]["wqkv"]
                assert bool((bw[:C] > 0).any()) and not bool(bw[C:].any()) and float(bw.max()) < 1e-3 * float(c["refs"]["wqkv"][:C].abs().max())
                assert not bool(c["refs"]["wqkv"][C:2 * C].any()) and bool(c["refs"]["wqkv"][:C].any())
            if case[6]:                                                # the modulator gradient summed over the wrong window axis
                assert not torch.equal(L.modulator_grad_wrong_axis(c, C), c["refs"]["modulator"])


# ---------------------------------------------------------------------------------------------------------------------------
# the references move under the faults; the present gates on Gaussian inputs
# ---------------------------------------------------------------------------------------------------------------------------
ATTN_FAULTS = ["dot48", "p_neighbour", "dbias_second_window", "mask_ignored", "mask_other_window", "dk_unscaled_q", "dv_untransposed"]


def attn_fault(c, dtype, fault):
    if fault == "mask_ignored":
        return L.attn_bwd_eval(c, dtype, mask=torch.zeros_like(c["mask"]))
    if fault == "mask_other_window":
        return L.attn_bwd_eval(c, dtype, mask=c["mask"].roll(1, 0))
    return L.attn_bwd_eval(c, dtype, fault)


def moved(bad, ref, keys):
    return [k for k in keys if not torch.equal(bad[k], ref[k])]


def test_attention_references_move_under_every_fault():
    keys = ("dq", "dk", "dvt", "dbias")
    cases = {"uniform": L.attn_bwd_case(1, 16, 16, 1, 32, 4, "uniform", False), "tie": L.attn_bwd_case(1, 16, 16, 2, 32, 4, "tie", False),
             "onehot": L.attn_bwd_case(1, 16, 16, 4, 32, 4, "onehot", False), "masked": L.attn_bwd_case(1, 16, 16, 2, 32, 0, "uniform", True)}
    seen = {f: {k: moved(attn_fault(c, BF16, f), c["ref"], keys) for k, c in cases.items()} for f in ATTN_FAULTS}
    print(seen)
    assert {"dq", "dk", "dbias"} <= set(seen["dot48"]["uniform"])
    assert seen["p_neighbour"]["tie"] and seen["p_neighbour"]["onehot"]
    assert seen["dbias_second_window"]["uniform"] == ["dbias"] and seen["dbias_second_window"]["tie"] == ["dbias"]
    assert set(seen["mask_ignored"]["uniform"]) == set(keys) and set(seen["mask_ignored"]["masked"]) == set(keys)
    assert seen["mask_other_window"]["uniform"] and seen["mask_other_window"]["masked"]
    assert seen["dk_unscaled_q"]["uniform"] == ["dk"] and seen["dk_unscaled_q"]["tie"] == ["dk"]
    assert seen["dv_untransposed"]["tie"] == ["dvt"] and seen["dv_untransposed"]["onehot"] == ["dvt"]
    c4 = L.attn4_bwd_case(1, 8, 8, 5, 32, "tie")
    for f in ("dot48", "p_neighbour", "dv_untransposed"):
        bad = L.attn4_bwd_eval(c4, f)
        assert any(not torch.equal(bad[k], c4["ref"][k]) for k in ("dq", "dk", "dv", "dS")), f


def test_layernorm_references_move_under_every_fault():
    B, H, W, C = 3, 8, 24, 64
    c = L.ln_bwd_case(C, B * H * W, seed=3)
    tok = X.window_tokens(B, H, W, 4)
    spec = (L.cast_rows(B, H, W, True, 4), L.DROPS, H * W)
    ref = L.ln_bwd_eval(c, tok, True, spec, BF16)
    for fault, key in (("dgamma_row_lane", "dgamma"), ("s2_dropped", "dx"), ("add_at_window_row", "dx"), ("cast_scale_neighbour", "cast")):
        bad = L.ln_bwd_eval(c, tok, True, spec, BF16, fault)
        assert not torch.equal(bad[key], ref[key]), fault
    assert not torch.equal(L.ln_bwd_eval(c, tok, True, spec, BF16, "dgamma_row_lane")["dbeta"], ref["dbeta"])


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_gelu_references_move_under_every_fault(dtype):
    c = L.gelu_bwd_case(L.GELU_BWD_N[1], dtype)
    for k in (1, 2):                                               # class 0 has GELU' = 1: skipping it is no fault; classes 1 and 2 must show
        assert not torch.equal(L.mul_dgelu(c["dy"], c["pre"], dtype, skip=k), c["dx"]), k
    d = L.dw_bwd_case(2, 16, 16, 32, dtype)
    assert not torch.equal(L.dw_bwd_eval(d, dtype, "taps_unflipped")["da"], d["da"])
    bad = L.dw_bwd_eval(d, dtype, "h_not_gelu")
    assert not torch.equal(bad["dw9"], d["dw9"]) and torch.equal(bad["da"], d["da"])
    for k in (1, 2):
        assert not torch.equal(L.dw_bwd_eval(d, dtype, skip=k)["da"], d["da"])


def rel(got, ref):
    return float((got - ref).abs().max()) / max(1e-12, float(ref.abs().max()))


def test_which_faults_the_present_gates_pass_on_gaussian_inputs():
    """tests/test_gpu_bwd.py gates the op-level backward at 2.5e-2 of the largest reference magnitude for bf16 operands (2e-4 for the f32 LayerNorm backward), on
    Gaussian inputs.  The same faults on such inputs (8 / 64 windows of 2 heads of 32, shift 4 on 16 x 16 maps; LayerNorm 257 / 4096 rows of 64; GELU 9600 elements):
    largest error over largest |reference|, measured here, and what a gate of 2.5e-2 does with it:
      dot over 48 of 64 keys, every row              dq 0.85   dk 0.67   dbias 0.84     caught
      dot over 48 keys in ONE wave's 16 rows of one window and head        dq 0.053 (8 windows), 0.046 (64)     caught, by a factor of two
      dS with P of the neighbouring row              1.5                                caught
      dbias without the second window                0.64 (8 windows)   0.28 (64)       caught
      dbias without ONE wave's slice of that window  0.56 (8 windows)   0.13 (64)       caught; falls with the window count (a model step has thousands)
      shift mask ignored / of another window         0.77 ... 1.04                      caught
      dk with the unscaled q                         4.7                                caught
      dv with P untransposed                         1.1                                caught
      s2 dropped (f32 gate 2e-4)                     0.22                               caught
      dgamma without one row                         0.080 (257 rows)   0.023 (4096)    PASSES 2.5e-2 at 4096 rows; caught by the 2e-4 the f32 test has
      GELU' skipped for a <= -3 / |a| <= 1/16        0.81 / 0.29                        caught
      GELU' skipped for a >= 3                       0.0068                             PASSES
    So on Gaussian inputs the max-norm gates see every fault that moves SOME output by 2.5 % of the largest one, which these stand-ins mostly do; they pass what is
    bounded by construction (a derivative that is almost 1, one row of thousands) and lose a factor with every reduction the fault is diluted in (windows per dbias
    entry, rows per dgamma entry) -- at the sizes of a training step rather than of a test.  The lattice gate is zero at every size.  Asserted: this table."""
    gate = 2.5e-2
    seen = {}
    for n in (8, 64):
        g = torch.Generator().manual_seed(17)
        heads, hd, H = 2, 32, 16
        rn = lambda *s: torch.randn(*s, generator=g).to(BF16).double()             # noqa: E731
        c = {"q": rn(n, heads, 64, hd) * hd ** -0.5, "k": rn(n, heads, 64, hd), "v": rn(n, heads, 64, hd), "dO": rn(n, heads, 64, hd),
             "bias": 0.3 * torch.randn(heads, 64, 64, generator=g).double(), "mask": L.total_mask(n, H, H, 4, None), "hd": hd}
        ref = L.attn_bwd_eval(c, BF16)
        if n == 8:
            for f in ATTN_FAULTS:
                bad = attn_fault(c, BF16, f)
                seen[f] = max(rel(bad[k], ref[k]) for k in ("dq", "dk", "dvt", "dbias") if not torch.equal(bad[k], ref[k]))
        slice_lost = ref["dbias"].clone()
        slice_lost[0, 16:32] -= ref["dS"][1, 0, 16:32]
        seen[f"dbias_wave_slice_{n}"] = rel(slice_lost, ref["dbias"])
        dq = ref["dq"].clone()
        dq[1, 0, 16:32] = L.attn_bwd_eval(c, BF16, "dot48")["dq"][1, 0, 16:32]
        seen[f"dot48_one_wave_{n}"] = rel(dq, ref["dq"])
    for rows in (257, 4096):
        g = torch.Generator().manual_seed(3)
        x, gm, dy = torch.randn(rows, 64, generator=g).double() * 1.7 + 0.3, 1 + 0.1 * torch.randn(64, generator=g).double(), torch.randn(rows, 64, generator=g).double()
        mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
        xhat, rstd = (x - mu) / torch.sqrt(var + 1e-5), 1 / torch.sqrt(var + 1e-5)
        g_ = dy * gm
        dx = (g_ - g_.mean(1, keepdim=True) - xhat * (g_ * xhat).mean(1, keepdim=True)) * rstd
        seen[f"s2_dropped_{rows}"] = rel((g_ - g_.mean(1, keepdim=True)) * rstd, dx)
        dgam = (dy * xhat).sum(0)
        seen[f"dgamma_one_row_{rows}"] = rel(dgam - (dy * xhat)[17], dgam)
    g = torch.Generator().manual_seed(5)
    a, dyg = (2 * torch.randn(9600, generator=g)).to(BF16).double(), torch.randn(9600, generator=g).to(BF16).double()
    gp = L.gelu_grad_doc64(a, F32)
    good = (dyg * gp).to(BF16).double()
    for name, m in (("neg", a <= -3), ("zero", a.abs() <= 1 / 16), ("pos", a >= 3)):
        seen["gelu_skip_" + name] = rel((dyg * torch.where(m, torch.ones_like(gp), gp)).to(BF16).double(), good)
    print({k: round(v, 4) for k, v in seen.items()})
    passes = {k for k, v in seen.items() if v <= gate}
    assert passes == {"gelu_skip_pos", "dgamma_one_row_4096"}, passes
    assert seen["dgamma_one_row_4096"] > 2e-4 and seen["s2_dropped_257"] > 2e-4                  # the f32 gate of test_layernorm_bwd catches both
    assert seen["dbias_wave_slice_64"] < seen["dbias_wave_slice_8"] / 3 and seen["dot48_one_wave_64"] < 3 * gate
    assert math.isfinite(sum(seen.values()))
