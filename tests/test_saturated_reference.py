"""CPU: the facts, the conditions and the fault sensitivity behind tests/test_gpu_saturated.py (tests/saturated_lattice.py has the argument).

  1. the three saturation facts, with float32 emulation of the kernels' formulas (GELU, LayerNorm, softmax);
  2. every condition of every GPU case, for every type (the case builders assert them on the float64 reference);
  3. the reference MOVES under each fault it is built for (stand-ins of faulty kernels, in the style of tests/test_exact_reference.py), and the
     relative gate of the existing op tests lets the bounded ones through on the same inputs: the gap this file closes.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import exact_lattice as X
import saturated_lattice as S
from exact_lattice import BF16, F16, F32, MODES, TAG

BF16_REL = 0.025                                                          # the op gate of tests/test_gpu_ops.py for a bf16 kernel


def old_gate_passes(got, ref):
    return float((got.double() - ref.double()).abs().max()) <= BF16_REL * max(1.0, float(ref.abs().max()))


def moved(bad, ref, dtype=F32):
    """the fault changes at least one element of the output as stored"""
    return not torch.equal(X._bits(bad.to(dtype)), X._bits(ref.to(dtype)))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the facts
# ---------------------------------------------------------------------------------------------------------------------------
def test_gelu_saturates_in_the_kernels_own_arithmetic():
    pos, neg = torch.arange(6, 257, dtype=F32), -torch.arange(11, 257, dtype=F32)
    for dtype in (BF16, F16):
        assert torch.equal(S.gelu_kernel_f32(pos, dtype), pos)                                            # denominator 1.0f
        g = S.gelu_kernel_f32(neg, dtype)
        assert bool((g == 0).all()) and bool(torch.signbit(g).all())                                      # exp2 -> inf, rcp -> 0, x * 0 = -0
        # the documented form in float64 rounds to the same T values
        assert torch.equal(S.gelu_doc64(pos.double(), dtype).to(dtype).double(), pos.double())
        gd = S.gelu_doc64(neg.double(), dtype).to(dtype)
        assert bool((gd == 0).all()) and bool(torch.signbit(gd).all())
    # between the two ranges bf16 keeps a non-zero value: pre-activations must stay out of (-11, 6)
    mid = -torch.arange(6, 11, dtype=F32)
    assert bool((S.gelu_kernel_f32(mid, BF16).to(BF16) != 0).all())
    assert bool((S.gelu_kernel_f32(torch.arange(1, 5, dtype=F32), BF16) != torch.arange(1, 5, dtype=F32)).all())
    # f32: erff saturates from 8 on
    big = torch.arange(8, 257, dtype=F32)
    assert bool((torch.erf(big * torch.tensor(0.70710678118654752440, dtype=F32)) == 1).all())
    assert torch.equal(S.gelu_kernel_f32(big, F32), big)
    g = S.gelu_kernel_f32(-big, F32)
    assert bool((g == 0).all()) and bool(torch.signbit(g).all())
    # ... but the documented erf form in float64 is a float32 value down to -14.5: the cases use -15
    assert float(S.gelu_doc64(torch.tensor([-11.0], dtype=torch.float64), F32).to(F32)) != 0.0
    gd = S.gelu_doc64(-torch.arange(-S.NEG_MAX, 257, dtype=torch.float64), F32).to(F32)
    assert bool((gd == 0).all()) and bool(torch.signbit(gd).all())
    assert torch.equal(S.gelu_doc64(big.double(), F32).to(F32), big)


@pytest.mark.parametrize("C", [16, 32, 64, 128, 256, 512])
def test_layernorm_of_a_balanced_row_rounds_to_the_lattice(C):
    """float32 emulation of the kernels' LayerNorm on rows a s, every combination of weight, bias and modulator: xn rounded to T is s gamma + beta + mod"""
    h = S.hadamard(C)
    s = torch.cat([h[1:9], -h[C - 8:]], 0)                                                                 # 16 balanced patterns
    worst = 0.0
    for a in S.AMPLITUDES:
        x = (s * a).float()
        assert float(x.sum(1).abs().max()) == 0.0 and torch.equal((x * x).sum(1) / C, torch.full((16,), float(a * a)))
        for gm in (-3, -1, 1, 3):
            for bt in (-2, 0, 2):
                for md in (-2, 0, 2, 4):
                    g, b, m = (torch.full((C,), float(v), dtype=torch.float64) for v in (gm, bt, md))
                    y = S.ln_kernel_f32(x, g, b, m)
                    want = s * gm + bt + md
                    worst = max(worst, float(((y.double() - want) / want).abs().max()))
                    for dtype in (BF16, F16):
                        assert torch.equal(y.to(dtype).double(), want), (a, gm, bt, md, TAG[dtype])
    assert worst <= 1.6e-5 and worst * 16 <= 2.0 ** -12                                                    # 16 x under f16's relative half-ulp
    # f32 stores no xn: with weight 0 the kernels' arithmetic returns bias + modulator exactly
    y = S.ln_kernel_f32((s * 3).float(), torch.zeros(C, dtype=torch.float64), torch.full((C,), 3.0, dtype=torch.float64), torch.full((C,), 4.0, dtype=torch.float64))
    assert bool((y == 7).all())


def test_softmax_saturates():
    log2e = torch.tensor(1.4426950408889634, dtype=F32)
    lose = torch.tensor([-S.MARGIN, -120.0, -124.0, -512.0], dtype=F32)
    assert bool((torch.exp2(lose * log2e) == 0).all()) and bool((torch.exp(lose) == 0).all())           # one-hot: every other e is exactly 0
    assert float(torch.exp(torch.zeros((), dtype=F32))) == 1.0
    masked = torch.exp(torch.tensor(-100.0, dtype=F32))                                                   # behind the shift mask: a float32 subnormal
    assert 0.0 < float(masked) < 1e-40 and float(masked.to(BF16)) == 0.0 and float(masked.to(F16)) == 0.0
    for n in (16, 32, 64):                                                                                # uniform: sum n whether the subnormals flush or not
        total = torch.tensor(float(n), dtype=F32) + (64 - n) * masked
        assert float(total) == n and float(1.0 / total) * n == 1.0
        # a reciprocal that is one ulp off is absorbed by the store of o: o * inv is a T value (steps of 1 / n, at most 192 of them)
        inv = torch.nextafter(1.0 / total, torch.tensor(1.0))
        sums = torch.arange(-192, 193, dtype=F32)
        for dtype in (BF16, F16):
            assert torch.equal((sums * inv).to(dtype).double(), sums.double() / n)
    assert 32 * 20 * 32 ** -0.5 * math.log2(math.e) >= 150                                                # the figure of the argument: A = 20 at head_dim 32, log2 domain


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the conditions of every GPU case
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_conditions_of_every_gpu_case(dtype):
    for M, C in S.LNL1_CASES:
        c = S.lnl1_case(M, C, dtype)
        assert min(c["shares"]) >= 0.25
        X.check_representable(c["pre"], dtype)
        if dtype != F32:
            assert len(c["xn"].unique(dim=0)) >= min(2 * (C - 1), M // 4)                                   # live LayerNorm: the rows differ (the amplitude is normalised away: 2 (C - 1) patterns)
    for B, M, C in S.FFN_CASES:
        c = S.ffn_case(B, M, C, dtype)
        for scale in S.FFN_SCALES:
            out = S.ffn_out(c, B, scale)
            assert torch.equal(out.float().double(), out)
    for case in S.LNQKV_CASES:
        c = S.lnqkv_case(*case, dtype)
        for key in ("q", "k", "vt"):
            assert torch.isfinite(c[key].double()).all()
    for case in S.CONVQKV_CASES:
        if dtype != F32:
            c = S.convqkv_case(*case, dtype)
            assert case[4] > 1 and all(torch.isfinite(c[key].double()).all() for key in ("q", "k", "vt"))
    for case in S.ATTN4_CASES:
        c = S.attn4_case(*case, dtype)
        assert bool((c["v"] % 2 == 1).all()) and torch.equal(c["o"].to(dtype).double(), c["o"])
    for case in S.LEFF2_CASES + [cs for cs, _ in S.LEFF2_WALK_CASES]:
        c = S.leff2_case(*case, dtype)
        assert min(c["shares"]) >= 0.25 and torch.equal(c["out"].float().double(), c["out"])
        assert torch.equal(S.leff2_out(c, dtype=dtype), c["out"])                                         # the stand-in machinery reproduces the reference
    for case in S.ATTN_CASES:
        c = S.attn_case(*case, dtype)
        assert bool((c["vt"] % 2 == 1).all()), "v must be odd"
    # the walk cases do walk: more tiles than the workgroups their forms keep resident (768 at C <= 128 with 2-byte operands, 256 in f32), and every
    # forced form is used where it changes the launch
    for (B, H, W, C), variants in S.LEFF2_WALK_CASES:
        assert C <= 128 and B * (H // 8) * (W // 8) > 768
    assert S.LEFF2_WALK_CASES[0][0][3] == 32 and S.LEFF2_WALK_CASES[1][0][3] == 64 and "persist=1" in S.LEFF2_WALK_CASES[1][1]
    assert all((B, H, W, C) in S.LEFF2_CASES for C in (32, 64, 128, 256, 512) for (B, H, W) in S.LEFF2_MAPS)
    assert any(M >= C for _, M, C in S.FFN_CASES if C == 256) and any(M >= C for _, M, C in S.FFN_CASES if C == 512)


def test_onehot_regions_are_closed_under_the_pairing():
    for case in S.ATTN_CASES:
        B, H, W, heads, hd, shift, kind = case
        if kind != "onehot" or not shift:
            continue
        c = S.attn_case(*case, BF16)
        t = torch.arange(64)
        quad = (t // 8 >= 4).long() * 2 + (t % 8 >= 4).long()
        assert bool((quad[c["target"]] == quad).all())                                                    # selected key and query in one quadrant: never masked
        assert bool((c["target"] != t).all())                                                             # and never the query itself


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the reference moves under each fault; the relative gate does not see the bounded ones
# ---------------------------------------------------------------------------------------------------------------------------
def test_leff2_reference_moves_under_each_fault_and_the_relative_gate_passes_the_bounded_ones():
    """Stand-ins of faulty kernels on the 3 x 8 x 24, C = 512 case in bf16 (max |reference| 6707, so the 2.5 % gate of the existing op tests is 167).  Every one moves
    the reference, so the zero gate fails it.  Measured against the relative gate (asserted below; nothing was adjusted until it passed):
      one term of the K = 2048 contraction of linear2 dropped                  passes   (max change 69)
      the seam halo read one pixel off in ONE 16-byte piece (8 channels)       passes   (22)
      one 32-wide k-step of linear2 dropped                                    caught   (744: W2 is dense +-1 and g2 reaches 84, 16 live terms are 11 % of max |ref|)
      the seam halo read one pixel off in every channel                        caught   (818)
      a tap outside the image reads 1 instead of 0                             caught   (659)
      two taps swapped, the GELU skipped                                       caught
    So on these inputs the relative gate does see a whole k-step and a whole halo column; what it cannot see is the same fault confined to one lane's
    fragment -- one term, one 16-byte piece of the halo -- which is the bounded kind a wrong index in a fragment layout or a DMA offset produces."""
    c = S.leff2_case(3, 8, 24, 512, BF16)
    ref = c["out"]
    live = int(c["up"].nonzero()[3])
    piece = slice(8 * (live // 8), 8 * (live // 8) + 8)
    faults = {"term_dropped": S.leff2_out(c, drop_channel=live), "seam_halo_one_piece": S.leff2_out(c, seam_shift=True, seam_channels=piece),
              "kstep_dropped": S.leff2_out(c, drop_kstep=5), "seam_halo": S.leff2_out(c, seam_shift=True), "no_zero_pad": S.leff2_out(c, pad_value=1.0),
              "gelu_skipped": S.leff2_out(c, gelu=False)}
    sw = dict(c)
    sw["taps"] = c["taps"].clone()
    sw["taps"][:, 1], sw["taps"][:, 3] = c["taps"][:, 3], c["taps"][:, 1]                                 # ky / kx swapped
    faults["taps_swapped"] = S.leff2_out(sw)
    seen = {}
    for name, bad in faults.items():
        assert moved(bad, ref), name
        seen[name] = old_gate_passes(bad, ref)
    print(seen)
    assert seen["term_dropped"] and seen["seam_halo_one_piece"], seen                                     # the evidence for the gap
    assert not any(seen[k] for k in ("kstep_dropped", "seam_halo", "no_zero_pad", "gelu_skipped", "taps_swapped")), seen
    # confined where they should be: the seam fault touches output column 7 only, the pad fault border pixels only
    d = (faults["seam_halo"] != ref).reshape(3, 8, 24, -1).any(3)
    assert bool(d[:, :, 7].any()) and not bool(d[:, :, :7].any()) and not bool(d[:, :, 8:].any())
    d = (faults["no_zero_pad"] != ref).reshape(3, 8, 24, -1).any(3)
    assert not bool(d[:, 1:-1, 1:-1].any()) and bool(d[:, 0].all())


def test_ffn_and_fc1_references_move_under_each_fault():
    c = S.ffn_case(3, 192, 256, BF16)
    ref = S.ffn_out(c, 3, (0.0, 2.0, 1.0))
    h = c["h1"].double()
    keep = torch.ones(1024, dtype=torch.bool)
    keep[96:128] = False
    s = torch.tensor((0.0, 2.0, 1.0), dtype=torch.float64).repeat_interleave(64)[:, None]
    dropped = c["x"] + s * (h[:, keep] @ c["w2"][:, keep].t() + c["b2"])
    assert moved(dropped, ref) and not old_gate_passes(dropped, ref)                                      # one k-step of fc2: dense W2, the relative gate catches it too
    live = int((c["pre"][64] > 0).nonzero()[0])
    keep[:] = True
    keep[live] = False
    one = c["x"] + s * (h[:, keep] @ c["w2"][:, keep].t() + c["b2"])
    assert moved(one, ref) and old_gate_passes(one, ref)                                                  # one term of it: the relative gate passes it
    assert moved(c["x"] + s * (c["pre"] @ c["w2"].t() + c["b2"]), ref)                                    # GELU skipped
    assert moved(c["x"] + s.roll(64, 0) * c["branch"], ref)                                               # the scale of the neighbouring image
    # fc1: one 32-wide k-step dropped moves h1 (sparse rows: every k-step holds entries of some row)
    for ks in range(256 // 32):
        w = c["w1"].clone()
        w[:, 32 * ks:32 * ks + 32] = 0
        pre = c["xn"] @ w.t() + c["b1"]
        assert moved(torch.where(pre >= S.POS_MIN, pre, torch.zeros_like(pre)), torch.where(c["pre"] > 0, c["pre"], torch.zeros_like(c["pre"])), BF16), ks
    # a row normalised from the neighbouring row's data
    assert not torch.equal(c["xn"][1:], c["xn"][:-1])


def test_qkv_reference_moves_under_each_fault():
    B, H, W, C, heads, shift, use_mod = 1, 16, 16, 64, 2, 4, True
    c = S.lnqkv_case(B, H, W, C, heads, shift, use_mod, BF16)
    M = B * H * W

    def qkv(tok=None, mod_rows=None, swap_heads=False):
        tok = c["tok"] if tok is None else tok
        mod_rows = c["mod"].repeat(M // 64, 1) if mod_rows is None else mod_rows
        xn = c["s"][tok] * c["gamma"] + c["beta"] + mod_rows
        P = xn @ c["w"].t() + c["b"]
        if swap_heads:
            P = P.reshape(M, 3, heads, C // heads).flip(2).reshape(M, 3 * C)
        return X.ref_qkv(P, M, C, heads)
    base = qkv()
    assert all(torch.equal(a.double(), b.double()) for a, b in zip(base, (c["q"], c["k"], c["vt"])))
    faults = {"rolled_the_wrong_way": qkv(tok=X.window_tokens(B, H, W, -shift)), "not_rolled": qkv(tok=X.window_tokens(B, H, W, 0)),
              "modulator_row_of_another_position": qkv(mod_rows=c["mod"].roll(1, 0).repeat(M // 64, 1)), "heads_swapped": qkv(swap_heads=True)}
    for name, bad in faults.items():
        assert all(moved(b.double(), r.double(), BF16) for b, r in zip(bad, base)), name


def test_attention_reference_moves_under_each_fault():
    def out(c, bias=None, mask=None, vt=None):
        o = S.attn_doc64(c["q"], c["k"], c["vt"] if vt is None else vt, c["bias"] if bias is None else bias, c["mask"] if mask is None else mask, BF16)[3]
        return o.to(BF16)
    t = S.attn_case(1, 16, 16, 2, 32, 0, "table", BF16)
    assert torch.equal(out(t).double(), t["o"])
    assert moved(out(t, bias=t["bias"].transpose(1, 2)), t["o"], BF16)                                    # the table read transposed
    assert moved(out(t, bias=t["bias"].flip(0)), t["o"], BF16)                                            # the table of the other head
    u = S.attn_case(1, 16, 16, 2, 32, 4, "uniform", BF16)
    assert moved(out(u, mask=torch.zeros_like(u["mask"])), u["o"], BF16)                                  # the shift mask ignored
    assert moved(out(u, mask=u["mask"].flip(0)), u["o"], BF16)                                            # the mask of another window
    h = S.attn_case(1, 16, 16, 4, 32, 4, "onehot", BF16)
    assert moved(out(h, vt=h["vt"].flip(1)), h["o"], BF16)                                                # two heads' channels swapped
    assert moved(out(h, vt=h["vt"].roll(1, 0)), h["o"], BF16)                                             # v of the neighbouring window
    assert moved(out(h, vt=h["vt"].roll(1, 3)), h["o"], BF16)                                             # keys off by one


# ---------------------------------------------------------------------------------------------------------------------------
# the fused window kernel: conditions of every case, and the faults its constructions are built for
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_conditions_of_every_block_case(dtype):
    kinds = set()
    for case in S.block_cases(dtype):
        B, H, W, C, shift, kind, use_mod = case
        c = S.block_case(*case, dtype)                                                                    # asserts margins, e in {0, 1}, sums, representability, v odd
        kinds.add(kind)
        rows = S.block_attn_out(c, B)
        assert torch.equal(rows.float().double(), rows)
        if B <= 3:
            assert torch.equal(S.block_attn_eval(c, B, H, W, shift, dtype), rows)                         # the stand-in machinery reproduces the reference
        for drop in ((None,) if B > 3 else (None, (0.0, 2.0, 1.0)[:B])):
            x1 = S.block_attn_out(c, B, drop)
            z, a1, h1, out = S.block_ffn_half(c, x1, B, H, W, dtype, drop=drop)                           # asserts both pre-activation ranges and branch shares
            assert torch.equal(out.float().double(), out)
            if kind == "self" and dtype != F32:
                assert len(z.unique(dim=0)) >= 32                                                         # LN2 is live: z differs from row to row
        if kind in ("onehot", "self"):
            assert float(c["lead"].min()) >= S.LEAD2
    assert kinds == ({"uniform", "table"} if dtype == F32 else set(S.BLOCK_KINDS))
    # every form of the launcher is reached: the forced forms where they are built, and both launch shapes of C = 256
    wins = {(case[3], case[0] * case[1] * case[2] // 64) for case in S.block_cases(dtype)}
    assert any(C == 256 and n <= 256 for C, n in wins) and (dtype == F32 or any(C == 256 and n > 256 for C, n in wins))
    if dtype != F32:
        assert "attn=3" in S.block_variants(256, 320, dtype) and "attn=3" not in S.block_variants(256, 4, dtype)
        assert {"attn=0", "attn=1", "attn=2", "attn=4", "attn=5"} <= set(S.block_variants(64, 4, dtype)) and "attn=4" not in S.block_variants(128, 4, dtype)


def test_block_reference_moves_under_each_fault():
    B, H, W, C, shift = 1, 16, 16, 64, 4
    c = S.block_case(B, H, W, C, shift, "onehot", True, BF16)
    ref = S.block_attn_out(c, B)
    ev = lambda c_, **kw: S.block_attn_eval(c_, B, H, W, shift, BF16, **kw)                               # noqa: E731
    assert moved(ev(c, scatter_shift=-shift), ref), "the scatter rolled the wrong way"
    assert moved(ev(c, gather_shift=0), ref), "rows gathered without the roll"
    assert moved(ev(c, mod_roll=1), ref), "the modulator row of another window position"
    assert moved(ev(c, swap_heads=True), ref), "two heads' channels swapped"
    # a row gathered from the neighbouring WINDOW: every window has its own placement of the codes
    c2 = dict(c)
    c2["x"] = c["x"].roll(8, 0)
    assert moved(ev(c2) - c2["x"] + c["x"], ref), "rows of another window"
    # one 32-wide k-step of the projection dropped, and one term of it (Wproj holds three entries per row and |o| <= 11: the rows after the attention
    # half stay below 50, so here the relative gate would see even the single term; it is the dense linear2 of the LeFF half where it does not)
    c3 = dict(c)
    c3["wp"] = c["wp"].clone()
    c3["wp"][:, 32:64] = 0
    assert moved(ev(c3), ref)
    c4 = dict(c)
    c4["wp"] = c["wp"].clone()
    c4["wp"][5, int(c["wp"][5].nonzero()[0])] = 0
    assert moved(ev(c4), ref)
    u = S.block_case(B, H, W, C, shift, "uniform", True, BF16)
    assert moved(S.block_attn_eval(u, B, H, W, shift, BF16, use_mask=False), S.block_attn_out(u, B)), "the shift mask ignored"
    t = S.block_case(B, H, W, C, 0, "table", True, BF16)
    assert moved(S.block_attn_eval(t, B, H, W, 0, BF16, bias=t["bias"].transpose(1, 2)), S.block_attn_out(t, B)), "the table read transposed"
    assert moved(S.block_attn_eval(t, B, H, W, 0, BF16, bias=t["bias"].flip(0)), S.block_attn_out(t, B)), "the table of the other head"


def test_window4_reference_moves_under_each_fault():
    def out(c, bias=None, v=None, k=None):
        z = torch.zeros(1, 16, 16, dtype=torch.float64)
        o = S.attn_doc64(c["q"] * c["scale"], c["k"] if k is None else k, (c["v"] if v is None else v).transpose(2, 3), c["bias"] if bias is None else bias, z, F32)[3]
        return o.to(BF16)
    t = S.attn4_case(1, 8, 8, 5, 32, "table", BF16)
    base = out(t)
    assert moved(out(t, bias=t["bias"].transpose(1, 2)), base, BF16)                                     # the table read transposed
    assert moved(out(t, bias=t["bias"].roll(1, 0)), base, BF16)                                          # the table of another head
    h = S.attn4_case(1, 8, 8, 5, 32, "onehot", BF16)
    base = out(h)
    assert moved(out(h, v=h["v"].roll(1, 1)), base, BF16)                                                # another head's v
    assert moved(out(h, v=h["v"].roll(1, 0), k=h["k"].roll(1, 0)), base, BF16)                           # keys and values of the neighbouring window
    u = S.attn4_case(3, 4, 12, 1, 32, "uniform", BF16)
    assert moved(out(u, v=u["v"].roll(1, 0)), out(u), BF16)                                              # the mean over another window's 16 keys
    # the raster placement: window w, token t sits at row w4(w, t); rows in window-major order would be another tensor
    assert not torch.equal(S.window4_rows(1, 8, 8).reshape(-1), torch.arange(64))
