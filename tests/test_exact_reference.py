"""CPU: the integer-lattice method of tests/test_gpu_exact.py stands on its own feet.

* float32 sums of lattice products equal float64 in three summation orders at the largest contraction and reduction the GPU file uses;
* the two conditions (exact_lattice) hold for every parameter set of the GPU file: the case lists are imported from exact_lattice;
* assert_exact catches CPU stand-ins of eight subtly faulty kernels, and the relative gate of the existing op tests (BF16_REL x max |ref|,
  tests/test_gpu_ops.py) lets the single-term and the single-border-column fault through, on the lattice inputs and on Gaussian ones.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_lattice as X
from exact_lattice import BF16, F16, F32, PM1, PM2, assert_exact
from test_gpu_ops import BF16_REL


# ---------------------------------------------------------------------------------------------------------------------------
# the lattice properties
# ---------------------------------------------------------------------------------------------------------------------------
def sums_f32(prod):
    """float32 sums over the last axis in three orders: forward, reversed, pairwise tree"""
    fwd = torch.zeros(prod.shape[:-1], dtype=torch.float32)
    rev = torch.zeros_like(fwd)
    for k in range(prod.shape[-1]):                              # explicit loops: one float32 add per term, in the stated order
        fwd = fwd + prod[..., k]
        rev = rev + prod[..., prod.shape[-1] - 1 - k]
    t = prod
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = torch.cat([t, torch.zeros_like(t[..., :1])], -1)
        t = t[..., 0::2] + t[..., 1::2]
    return fwd, rev, t[..., 0]


def test_largest_contraction_is_derived_from_the_case_lists():
    """uf_conv4s2_fwd at 512 input channels: 16 taps x 512; the weight gradient of 4096 tokens"""
    assert X.LARGEST_K == 16 * 512 == max(k * k * ci for (ci, _) in X.CONV_PAIRS for k in (1, 3, 4)) and X.LARGEST_REDUCTION == max(X.WGRAD_M)


@pytest.mark.parametrize("K,a_values,b_values", [(X.LARGEST_K, PM2, PM1), (X.LARGEST_REDUCTION, PM2, PM1), (2048, PM1, PM1)])
def test_f32_sums_equal_f64_in_three_orders(K, a_values, b_values):
    X.check_accumulation(K, a_values, b_values)
    a, b = X.lattice((24, K), a_values, 1, k=1), X.lattice((16, K), b_values, 2)
    ref = a @ b.t()
    prod = (a[:, None, :] * b[None, :, :]).float()
    assert torch.equal(prod.double(), a[:, None, :] * b[None, :, :])
    for s in sums_f32(prod):
        assert s.dtype == torch.float32 and torch.equal(s.double(), ref)
    assert torch.equal((a.float() @ b.float().t()).double(), ref)


def test_bound_and_double_to_bf16_rounding():
    assert X.max_partial_steps(512, PM2, PM1, addend_steps=1) == 1025
    with pytest.raises(AssertionError):
        X.check_accumulation(2 ** 23, PM2, PM1)
    t = torch.tensor([257.0, 259.0, 258.0, 262.0, -257.0, 2049.0, 2051.0], dtype=torch.float64)
    assert t.to(BF16).tolist() == [256.0, 260.0, 258.0, 262.0, -256.0, 2048.0, 2048.0]          # ties go to the even neighbour
    assert t.to(F16).tolist()[5:] == [2048.0, 2052.0]
    with pytest.raises(AssertionError):
        X.check_representable(t, BF16)
    with pytest.raises(AssertionError):
        X.lattice((4,), (0, 1), 0)


def test_conditions_hold_for_the_dense_gemm_cases():
    """condition 1 inside gemm_case, condition 2 on P for both 2-byte types -- every (M, N, K) of the GPU file, the q|k|v cases included"""
    worst = 0.0
    for (M, N, K) in X.GEMM_CASES + [X.GEMM_WIDE_TILE_CASE] + [(M, 3 * C, C) for (M, C, _) in X.QKV_CASES]:
        c = X.gemm_case(M, N, K)
        assert c["bound"] < X.ACC_STEPS
        for dtype in (BF16, F16):
            worst = max(worst, X.check_representable(c["P"], dtype))
    assert worst <= 256
    for (M, C, heads) in X.QKV_CASES:
        q, k, vt = X.ref_qkv(X.gemm_case(M, 3 * C, C)["P"], M, C, heads)
        assert q.dtype == torch.float32 and k.shape == (M // 64, heads, 64, C // heads) and vt.shape == (M // 64, heads, C // heads, 64)
        if C // heads != 32:                                     # the query scale is a power of two: nothing rounds
            assert torch.equal(q.to(BF16).double(), q.double())
    for dtype in (BF16, F16):
        for args in ((dtype,), (dtype, 64, 96, 32), (dtype, 192, 96, 32)):
            c = X.gemm_rounding_case(*args)
            prof = X.rounding_profile(c["P"], dtype)
            assert prof["away"] > 0 and prof["ties"] > 0 and float(c["P"].abs().max()) > X.OUT_STEPS[dtype]


def test_conditions_hold_for_the_other_t_output_cases():
    """depthwise stencil outputs; the T-stored input gradients of uf_downsample_bwd (tap by tap) and uf_upsample_cat_bwd"""
    for case in X.DWCONV_CASES:
        c = X.dwconv_case(*case)
        for dtype in (BF16, F16):
            X.check_representable(c["plain"], dtype, step=0.5)
            X.check_representable(c["biased"], dtype, step=0.5)
    for case in X.DOWN_BWD_CASES:
        for dtype in (BF16, F16):
            X.check_representable(X.down_bwd_case(*case)["taps"], dtype)
    for case in X.UP_BWD_CASES:
        for dtype in (BF16, F16):
            X.check_representable(X.up_bwd_case(*case)["dx"], dtype)


@pytest.mark.parametrize("family", ["samplers", "stem", "conv3", "conv41", "wgrad", "conv3_bwd"])
def test_condition_one_holds_for_the_f32_output_cases(family):
    """the case constructors assert condition 1 (check_accumulation) for their lattices; their float32-ending references must be exact in float32"""
    if family == "samplers":
        for case in [(B, H, W, C) for B in X.SAMPLER_B for (H, W) in X.SAMPLER_MAPS for C in X.SAMPLER_C] + X.DOWN_PATCH_CASES:
            c = X.sampler_case(*case)
            assert torch.equal(c["down"].float().double(), c["down"]) and torch.equal(c["up"].float().double(), c["up"])
    elif family == "stem":
        for case in [(B, H, W, E) for B in X.SAMPLER_B for (H, W) in X.STEM_MAPS for E in X.SAMPLER_C]:
            c = X.stem_case(*case)
            assert c["stem"].dtype == torch.float32
        for case in [(B, H, W, C2) for B in X.SAMPLER_B for (H, W) in X.STEM_MAPS for C2 in X.HEAD_C]:
            c = X.head_case(*case)
            assert torch.equal(c["head_img"].float().double(), c["head_img"]) and torch.equal(c["head"].float().double(), c["head"])
    elif family == "conv3":
        for (ci, co, H, W, B) in X.conv3_cases():
            c = X.conv_case(3, B, H, W, ci, co)
            assert c["lrelu"].dtype == torch.float32 and c["dgrad_acc"].dtype == torch.float32
            assert torch.equal(c["pre_acc"].float().double(), c["pre_acc"])
    elif family == "conv41":
        for (ci, co) in X.CONV_PAIRS:
            for (k, H, W, B) in X.conv41_cases(ci, co):
                c = X.conv_case(k, B, H, W, ci, co)
                assert torch.equal(c["out"].float().double(), c["out"])
    elif family == "wgrad":
        for case in X.WGRAD_CASES:
            c = X.wgrad_case(*case)
            assert torch.equal(c["dW"].float().double(), c["dW"])
    else:
        for case in X.CONV3_BWD_CASES:
            c = X.conv3_bwd_case(*case)
            assert all(torch.equal(c[n].float().double(), c[n]) for n in ("dx", "dW", "db"))


def test_layout_helpers():
    tok = X.window_tokens(2, 16, 24, 4)
    assert sorted(tok.tolist()) == list(range(2 * 16 * 24))
    assert tok[0] == 4 * 24 + 4 and X.window_tokens(1, 8, 8, 0).tolist() == list(range(64))
    idx = X.rpb_index(8)
    assert idx.shape == (64, 64) and int(idx.min()) == 0 and int(idx.max()) == 224 and int(idx[0, 0]) == 112
    x = X.lattice((2, 3, 6, 10), PM2, 3)
    cols = X.ref_im2col(x, 4, 2, 1)
    assert cols.shape == (2 * 3 * 5, 48)
    assert torch.equal(X.ref_col2im(torch.ones_like(cols), 2, 6, 10, 3, 4, 2, 1)[0, 0, 0], torch.tensor([1.0, 2, 2, 2, 2, 2, 2, 2, 2, 1], dtype=torch.float64) * 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison catches subtly wrong kernels; the relative gate does not
# ---------------------------------------------------------------------------------------------------------------------------
def old_gate_passes(got, ref):
    """the check of tests/test_gpu_ops.py for a bf16 kernel: max abs error against BF16_REL x max(1, max |ref|)"""
    return float((got.float() - ref.float()).abs().max()) <= BF16_REL * max(1.0, float(ref.abs().max()))


def exact_fails(name, got, ref64, dtype):
    try:
        assert_exact("standin/" + name, got, ref64, dtype)
    except AssertionError as e:
        assert "differ" in str(e) and "tile" in str(e) and "expected" in str(e)
        return True
    finally:
        X.RECORDS.pop("standin/" + name, None)
    return False


def trunc_bf16(x64):
    """store with truncation toward zero in place of round-to-nearest-even"""
    return (x64.float().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def gemm_inputs(kind, M, N, K):
    if kind == "lattice":
        c = X.gemm_case(M, N, K)
        return c["A"], c["W"], c["bias"]
    g = torch.Generator().manual_seed(5)                          # the inputs of the existing op tests: Gaussian, weights scaled by K ** -0.5, rounded to bf16
    return (torch.randn(M, K, generator=g).to(BF16).double(), (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16).double(), 0.1 * torch.randn(N, generator=g).double())


def conv_inputs(kind, B, cin, cout, H, W):
    if kind == "lattice":
        c = X.conv_case(3, B, H, W, cin, cout)
        return c["x"], c["w"], c["bias"]
    g = torch.Generator().manual_seed(6)
    return (torch.randn(B, cin, H, W, generator=g).to(BF16).double(), (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(BF16).double(),
            0.1 * torch.randn(cout, generator=g).double())


def test_every_faulty_standin_is_caught_and_the_relative_gate_is_not_enough():
    """Eight faulty kernels (and the single dropped term, and the single tap of the border fault), as CPU stand-ins.  assert_exact fails on every one on the lattice inputs.
    Whether the relative gate of the existing op tests (max abs error <= BF16_REL x max(1, max |ref|)) lets the fault through, measured here on
    the lattice inputs / on Gaussian inputs as the existing tests draw them (M = 130, N = 96, K = 512; 3x3 conv 64 -> 96 on 17 x 23):
      one term of the K = 512 contraction dropped      passes / caught   (a Gaussian term reaches 0.4 somewhere among 12480 outputs, the gate is 0.1)
      truncating store                                 passes / passes   (one bf16 ulp is 2^-8 relative, a sixth of the gate)
      one tap from the clamped neighbour, right column caught / caught   (a tap of the implicit GEMM is 64 terms, not one: 10 % of max |ref|)
      padding predicate off by one, right and bottom   caught / caught   (every tap of the last column and the last row, nothing elsewhere)
      one 8-element k-chunk added twice                caught / caught
      last 32-element k-step dropped                   caught / caught
      two stencil taps swapped                         caught / caught
      tail rows of the last tile from the clamped row  caught / caught
      wrong leading dimension of the destination       caught / caught
      per-image scale from the neighbouring image      caught / caught
    So the max-norm gate does catch a fault that moves SOME output by more than 2.5 % of the largest one, which on 10^4 outputs most structural
    faults do; what it cannot see is a fault of bounded size -- one lattice step in a sum of hundreds, the rounding mode of a store, and by the same
    arithmetic anything below 2.5 % of max |ref| (0.1 on the Gaussian inputs, 3 to 5 lattice steps here).  The single-border-column stand-in does
    NOT get through the old gate at this shape; it was not adjusted until it did.  Asserted below: what passes the old gate in this table."""
    M, N, K = 130, 96, 512
    seen = {}
    for kind in ("lattice", "gauss"):
        A, W, b = gemm_inputs(kind, M, N, K)
        P = A @ W.t() + b
        ref = P.to(BF16)
        faults = {
            "term_dropped": P - A[:, 100:101] @ W[:, 100:101].t(),
            "chunk_twice": P + A[:, 64:72] @ W[:, 64:72].t(),
            "last_kstep_dropped": A[:, :K - 32] @ W[:, :K - 32].t() + b,
            "tail_rows_clamped": torch.cat([P[:128], P[M - 1:M].expand(M - 128, N)]),
        }
        wrong_ld = torch.zeros(M * (N + 16), dtype=torch.float64)
        for m in range(M):
            wrong_ld[m * (N + 8):m * (N + 8) + N] = P[m]          # written with ld = N + 8, read with ld = N + 16
        faults["wrong_ld"] = wrong_ld.reshape(M, N + 16)[:, :N]
        Bi, H, Wd = X.RES_PLAIN[M]
        scale = torch.tensor([0.5, 2.0], dtype=torch.float64)
        resid = X.lattice((M, N), PM2, 9)
        res_ref = X.ref_residual(P, resid, scale, Bi, H, Wd)
        for name, bad in faults.items():
            if kind == "lattice":
                assert exact_fails(name, bad.to(BF16), P, BF16), name
            seen[(name, kind)] = old_gate_passes(bad.to(BF16), ref)
        bad = X.ref_residual(P, resid, scale.flip(0), Bi, H, Wd)
        if kind == "lattice":
            assert exact_fails("neighbour_scale", bad.float(), res_ref, F32)
        seen[("neighbour_scale", kind)] = old_gate_passes(bad, res_ref)
        # truncation: on results T cannot hold
        Pr = X.gemm_rounding_case(BF16)["P"] if kind == "lattice" else P * 37.0
        if kind == "lattice":
            assert exact_fails("truncating_store", trunc_bf16(Pr), Pr, BF16)
        seen[("truncating_store", kind)] = old_gate_passes(trunc_bf16(Pr), Pr.to(BF16))
        # stencil faults on the 3x3 implicit GEMM
        Bc, cin, cout, Hc, Wc = 1, 64, 96, 17, 23
        x, w, bias = conv_inputs(kind, Bc, cin, cout, Hc, Wc)
        conv = F.conv2d(x, w, bias, padding=1)
        xp = F.pad(x, (1, 1, 1, 1))
        xp_bad = xp.clone()
        xp_bad[:, :, :, -1] = xp[:, :, :, -2]                      # the right zero column reads the clamped neighbour: predicate ix < W off by one
        xp_bad[:, :, -1, :] = xp_bad[:, :, -2, :]                  # and the bottom zero row: predicate iy < H off by one
        one_tap = conv.clone()                                     # ONE tap (ky = 0, kx = 2) at the ONE border column ox = W - 1
        one_tap[:, :, :, -1] += torch.einsum("bchw,oc->bohw", xp_bad[:, :, 0:Hc, -1:], w[:, :, 0, 2])[..., 0]
        both = sum(torch.einsum("bchw,oc->bohw", xp_bad[:, :, ky:ky + Hc, kx:kx + Wc], w[:, :, ky, kx]) for ky in range(3) for kx in range(3)) + bias[None, :, None, None]
        if kind == "lattice":                                      # exact arithmetic: the fault is confined to the last column and the last row
            assert torch.equal(both[:, :, :-1, :-1], conv[:, :, :-1, :-1]) and bool((both[:, :, -1, :] != conv[:, :, -1, :]).any()) and bool((both[:, :, :, -1] != conv[:, :, :, -1]).any())
        w_sw = w.clone()
        w_sw[:, :, 0, 1], w_sw[:, :, 1, 0] = w[:, :, 1, 0], w[:, :, 0, 1]
        for name, bad in (("border_tap", one_tap), ("border_right_bottom", both), ("taps_swapped", F.conv2d(x, w_sw, bias, padding=1))):
            if kind == "lattice":
                assert exact_fails(name, bad.float(), conv, F32), name
            seen[(name, kind)] = old_gate_passes(bad.to(BF16), conv.to(BF16))
    print({f"{n}/{k}": v for (n, k), v in sorted(seen.items())})
    assert seen[("term_dropped", "lattice")] and seen[("truncating_store", "lattice")] and seen[("truncating_store", "gauss")]      # the evidence for the gap
    caught = [k for k, v in seen.items() if not v]
    assert {("border_tap", "lattice"), ("border_right_bottom", "lattice"), ("border_right_bottom", "gauss"), ("term_dropped", "gauss")} <= set(caught), \
        "the docstring's table no longer describes the old gate"
