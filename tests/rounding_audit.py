"""Rounding audit of the 2-byte stores of the nonlinear kernels (helpers; no GPU needed).  DESIGN.md section 2.3 has the argument.

Kind A, boundary-aware exactness: where the stored T value is ONE rounding of float32 arithmetic on a bit-known input, the kernel must
return the float64 value of the documented function rounded to T, nearest-even, TO THE BIT -- except where that value lies within
``tau`` of a midpoint between two T values (there either neighbour is accepted; ``tau`` bounds the float32 evaluation error and is
computed from the reference alone) and below T's smallest normal (there: within one subnormal step).

Kind B, signed-error statistics: where several T roundings lie between input and output, the shrinkage slope ``beta`` and the mean
signed error in ulps ``mu`` of the kernel are gated against what the CPU emulation of the kernel's arithmetic shows when ONE of its
rounding points truncates toward zero (beta) or its final store rounds toward minus infinity (mu).

The case lists of tests/test_gpu_rounding.py live here, so that tests/test_rounding_reference.py (CPU) asserts the conditions of both
kinds on exactly the cases the GPU file runs.
"""
import functools
import json
import math
import os

import torch
import torch.nn.functional as F

import edge_cases as E
import exact_lattice as X
from edge_cases import BF16, F16, F32, GELU_A, GELU_B, MARGIN, TAG
from oracle.bf16_budget import ALL, Budget

HALF = [BF16, F16]
EPS32 = 2.0 ** -23                       # spacing of float32 at 1: an operation rounded to nearest errs by at most EPS32 / 2 relative
TINY32 = 2.0 ** -126                     # float32's smallest normal: v_rcp_f32 / v_exp_f32 may flush what lies below it
LN2 = math.log(2.0)
NEAR_CAP = 0.02                          # largest share of a case that may lie near a midpoint
# GELU'(a) = s + a e s^2 (DG0 + DG1 a^2): the constants of gelu_grad_t (uf_common.h), = -ln2 (A + 3 B a^2) to 7 digits
DG0, DG1 = 1.5957691216, 0.2140610
U_CLAMP = 80.0                           # gelu_grad_t: u = min(a (A + B a^2), 80)


# ---------------------------------------------------------------------------------------------------------------------------
# the grid of T, directed roundings
# ---------------------------------------------------------------------------------------------------------------------------
def tiny(dtype):
    return float(torch.finfo(dtype).tiny)


def sub_step(dtype):
    """spacing of T's subnormals"""
    return tiny(dtype) * float(torch.finfo(dtype).eps)


def spacing(ref, dtype):
    """float64 distance between the two T values around ``ref`` (the subnormal step below T's smallest normal)"""
    a = ref.double().abs()
    _, e = torch.frexp(a)                                              # a = m 2^e, m in [0.5, 1)
    emin = int(round(math.log2(tiny(dtype))))
    e = torch.where(a > 0, e - 1, torch.full_like(e, emin)).clamp_min(emin)
    return torch.ldexp(torch.full_like(a, float(torch.finfo(dtype).eps)), e)


def _toward(r, target):
    return torch.nextafter(r, torch.full_like(r, target))


def round_to(x, dtype, mode="rne"):
    """``x`` (float32 / float64) rounded to T and widened again: rne = nearest-even, rz = toward zero (a shift instead of a conversion),
    floor = toward minus infinity"""
    r = x.to(dtype)
    if mode == "rz":
        r = torch.where(r.to(x.dtype).abs() > x.abs(), _toward(r, 0.0), r)
    elif mode == "floor":
        r = torch.where(r.to(x.dtype) > x, _toward(r, float("-inf")), r)
    elif mode != "rne":
        raise KeyError(mode)
    return r.to(x.dtype)


class Rounder(Budget):
    """oracle.bf16_budget.Budget whose named rounding points can be given another mode: ``modes`` = {switch: "rz" | "floor"}; every
    other switch in ``on`` rounds to nearest even"""

    def __init__(self, on, dtype, modes=None):
        super().__init__([s for s in on if s in ALL], TAG[dtype])
        self.names, self.dtype, self.modes = frozenset(on), dtype, dict(modes or {})

    def r(self, name, x):
        return round_to(x, self.dtype, self.modes.get(name, "rne")) if name in self.names else x


def faults(switches, final=None):
    """the faulty emulations of Kind B: toward-zero truncation of each switch, and a floor-type store of ``final`` (a T output)"""
    out = [("rz:" + s, {s: "rz"}) for s in switches]
    return out + ([("floor:" + final, {final: "floor"})] if final else [])


# ---------------------------------------------------------------------------------------------------------------------------
# Kind A: the check
# ---------------------------------------------------------------------------------------------------------------------------
RECORDS = {}            # "entry_point/case" -> figures


def _bits(t):
    return t.contiguous().view(torch.int16)


def classify(ref64, tau, dtype, flush=None, abs_floor=None):
    """want (T), the other neighbour (T), near mask, small mask, and the absolute bound of the small elements"""
    ref64, tau = ref64.double(), tau.double()
    want = ref64.to(dtype)
    wd = want.double()
    other = torch.where(wd <= ref64, _toward(want, float("inf")), _toward(want, float("-inf")))
    mid = 0.5 * (wd + other.double())
    small = ref64.abs() < tiny(dtype)
    if flush is not None:
        small = small | flush
    near = ((ref64 - mid).abs() <= tau) & ~small
    bound = torch.full_like(ref64, sub_step(dtype)) + (0.0 if abs_floor is None else abs_floor.double())
    return want, other, near, small, bound


def audit_exact(name, got, ref64, tau, dtype, flush=None, abs_floor=None, cap=NEAR_CAP):
    """the three assertions of Kind A on ``got`` (a T tensor or a float tensor of T values, any device) + the cap on the near share.
    ``flush`` marks elements at which a factor of the documented product lies below float32's smallest normal (the float32 evaluation
    may flush it): they are held to ``abs_floor`` + one subnormal step of T, as the elements below T's smallest normal are."""
    got = got.detach().cpu()
    if got.dtype != dtype:
        assert torch.equal(got.to(dtype).to(got.dtype), got), f"{name}: not a tensor of {TAG[dtype]} values"
        got = got.to(dtype)
    ref64 = ref64.detach().cpu().double().reshape(got.shape)
    tau = tau.detach().cpu().double().reshape(got.shape)
    want, other, near, small, bound = classify(ref64, tau, dtype, None if flush is None else flush.reshape(got.shape),
                                               None if abs_floor is None else abs_floor.reshape(got.shape))
    gb = _bits(got)
    eq_want, eq_other = gb == _bits(want), gb == _bits(other)
    ok_small = (got.double() - ref64).abs() <= bound
    ok = torch.where(small, ok_small, torch.where(near, eq_want | eq_other, eq_want))
    n = got.numel()
    rec = {"elements": n, "near": int(near.sum()), "near_share": float(near.sum()) / n, "small": int(small.sum()),
           "mismatches": int((~ok).sum()), "near_other": int((near & eq_other & ~eq_want).sum())}
    RECORDS[name] = rec
    assert rec["near_share"] <= cap, f"{name}: {rec['near_share']:.2%} of the elements lie near a midpoint (cap {cap:.0%}): the test would hide a failure"
    if rec["mismatches"]:
        i = int((~ok).reshape(-1).nonzero()[0])
        kind = "small" if bool(small.reshape(-1)[i]) else ("near" if bool(near.reshape(-1)[i]) else "plain")
        raise AssertionError(f"{name}: {rec['mismatches']} of {n} elements are not the documented value rounded to nearest even; first at flat {i} ({kind}): "
                             f"got {float(got.reshape(-1)[i])!r}, expected {float(want.reshape(-1)[i])!r} (float64 {float(ref64.reshape(-1)[i])!r}, tau {float(tau.reshape(-1)[i]):.3e})")
    return rec


def emulation_within(emu32, ref64, tau, small=None):
    """condition of Kind A: the float32 emulation (before the rounding to T) stays within tau / MARGIN of the reference"""
    d = (emu32.double() - ref64.double()).abs()
    lim = tau.double() / MARGIN
    bad = d > lim
    if small is not None:
        bad = bad & ~small
    return not bool(bad.any()), float((d / lim.clamp_min(1e-300))[~small if small is not None else slice(None)].max())


# ---------------------------------------------------------------------------------------------------------------------------
# Kind A: the documented GELU (sigmoid form) and its float32 error bound
# ---------------------------------------------------------------------------------------------------------------------------
def _kappa_s(s, u):
    """relative error of s = 1 / (1 + 2^u) evaluated in float32, in units of EPS32: u carries three roundings (1.5), 2^u amplifies them
    by ln2 |u| and adds one ulp of its own, the sum 1 + e passes the share e / (1 + e) = 1 - s of that on and rounds once, the
    reciprocal errs by one ulp"""
    return (1.0 - s) * (1.0 + 1.5 * LN2 * u.abs()) + 1.5


def gelu_doc(x, clamp=False):
    """float64 (value, tau, flush, abs_floor) of the documented forward x / (1 + 2^u), u = x (A + B x^2) (gelu_bf2; ``clamp``: u limited
    to 80, gelu_and_grad_t).  tau = MARGIN EPS32 (kappa_s + 1/2) |value|."""
    x = x.double()
    u = x * (GELU_A + GELU_B * x * x)
    if clamp:
        u = u.clamp(max=U_CLAMP)
    s = torch.sigmoid(-LN2 * u)
    ref = x * s
    tau = MARGIN * EPS32 * (_kappa_s(s, u) + 0.5) * ref.abs()
    flush = s < 4 * TINY32              # 1 + 2^u reaches float32's largest binade: its reciprocal is a float32 subnormal
    return ref, tau, flush, x.abs() * 4 * TINY32


def gelu_grad_doc(x, dy=None):
    """float64 (value, tau) of the documented dy * GELU'(x) = dy (s + x e s^2 (DG0 + DG1 x^2)), e = 2^u, u = min(x (A + B x^2), 80), s = 1 / (1 + e)
    (gelu_grad_t).  The two terms can cancel (GELU' crosses zero near -0.75), so tau is absolute: each term's magnitude times its own
    relative error, + the rounding of the sum and of the product with dy."""
    x = x.double()
    u = (x * (GELU_A + GELU_B * x * x)).clamp(max=U_CLAMP)
    e = torch.exp2(u)
    s = 1.0 / (1.0 + e)
    t2 = x * e * s * s * (DG0 + DG1 * x * x)
    g = s + t2
    ks = _kappa_s(s, u)
    kt = (1.0 + 1.5 * LN2 * u.abs()) + 2.0 * ks + 1.5 + 2.0         # e, s^2, the polynomial (3 roundings), four products
    err = s.abs() * ks + t2.abs() * kt + g.abs()
    d = torch.ones_like(x) if dy is None else dy.double()
    return d * g, MARGIN * EPS32 * d.abs() * err


def gelu32(x, clamp=False):
    """the forward in float32 arithmetic, not rounded"""
    x = x.float()
    u = x * (x * x * GELU_B + GELU_A)
    if clamp:
        u = u.clamp(max=U_CLAMP)
    return x * (1.0 / (torch.exp2(u) + 1.0))


def gelu_grad32(x, dy):
    x, dy = x.float(), dy.float()
    u = torch.clamp(x * (x * x * GELU_B + GELU_A), max=U_CLAMP)
    e = torch.exp2(u)
    sg = 1.0 / (e + 1.0)
    return dy * (sg + x * e * sg * sg * (DG0 + DG1 * x * x))


def gelu_erf64(x):
    x = x.double()
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu_off64(x, a=GELU_A * (1 + 5e-4)):
    """the sigmoid form with the constant A off in its 4th digit (-2.3022 -> -2.3034)"""
    x = x.double()
    return x * torch.sigmoid(-LN2 * x * (a + GELU_B * x * x))


@functools.lru_cache(maxsize=None)
def gelu_domain(dtype):
    """every T value with |x| in [2^-14, 16), both signs (bf16: 4608, f16: 36864) + the two zeros + -8.4 snapped to T and its two neighbours"""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = bits.view(dtype)
    a = v.double().abs()
    x = v[(a >= 2.0 ** -14) & (a < 16.0)]
    n = {BF16: 4608, F16: 36864}[dtype]
    assert x.numel() == n
    c = torch.tensor(-8.4).to(dtype)
    extra = torch.stack([torch.tensor(0.0).to(dtype), torch.tensor(-0.0).to(dtype), c, _toward(c, float("inf")), _toward(c, float("-inf"))])
    x = torch.cat([x, extra])
    pad = (-x.numel()) % 8                                    # whole 16-byte chunks
    return torch.cat([x, torch.ones(pad, dtype=dtype)]).contiguous()


def gelu_dy(dtype, which):
    n = gelu_domain(dtype).numel()
    if which == "one":
        return torch.ones(n, dtype=dtype)
    return torch.randn(n, generator=torch.Generator().manual_seed(7)).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# Kind A: GEMM and stencil epilogues on lattices (the pre-activation is exact: only the epilogue rounds)
# ---------------------------------------------------------------------------------------------------------------------------
# (M, N, K, UF_VARIANT): N <= 32 -> the 32-column tile, N <= 64 and small products -> the 64-column tile, one K tile (single LDS buffer) and several, both
# staging paths where the LDS-DMA one exists, a ragged M (130 = one whole row tile + 2 rows); the 128-column tile needs 512 tiles of 128 x 128
EPI_GEMM_CASES = [(130, 32, 32, None), (64, 64, 64, None), (130, 96, 128, "gemm_dma=0"), (130, 96, 128, "gemm_dma=1"), X.GEMM_WIDE_TILE_CASE + (None,)]


def epi_shift(K):
    """power of two that scales the lattice pre-activations (sums of K products of {-2..2} x {-1, 1}: standard deviation sqrt(2.5 K)) to a
    standard deviation of about 2.5, so that they cover about [-6, 6]"""
    return max(0, round(math.log2(math.sqrt(2.5 * K) / 2.5)))


@functools.lru_cache(maxsize=4)
def epi_gemm_case(M, N, K):
    """A (M, K) in {-2..2} 2^-k, W (N, K) and bias in {-1, 1} (bias 2^-k): pre = A W^T + bias is exact in float32 and a T value; dy / Wt of
    the gradient form are the same lattices (dy (M, K) against Wt (N, K)), the pre-activation it differentiates at is ``a`` (dgelu_points)"""
    k = epi_shift(K)
    A, W, b = X.lattice((M, K), X.PM2, 4000 + K + M, k=k), X.lattice((N, K), X.PM1, 5000 + K + N), X.lattice((N,), X.PM1, 6000 + N, k=k)
    X.check_accumulation(K, X.PM2, X.PM1, addend_steps=1)
    pre = A @ W.t() + b
    return {"A": A, "W": W, "bias": b, "pre": pre, "g": A @ W.t(), "k": k, "a": dgelu_points((M, N), 7000 + M + N)}


def dgelu_points(shape, seed):
    """pre-activations of the gradient forms (a free input there): multiples of 1/8 in [-6, 6], T values.  Where GELU' cancels (its zero crossing at
    -0.752) or is tiny (the negative tail, where ln2 |u| amplifies the error of u), tau is of the order of T's spacing: measured near shares of 3 % to
    30 % for f16 on [-5, 0] against 0.3 % on [0, 6].  So that the cap holds, the grid leaves out [-1.25, 0] and draws a negative value a quarter of the
    time; the exhaustive domain of uf_gelu_bwd covers what is left out."""
    g = torch.Generator().manual_seed(seed)
    pos, neg = torch.arange(1, 49, dtype=torch.float64) / 8.0, -torch.arange(11, 49, dtype=torch.float64) / 8.0
    p = pos[torch.randint(len(pos), tuple(shape), generator=g)]
    n = neg[torch.randint(len(neg), tuple(shape), generator=g)]
    return torch.where(torch.rand(tuple(shape), generator=g) < 0.25, n, p)


def check_t_exact(ref64, dtype):
    assert torch.equal(ref64.to(dtype).double(), ref64), f"a lattice value is not a {TAG[dtype]} value"


# (B, H, W, C): 8 x 8 is all border; W = 16 / 24 are multiples of 8 (the walking kernel), W = 12 is not (the strip kernel, exact_lattice.DWCONV_CASES)
EPI_DWCONV_CASES = [(1, 8, 8, 64), (2, 16, 16, 32), (1, 8, 24, 128), (2, 8, 12, 16), (1, 12, 12, 32)]


@functools.lru_cache(maxsize=None)
def epi_dwconv_case(B, H, W, C):
    """x in {-2..2}, taps in {-2..2} / 4, bias in {-1, 1} / 4: pre = stencil + bias within +-9.25 in steps of 1/4 (a T value); dc in {-1, 1} and the flipped-tap
    stencil of dc, g (steps of 1/4, |g| <= 4.5); ``a`` = the pre-activation the gradient forms differentiate at (dgelu_points)"""
    x, w, b = X.lattice((B, C, H, W), X.PM2, 131 + C), X.lattice((C, 1, 3, 3), X.PM2, 132 + C, k=2), X.lattice((C,), X.PM1, 133 + C, k=2)
    dc = X.lattice((B, C, H, W), X.PM1, 134 + C)
    X.check_accumulation(9, X.PM2, X.PM2, addend_steps=1)
    pre = F.conv2d(x, w, b, padding=1, groups=C)
    g = F.conv2d(dc, w.flip(2, 3), None, padding=1, groups=C)             # input gradient of the stencil: the flipped taps
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()                   # noqa: E731
    return {"x": nhwc(x), "w9": w.reshape(C, 9).t().contiguous(), "bias": b, "pre": nhwc(pre), "dc": nhwc(dc), "g": nhwc(g),
            "a": dgelu_points((B, H, W, C), 135 + C + W)}


# ---------------------------------------------------------------------------------------------------------------------------
# Kind A: LayerNorm with a T output on integer rows (mean and centred values exact in float32: only relative errors remain)
# ---------------------------------------------------------------------------------------------------------------------------
LN_CS = E.LN_CS
LN_MODES = [("plain", 0, 0, False), ("plain_mod", 0, 0, True), ("win0", 1, 0, False), ("win0_mod", 1, 0, True), ("win4", 1, 4, False), ("win4_mod", 1, 4, True)]
LN_MAP = (2, 8, 8)                       # B, H, W: 128 rows, two windows


@functools.lru_cache(maxsize=None)
def ln_case(C):
    """128 rows of integers: {-2..2} + a row offset in -3..3 (row means differ; max|x| / std stays below 5)"""
    rows = LN_MAP[0] * LN_MAP[1] * LN_MAP[2]
    g = torch.Generator().manual_seed(300 + C)
    x = X.lattice((rows, C), X.PM2, 301 + C) + torch.randint(-3, 4, (rows, 1), generator=g).double()
    gm, bt = E.ln_affine(C)
    mod = (0.1 * torch.randn(64, C, generator=g)).float()       # small against the normalised rows: the sum rarely cancels (a cancelled sum is small against tau)
    return {"x": x.float(), "gamma": gm, "beta": bt, "mod": mod}


def ln_doc(x, gamma, beta, mod, windowed, shift, C):
    """float64 (value, tau, emulation) of LayerNorm (+ roll, partition, modulator), rows in the order the kernel writes them.
    The inputs are integers and C is a power of two, so the float32 mean (any order of the sum, times 1 / C) and the centred values are EXACT
    (asserted here): the factor ln_condition(x) multiplies an input error of zero, and what remains is relative -- the sum of squares (one rounding
    per square, log2(C) levels of a sum of positive terms), + eps, the reciprocal square root (one ulp), two products, the two additions."""
    B, H, W = LN_MAP
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    v = xd - mu
    assert torch.equal(E.tree_sum(x.float()) * (1.0 / C), mu.float()) and torch.equal((x.float() - mu.float()).double(), v), "the centred rows are not exact in float32"
    assert E.ln_condition(x) < 8.0
    t = v / (v.pow(2).mean(-1, keepdim=True) + 1e-5).sqrt() * gamma.double()
    y = t + beta.double()
    emu = E.ln_emu(x, gamma, beta, F32).double()
    if windowed:
        tok = X.window_tokens(B, H, W, shift)
        t, y, emu = t[tok], y[tok], emu[tok]
    out = y
    if mod is not None:
        m = mod.double().repeat(y.shape[0] // 64, 1)
        out, emu = y + m, (emu.float() + m.float()).double()
    kt = 3.0 + math.log2(C) / 4.0
    tau = MARGIN * EPS32 * (kt * t.abs() + 0.5 * y.abs() + 0.5 * out.abs())
    return out, tau, emu


# ---------------------------------------------------------------------------------------------------------------------------
# Kind B: statistics
# ---------------------------------------------------------------------------------------------------------------------------
MU_BULK = 0.25          # mu is taken over the elements with |ref| >= MU_BULK x rms(ref)


def signed_stats(got, ref64, out_dtype=None):
    """beta = sum((got - ref) ref) / sum(ref^2); mu = mean((got - ref) / spacing_T(ref)) for a T output, else None.
    mu runs over the bulk of the tensor, |ref| >= rms / 4: an element near zero carries the error of the roundings in front of it (which scales with
    its row, not with the element) at many times its own spacing, the ratio has a 1 / |ref| tail, and its mean over all elements does not settle
    (nearest-even emulations of uf_ln_qkv_fwd gave -56 and +4 ulp on two seeds; over the bulk, +-0.02)."""
    got, ref64 = got.detach().cpu().double().reshape(-1), ref64.detach().cpu().double().reshape(-1)
    d = got - ref64
    beta = float((d * ref64).sum() / (ref64 * ref64).sum())
    if out_dtype in (None, F32):
        return beta, None
    bulk = ref64.abs() >= MU_BULK * ref64.pow(2).mean().sqrt()
    return beta, float((d[bulk] / spacing(ref64[bulk], out_dtype)).mean())


STATS = {}              # "entry_point/case/output" -> figures of the report


def emulation_stats(ref64, run, switches, final, dtype):
    """``run(Rounder)`` -> output.  Returns {"b0", "mu0", "b": {fault: beta}, "mu_floor"}: nearest-even everywhere, each switch truncating,
    the final store of floor type"""
    on = tuple(switches)
    b0, mu0 = signed_stats(run(Rounder(on, dtype)), ref64, dtype if final else None)
    out = {"b0": b0, "mu0": mu0, "b": {}, "mu_floor": None}
    for name, modes in faults(switches, final):
        b, mu = signed_stats(run(Rounder(on, dtype, modes)), ref64, dtype if final else None)
        if name.startswith("rz:"):
            out["b"][name] = b
        else:
            out["mu_floor"] = mu
    return out


def condition_ok(st, factor=8.0):
    """|b0| <= min |b_s| / 8 over the truncating runs, |mu0| <= |mu_floor| / 8"""
    ok = abs(st["b0"]) <= min(abs(b) for b in st["b"].values()) / factor
    if st["mu_floor"] is not None:
        ok = ok and abs(st["mu0"]) <= abs(st["mu_floor"]) / factor
    return ok


def gate_kernel(name, got, ref64, st, out_dtype=None):
    """the GPU gate: |beta| <= min |b_s| / 4, |mu| <= |mu_floor| / 4; figures into STATS"""
    beta, mu = signed_stats(got, ref64, out_dtype)
    lim_b = min(abs(b) for b in st["b"].values()) / 4.0
    rec = {"beta": beta, "mu": mu, "b0": st["b0"], "mu0": st["mu0"], "b_s": st["b"], "mu_floor": st["mu_floor"], "gate_beta": lim_b}
    bad = []
    if not abs(beta) <= lim_b:
        bad.append(f"{name}: shrinkage slope {beta:.3e} outside +-{lim_b:.3e} (nearest-even emulation {st['b0']:.3e}, truncating {st['b']})")
    if mu is not None and st["mu_floor"] is not None:
        rec["gate_mu"] = abs(st["mu_floor"]) / 4.0
        if not abs(mu) <= rec["gate_mu"]:
            bad.append(f"{name}: mean signed error {mu:.3f} ulp outside +-{rec['gate_mu']:.3f} (nearest-even emulation {st['mu0']:.3f}, floor store {st['mu_floor']:.3f})")
    STATS[name] = rec
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# Kind B: cases, float64 references and emulations with named rounding points
# ---------------------------------------------------------------------------------------------------------------------------
ATT_B, ATT_H, ATT_W = 4, 16, 16          # 16 windows of 8 x 8
ATT_CASES = [(2, 16, 0), (2, 16, 4), (2, 32, 0), (2, 32, 4), (1, 64, 0), (1, 64, 4)]          # (heads, head_dim, shift)
SEEDS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def diffuse_case(heads, hd, shift, dtype, seed=0):
    """the diffuse class: q scaled by 0.3 keeps every softmax row spread over its keys, so no probability is exactly 0 or 1 (edge_cases'
    one_hot and uniform classes are blind to the rounding of P for that reason).  q, k (nW, heads, 64, hd), vt (nW, heads, hd, 64) of type T."""
    g = torch.Generator().manual_seed(900 + 100 * seed + 10 * heads + hd + shift)
    nW = ATT_B * (ATT_H // 8) * (ATT_W // 8)
    rn = lambda *s: torch.randn(*s, generator=g)                                # noqa: E731
    q, k, v = 0.3 * rn(nW, heads, 64, hd), rn(nW, heads, 64, hd), rn(nW, heads, 64, hd)
    do = rn(nW * 64, heads * hd)
    return {"q": q.to(dtype), "k": k.to(dtype), "vt": v.transpose(-1, -2).contiguous().to(dtype), "bias": (0.5 * rn(heads, 64, 64)).contiguous(),
            "do": do.to(dtype), "shift": shift, "heads": heads, "hd": hd, "nW": nW}


def att_logits(case, dt):
    s = case["q"].to(dt) @ case["k"].to(dt).transpose(-1, -2) + case["bias"].to(dt).unsqueeze(0)
    if case["shift"]:
        m = E.shift_mask(ATT_H, ATT_W, case["shift"]).to(dt)                   # (windows of one image, 64, 64)
        s = s + m.repeat(ATT_B, 1, 1).unsqueeze(1)
    return s


def _merge(o):
    return o.transpose(1, 2).reshape(o.shape[0] * 64, -1)


def att_fwd(case, R=None):
    """R None: float64 softmax(logits) v.  Else the kernel's arithmetic (edge_cases.attention_emu): float32 logits, the unnormalised
    probabilities rounded (``p``), 1 / sum applied to the float32 product, the result rounded (``o``)."""
    if R is None:
        return _merge(torch.softmax(att_logits(case, torch.float64), -1) @ case["vt"].double().transpose(-1, -2))
    s = att_logits(case, torch.float32)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    return R.r("o", _merge((R.r("p", e) @ case["vt"].float().transpose(-1, -2)) / e.sum(-1, keepdim=True)))


def att_bwd(case, R=None):
    """(dq, dk, dv) as edge_cases.attention_bwd: float32 logits, softmax, dP and dS; the normalised P (``p``) and dS (``ds``) rounded as MFMA
    operands; the three products rounded (``dq``, ``dk``, ``dv``)"""
    dt = torch.float64 if R is None else torch.float32
    nW, heads, hd = case["nW"], case["heads"], case["hd"]
    q, k, v = case["q"].to(dt), case["k"].to(dt), case["vt"].to(dt).transpose(-1, -2)
    do = case["do"].to(dt).reshape(nW, 64, heads, hd).permute(0, 2, 1, 3)
    s = att_logits(case, dt)
    dp = do @ v.transpose(-1, -2)
    if R is None:
        p = torch.softmax(s, -1)
        dot = (p * dp).sum(-1, keepdim=True)
        r = lambda n, t: t                                                       # noqa: E731
    else:
        e = torch.exp2((s - s.amax(-1, keepdim=True)) * torch.tensor(math.log2(math.e), dtype=dt))
        first = hd == 64
        p = e * (1.0 / E.lane_sum(e, first))
        dot = E.lane_sum(p * dp, first)
        r = R.r
    ds = p * (dp - dot)
    dsr, pr = r("ds", ds), r("p", p)
    return {"dq_f32": dsr @ k, "dq": r("dq", dsr @ k), "dk": r("dk", dsr.transpose(-1, -2) @ q), "dv": r("dv", pr.transpose(-1, -2) @ do),
            "dq_scaled": r("dq", (dsr @ k) * torch.tensor(float(hd) ** -0.5, dtype=torch.float32).to(dt))}


ATT_BWD_OUTPUTS = {"dq": ("ds", "dq"), "dk": ("ds", "dk"), "dv": ("p", "dv")}      # output -> the rounding points in front of it


# 4 x 4 windows: no intermediate rounding (P, dP and dS stay float32, csrc/uf_win4.hip): the only switch is the final store
ATT4_MAP = (1, 16, 16)                   # 16 windows
ATT4_CASES = [(2, 16), (2, 32)]          # (heads, head_dim)


@functools.lru_cache(maxsize=None)
def att4_case(heads, hd, dtype, seed=0):
    B, H, W = ATT4_MAP
    g = torch.Generator().manual_seed(1700 + 100 * seed + 10 * heads + hd)
    C, M = heads * hd, B * H * W
    qkv = torch.randn(M, 3 * C, generator=g)
    qkv[:, :C] *= 0.5
    return {"qkv": qkv.to(dtype), "rpb4": (0.5 * torch.randn(heads, 49, generator=g)).contiguous(), "do": torch.randn(M, C, generator=g).to(dtype),
            "heads": heads, "hd": hd}


def _win4(t, heads, hd, back=False):
    """(M, C) raster rows <-> (nW, heads, 16, hd)"""
    B, H, W = ATT4_MAP
    if not back:
        return t.reshape(B, H // 4, 4, W // 4, 4, heads, hd).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, heads, 16, hd)
    return t.reshape(B, H // 4, W // 4, heads, 4, 4, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B * H * W, heads * hd)


def att4(case, R=None):
    """{"o", "dq", "dk", "dv"} raster rows (M, C): float64, or float32 with the final stores rounded (``o``, ``dq``, ``dk``, ``dv``)"""
    dt = torch.float64 if R is None else torch.float32
    r = (lambda n, t: t) if R is None else R.r
    heads, hd = case["heads"], case["hd"]
    C = heads * hd
    qkv = case["qkv"].to(dt)
    q, k, v, do = (_win4(t, heads, hd) for t in (qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], case["do"].to(dt)))
    sc = torch.tensor(float(hd) ** -0.5, dtype=torch.float32).to(dt)
    s = (q @ k.transpose(-1, -2)) * sc + case["rpb4"].to(dt)[:, X.rpb_index(4)].unsqueeze(0)
    p = torch.softmax(s, -1)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    back = lambda t: _win4(t, heads, hd, back=True)                           # noqa: E731
    return {"o": r("o", back(p @ v)), "dq": r("dq", back((ds @ k) * sc)), "dk": r("dk", back((ds.transpose(-1, -2) @ q) * sc)),
            "dv": r("dv", back(p.transpose(-1, -2) @ do))}


# fused LN-GEMMs, the fused LeFF half, the fused FFN
LNG_MAP = (2, 16, 16)                    # B, H, W: 512 rows, 8 windows
LN_QKV_CASES = [(32, 1, 0), (32, 1, 4), (256, 8, 4)]      # (C, heads, shift)
LN_L1_CASES = [32, 256]
DWL2_CASES = [32, 128]
FFN_CASES = [64, 256]


def _ln32(x, gamma, beta):
    return E.ln_emu(x, gamma, beta, F32)


@functools.lru_cache(maxsize=None)
def lng_case(C, dtype, seed=0):
    """x f32 rows, LayerNorm affine, modulator, and T-valued GEMM weights of the three fused kernels"""
    B, H, W = LNG_MAP
    g = torch.Generator().manual_seed(2100 + 100 * seed + C)
    M = B * H * W
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3).float()
    gm, bt = E.ln_affine(C)
    mod = (0.5 * torch.randn(64, C, generator=g)).float()
    wq, bq = E.gemm_weights(3 * C, C, dtype, 2200 + seed)
    w1, b1 = E.gemm_weights(4 * C, C, dtype, 2300 + seed)
    w2, b2 = E.gemm_weights(C, 4 * C, dtype, 2400 + seed)
    h1 = torch.randn(M, 4 * C, generator=g).to(dtype)
    w9, bdw = (torch.randn(9, 4 * C, generator=g) / 3).float(), (0.1 * torch.randn(4 * C, generator=g)).float()
    return {"x": x, "gamma": gm, "beta": bt, "mod": mod, "wq": wq, "bq": bq.float(), "w1": w1, "b1": b1.float(), "w2": w2, "b2": b2.float(), "h1": h1,
            "w9": w9, "bdw": bdw}


def ln_qkv(c, heads, shift, R=None):
    """{"q", "k", "v"} (M, C) window-order rows: LN1 -> roll, partition, + modulator -> rounded (``xn``) -> projection -> q times head_dim^-0.5 -> rounded (``qkv``)"""
    B, H, W = LNG_MAP
    dt = torch.float64 if R is None else torch.float32
    r = (lambda n, t: t) if R is None else R.r
    C = c["x"].shape[1]
    y = E.ln_ref(c["x"], c["gamma"], c["beta"]) if R is None else _ln32(c["x"], c["gamma"], c["beta"])
    tok = X.window_tokens(B, H, W, shift)
    xn = r("xn", y[tok] + c["mod"].to(dt).repeat(len(tok) // 64, 1))
    out = xn @ c["wq"].to(dt).t() + c["bq"].to(dt)
    sc = torch.tensor(float(C // heads) ** -0.5, dtype=torch.float32).to(dt)
    return {"q": r("qkv", out[:, :C] * sc), "k": r("qkv", out[:, C:2 * C]), "v": r("qkv", out[:, 2 * C:])}


def ln_linear_gelu(c, R=None):
    """LN2 -> rounded (``xn``) -> linear1 -> GELU (the type's sigmoid form in both) -> rounded (``h1``)"""
    if R is None:
        return E.gelu_ref(E.ln_ref(c["x"], c["gamma"], c["beta"]) @ c["w1"].double().t() + c["b1"].double(), BF16)
    z = R.r("xn", _ln32(c["x"], c["gamma"], c["beta"]))
    return R.r("h1", gelu32(z @ c["w1"].float().t() + c["b1"]))


def dwconv_linear2(c, R=None):
    """the increment x_out - x_in: dwconv3x3(h1) + bias -> GELU -> rounded (``g2``) -> linear2 + bias"""
    B, H, W = LNG_MAP
    dt = torch.float64 if R is None else torch.float32
    hid = c["h1"].shape[1]
    h = c["h1"].to(dt).reshape(B, H, W, hid).permute(0, 3, 1, 2)
    a = F.conv2d(h, c["w9"].to(dt).t().reshape(hid, 1, 3, 3), c["bdw"].to(dt), padding=1, groups=hid).permute(0, 2, 3, 1).reshape(-1, hid)
    g2 = E.gelu_ref(a, BF16) if R is None else R.r("g2", gelu32(a))
    return g2 @ c["w2"].to(dt).t() + c["b2"].to(dt)


def ffn(c, R=None):
    """the increment of uf_ffn_fwd: LN2 -> rounded (``xn``) -> linear1 -> GELU -> rounded (``h1``) -> linear2 + bias"""
    if R is None:
        return ln_linear_gelu(c, None) @ c["w2"].double().t() + c["b2"].double()
    return ln_linear_gelu(c, R) @ c["w2"].float().t() + c["b2"]


# a whole LeWin block through oracle/bf16_budget.py's block (edge_cases.block_emu) with one rounding point truncating
BLOCK_CASES = [(32, 1, 0), (32, 1, 4)]                     # (C, heads, shift) on a 16 x 16 map, 4 images
BLOCK_MAP = (4, 16, 16)
BLOCK_POINTS = ("xn", "qkv", "p", "o", "z", "h1", "g2")     # the rounding points of BLOCK_SWITCHES (w: the weights are T already; gelu: a form, not a rounding)


@functools.lru_cache(maxsize=None)
def block_case(C, heads, shift, dtype, seed=0):
    """(x (B, H W, C) f32, the block's parameters with T-valued GEMM weights, the module): as tests/test_gpu_edges.py builds its blocks"""
    from uformer_amd import model
    B, H, W = BLOCK_MAP
    with torch.random.fork_rng():
        torch.manual_seed(3100 + 100 * seed + C + shift)
        blk = model.LeWinTransformerBlock(C, (H, W), heads, win_size=8, shift_size=shift, modulator=True)
        with torch.no_grad():
            for n, q in blk.named_parameters():                      # biases and tables away from their zero initial values
                if q.dim() == 1 or "table" in n:
                    q.add_(0.1 * torch.randn(q.shape))
        x = torch.randn(B, H * W, C)
    p = E.block_params({k: v.detach().clone() for k, v in blk.state_dict().items()}, dtype)
    return x, p, blk.eval()


def block_run(x, p, heads, shift, R=None):
    """the increment block(x) - x.  R None: the float64 block with the type's GELU form"""
    from oracle import bf16_budget as BB
    if R is None:
        pd = {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}
        return BB._block(x.double(), pd, "", heads, shift, Budget(("gelu",), "bf16")) - x.double()
    pf = {k: (v.float() if v.is_floating_point() else v) for k, v in p.items()}

    def ln_tree(x, w, b, eps=1e-5):
        C = x.shape[-1]
        v = x - E.tree_sum(x) * (1.0 / C)
        return v * (1.0 / torch.sqrt(E.tree_sum(v * v) * (1.0 / C) + eps)) * w + b
    R.on = R.on | {"gelu"}
    keep, BB.O.layer_norm = BB.O.layer_norm, ln_tree
    try:
        return BB._block(x.float(), pf, "", heads, shift, R) - x.float()
    finally:
        BB.O.layer_norm = keep


# measured on the CPU (three seeds): truncating z, h1 or g2 moves the slope of the whole block's increment by 1.5e-4 to 4e-4 (bf16), 2 to 8 times the
# nearest-even emulation's own slope -- the attention branch's roundings are the noise they would have to stand out of.  Not observable here; their kernels'
# own cases (SWITCH_OWNERS) see them at 60 to 500 times.
BLOCK_OBSERVABLE = ("xn", "qkv", "p", "o")
BLOCK_NOT_OBSERVABLE = ("z", "h1", "g2")


def _merge_heads(t):
    return t.permute(0, 2, 1, 3).reshape(t.shape[0] * 64, -1)


def kind_b_jobs(entry, case, *args):
    """[(output label, float64 reference, run(Rounder) -> emulation, switches, final switch or None)] of one case of one entry point"""
    if entry == "uf_window_attention_fwd":
        return [("o", att_fwd(case), lambda R: att_fwd(case, R), ("p", "o"), "o")]
    if entry in ("uf_window_attention_bwd", "uf_window_attention_bwd_qkv"):
        ref = att_bwd(case)
        key = {"dq": "dq_scaled" if entry.endswith("qkv") else "dq", "dk": "dk", "dv": "dv"}
        return [(o, ref[key[o]], (lambda R, o=o: att_bwd(case, R)[key[o]]), sw, sw[-1]) for o, sw in ATT_BWD_OUTPUTS.items()]
    if entry in ("uf_window4_attention_fwd", "uf_window4_attention_bwd"):
        ref = att4(case)
        outs = ("o",) if entry.endswith("fwd") else ("dq", "dk", "dv")
        return [(o, ref[o], (lambda R, o=o: att4(case, R)[o]), (o,), o) for o in outs]
    if entry == "uf_ln_qkv_fwd":
        heads, shift = args
        ref = ln_qkv(case, heads, shift)
        return [(o, ref[o], (lambda R, o=o: ln_qkv(case, heads, shift, R)[o]), ("xn", "qkv"), "qkv") for o in ("q", "k", "v")]
    if entry == "uf_ln_linear_gelu_fwd":
        return [("h1", ln_linear_gelu(case), lambda R: ln_linear_gelu(case, R), ("xn", "h1"), "h1")]
    if entry == "uf_dwconv_linear2_fwd":
        return [("dx", dwconv_linear2(case), lambda R: dwconv_linear2(case, R), ("g2",), None)]
    if entry == "uf_ffn_fwd":
        return [("dx", ffn(case), lambda R: ffn(case, R), ("xn", "h1"), None)]
    if entry == "uf_lewin_block_fwd":
        heads, shift = args
        x, p, _ = case
        return [("dx", block_run(x, p, heads, shift), lambda R: block_run(x, p, heads, shift, Rounder(BLOCK_POINTS, R.dtype, R.modes)), BLOCK_OBSERVABLE, None)]
    raise KeyError(entry)


def kind_b_cases(entry, dtype, seed=0):
    """[(case label, case, extra arguments of kind_b_jobs)] of one entry point"""
    tag = TAG[dtype]
    if entry in ("uf_window_attention_fwd", "uf_window_attention_bwd", "uf_window_attention_bwd_qkv"):
        return [(f"h{h}_d{hd}_s{sh}/{tag}", diffuse_case(h, hd, sh, dtype, seed), ()) for h, hd, sh in ATT_CASES]
    if entry in ("uf_window4_attention_fwd", "uf_window4_attention_bwd"):
        return [(f"h{h}_d{hd}/{tag}", att4_case(h, hd, dtype, seed), ()) for h, hd in ATT4_CASES]
    if entry == "uf_ln_qkv_fwd":
        return [(f"C{C}_h{h}_s{sh}/{tag}", lng_case(C, dtype, seed), (h, sh)) for C, h, sh in LN_QKV_CASES]
    if entry in ("uf_ln_linear_gelu_fwd", "uf_dwconv_linear2_fwd", "uf_ffn_fwd"):
        cs = {"uf_ln_linear_gelu_fwd": LN_L1_CASES, "uf_dwconv_linear2_fwd": DWL2_CASES, "uf_ffn_fwd": FFN_CASES}[entry]
        return [(f"C{C}/{tag}", lng_case(C, dtype, seed), ()) for C in cs]
    if entry == "uf_lewin_block_fwd":
        return [(f"C{C}_h{h}_s{sh}/{tag}", block_case(C, h, sh, dtype, seed), (h, sh)) for C, h, sh in BLOCK_CASES]
    raise KeyError(entry)


KIND_B_ENTRY_POINTS = ["uf_window_attention_fwd", "uf_window_attention_bwd", "uf_window_attention_bwd_qkv", "uf_window4_attention_fwd", "uf_window4_attention_bwd",
                       "uf_ln_qkv_fwd", "uf_ln_linear_gelu_fwd", "uf_dwconv_linear2_fwd", "uf_ffn_fwd", "uf_lewin_block_fwd"]
KIND_A_ENTRY_POINTS = ["uf_gelu_fwd", "uf_gelu_bwd", "uf_linear_fwd", "uf_linear_pre_gelu_fwd", "uf_linear_mul_dgelu", "uf_dwconv3x3_gelu_fwd", "uf_dwconv3x3_fwd",
                       "uf_dwconv3x3_pre_gelu_fwd", "uf_dwconv3x3_mul_dgelu", "uf_dwconv3x3_bwd", "uf_layernorm_fwd"]
# the rounding points of a block (BLOCK_POINTS) and of the attention backward, each with the entry point whose own case truncates it and the name it has there
# (asserted complete in tests/test_rounding_reference.py) (asserted complete in tests/test_rounding_reference.py)
SWITCH_OWNERS = {"xn": ("uf_ln_qkv_fwd", "xn"), "qkv": ("uf_ln_qkv_fwd", "qkv"), "p": ("uf_window_attention_fwd", "p"), "o": ("uf_window_attention_fwd", "o"),
                 "z": ("uf_ln_linear_gelu_fwd", "xn"), "h1": ("uf_ln_linear_gelu_fwd", "h1"), "g2": ("uf_dwconv_linear2_fwd", "g2"),
                 "ds": ("uf_window_attention_bwd", "ds")}


def dump_report(fname="parity_rounding.json"):
    """RECORDS and STATS to $UF_REPORT_DIR/parity_rounding.json when that variable names a directory (as tests/test_gpu_edges.py does)"""
    out = os.environ.get("UF_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, fname), "w") as f:
            json.dump({"kind_a": RECORDS, "kind_b": STATS}, f, indent=1, sort_keys=True)
