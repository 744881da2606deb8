"""Exact checks of the fused NONLINEAR kernels on saturated lattices (helpers; no GPU needed).

tests/exact_lattice.py gates every linear kernel at zero.  The fused block kernels contain a LayerNorm, a softmax or a GELU, which are exact
on no lattice in general -- but each has inputs on which the kernels' own float32 arithmetic returns an exact value:

  GELU, 2-byte types (gelu_bf2 in csrc/uf_common.h: x * rcp(1 + exp2(x (A + B x^2)))): for x >= 6 the exponent is below -24, the denominator is
      1.0f and the result is x; for x <= -11 the exponent exceeds 128, exp2 returns inf and the result is -0.  f32 (gelu_erf): erff is +-1
      for |x| >= 8, so the result is x or -0.  Every pre-activation here lies in [8, 256] or [-256, -15] (``check_saturated``; -15, because the
      float64 erf form itself is below the float32 subnormals only from -14.5 on).
  LayerNorm, 2-byte types: a row a * s with s a balanced +-1 pattern and C a power of two has float32 mean 0 and variance a^2 exactly; what eps
      leaves (1.5e-5 relative at worst) disappears when xn is rounded to T, provided the weight is an odd integer of at most 3 and bias +
      modulator are even integers: xn = s gamma + beta + modulator, odd, to the bit (``xn_lattice``).  f32 keeps xn unrounded, so f32 runs with
      LayerNorm weight 0 (xn = beta + modulator; the row gather is then NOT observed in f32).
  softmax: a winner ahead of every other key by 104 or more (150 in the log2 domain) leaves e = 1 for itself and exactly 0 for the rest; equal
      logits over n = 64 / 32 / 16 keys give e = 1 and sum n, whose reciprocal is a power of two.  Keys behind the -100 shift mask keep a float32
      subnormal e (flushed or not): it rounds to 0 as a 2-byte operand and disappears in the float32 sums, because no v entry is zero.

On such inputs a whole fused kernel is a linear map on small integers, and the gate is the one of exact_lattice: ``assert_exact`` against the
float64 evaluation of the DOCUMENTED formula (erf / sigmoid-form GELU, LayerNorm with eps, softmax), rounded once to T at each documented
rounding point (xn, q | k | v, e, o, h1, g2).  The float32 residual stream is not rounded.  Every condition is asserted on the float64 reference
alone, by the builders below, so tests/test_saturated_reference.py (CPU) and tests/test_gpu_saturated.py check the same cases.
"""
import functools
import math

import torch
import torch.nn.functional as F

import exact_lattice as X
from exact_lattice import BF16, F16, F32, PM1, PM2, check_accumulation, check_representable, lattice

HALF = [BF16, F16]
GELU_A, GELU_B = -2.3022081985, -0.10294324              # the float32 constants of gelu_bf2
# saturated pre-activations: [8, 256] and [-256, -15].  The kernels' own arithmetic saturates from 6 / -11 (2-byte) and +-8 (f32) on; the DOCUMENTED erf form
# in float64 still leaves -1e-27 at x = -11, a float32 value where the kernel stores -0: below -14.5 it is under half the smallest float32 subnormal
POS_MIN, NEG_MAX, PRE_MAX = 8, -15, 256
MARGIN = 104.0                                           # exp(-104) = 2^-150.04: below half the smallest float32 subnormal
LN_EPS = 1e-5


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------
# GELU
# ---------------------------------------------------------------------------------------------------------------------------
def gelu_doc64(x64, dtype):
    """the documented activation in float64: the erf form for f32, the sigmoid form x / (1 + 2^(x (A + B x^2))) for the 2-byte types"""
    if dtype == F32:
        return 0.5 * x64 * torch.special.erfc(-x64 / math.sqrt(2.0))
    a, b = float(torch.tensor(GELU_A, dtype=F32)), float(torch.tensor(GELU_B, dtype=F32))
    return x64 / (1.0 + torch.exp2(x64 * (a + b * x64 * x64)))


def gelu_kernel_f32(x32, dtype):
    """float32 emulation of the kernels' own arithmetic (gelu_erf / gelu_bf2), operation by operation"""
    assert x32.dtype == F32
    if dtype == F32:
        return torch.tensor(0.5, dtype=F32) * x32 * (1.0 + torch.erf(x32 * torch.tensor(0.70710678118654752440, dtype=F32)))
    a, b = torch.tensor(GELU_A, dtype=F32), torch.tensor(GELU_B, dtype=F32)
    u = x32 * (x32 * x32 * b + a)
    return x32 * (1.0 / (torch.exp2(u) + 1.0))


def check_saturated(pre64, min_share=0.25):
    """every pre-activation is an integer in [8, 256] or [-256, -15], and each branch holds at least a quarter of them (a skipped GELU shows)"""
    assert torch.equal(pre64, pre64.round())
    pos, neg = pre64 >= POS_MIN, pre64 <= NEG_MAX
    assert bool((pos | neg).all()), f"pre-activations inside ({NEG_MAX}, {POS_MIN}): {pre64[~(pos | neg)][:4].tolist()}"
    assert float(pre64.abs().max()) <= PRE_MAX
    shares = (float(pos.double().mean()), float(neg.double().mean()))
    assert min(shares) >= min_share, f"branch shares {shares}"
    return shares


def gelu_saturated(pre64, dtype):
    """GELU of saturated pre-activations as stored in T: the documented formula rounded once, which must be the lattice value (x or -0)"""
    check_saturated(pre64, min_share=0.0)
    g = gelu_doc64(pre64, dtype).to(dtype)
    want = torch.where(pre64 > 0, pre64, torch.full_like(pre64, -0.0)).to(dtype)
    assert torch.equal(X._bits(g), X._bits(want)), "the documented GELU does not round to the lattice value"
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# rows and LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hadamard(n):
    """Sylvester Hadamard matrix of order n (a power of two), float64 +-1; every row but the first is balanced"""
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == n
    return h


AMPLITUDES = (1, 2, 3, 5, 8)


def balanced_rows(M, C, seed, amps=AMPLITUDES):
    """M rows a * s: s a balanced +-1 pattern over the C channels (a signed Hadamard row, never the first), a an amplitude -> (rows, s)"""
    g = gen(seed)
    r = torch.randint(1, C, (M,), generator=g)
    sign = torch.randint(2, (M,), generator=g).double() * 2 - 1
    a = torch.tensor(amps, dtype=torch.float64)[torch.randint(len(amps), (M,), generator=g)]
    s = hadamard(C)[r] * sign[:, None]
    assert bool((s.sum(1) == 0).all())
    return s * a[:, None], s


def pick(values, shape, seed):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(len(values), tuple(shape), generator=gen(seed))]


def ln_params(C, seed, dtype):
    """LayerNorm weight and bias.  2-byte types: weight odd (+-1, +-3), bias even (0, +-2).  f32: weight 0 and an odd bias"""
    if dtype == F32:
        return torch.zeros(C, dtype=torch.float64), pick((-3, -1, 1, 3), (C,), seed + 1)
    return pick((-3, -1, 1, 3), (C,), seed), pick((-2, 0, 2), (C,), seed + 1)


def modulator_rows(C, seed):
    return pick((-2, 0, 2, 4), (64, C), seed)


def ln_doc64(x64, gamma, beta):
    mean = x64.mean(1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(1, keepdim=True)
    return (x64 - mean) / torch.sqrt(var + LN_EPS) * gamma + beta


def ln_kernel_f32(x32, gamma, beta, mod=None):
    """float32 emulation of phase 0 of the LN-fused kernels: mean = sum / C, centred squares, rstd = 1 / sqrt(var + eps), y = v rstd gamma + beta (+ mod)"""
    C = x32.shape[1]
    inv = torch.tensor(1.0 / C, dtype=F32)
    mean = x32.sum(1, keepdim=True) * inv
    v = x32 - mean
    rstd = 1.0 / torch.sqrt((v * v).sum(1, keepdim=True) * inv + torch.tensor(LN_EPS, dtype=F32))
    y = v * rstd * gamma.float() + beta.float()
    return y if mod is None else y + mod.float()


def xn_lattice(x64, s, gamma, beta, mod, dtype):
    """xn as the kernels hold it (T): the documented LayerNorm (+ modulator row) in float64, rounded once -- which must be s gamma + beta + mod"""
    doc = ln_doc64(x64, gamma, beta) + (0.0 if mod is None else mod)
    xn = doc.to(dtype)
    want = s * gamma + beta + (0.0 if mod is None else mod)
    assert torch.equal(xn.double(), want), "the documented LayerNorm does not round to the lattice value"
    if dtype != F32:
        assert bool((want.abs() % 2 == 1).all()), "xn must be odd: an even sum could cancel to zero"
    return want


def sparse_pm1(N, K, seed, nnz=3):
    """(N, K) weight with nnz entries of +-1 per row, zero elsewhere: an odd number of odd terms stays odd"""
    g = gen(seed)
    w = torch.zeros(N, K, dtype=torch.float64)
    cols = torch.rand(N, K, generator=g).argsort(1)[:, :nnz]
    w.scatter_(1, cols, torch.randint(2, (N, nnz), generator=g).double() * 2 - 1)
    return w


def saturating_bias(N, bound, seed):
    """per-channel bias that puts a sum of magnitude <= bound into [8, 8 + 2 bound] or [-15 - 2 bound, -15], the branch drawn per channel"""
    g = gen(seed)
    up = torch.randint(2, (N,), generator=g).bool()
    return torch.where(up, torch.tensor(float(POS_MIN + bound)), torch.tensor(float(NEG_MAX - bound))).double()


# ---------------------------------------------------------------------------------------------------------------------------
# LN -> linear1 -> GELU (uf_ln_linear_gelu_fwd) and the Mlp feed-forward (uf_ffn_fwd)
# ---------------------------------------------------------------------------------------------------------------------------
WIDTHS = [16, 32, 64, 128, 256, 512]
# (M, C): M = 130 has a row tail in the second 64-row block; 128-row blocks are chosen from 128 * 512 rows on where the operand tile fits
# (launch_bm in csrc/uf_lngemm.hip): one case there, with a row tail
LNL1_CASES = [(130, C) for C in WIDTHS] + [(128 * 512 + 72, 16)]
# (B, M, C): uf_ffn_fwd takes whole 64-row tiles only; three images of 64 tokens = one tile per image
FFN_CASES = [(3, 192, C) for C in WIDTHS] + [(3, 576, 256), (3, 576, 512)]      # uf_mlp_fwd reaches its unfused pair of launches ("ffn=1"; the default at C = 512, 2-byte types) only with M >= C
FFN_SCALES = (None, (0.0, 2.0, 1.0))


@functools.lru_cache(maxsize=None)
def lnl1_case(M, C, dtype):
    x, s = balanced_rows(M, C, 100 + C)
    gamma, beta = ln_params(C, 110 + C, dtype)
    xn = xn_lattice(x, s, gamma, beta, None, dtype)
    w1 = sparse_pm1(4 * C, C, 120 + C)
    bound = 3 * int(xn.abs().max())
    b1 = saturating_bias(4 * C, bound, 130 + C)
    pre = xn @ w1.t() + b1
    check_accumulation(3, (int(xn.abs().max()),), PM1, addend_steps=int(b1.abs().max()))
    shares = check_saturated(pre)
    h1 = gelu_saturated(pre, dtype)
    return {"x": x, "s": s, "gamma": gamma, "beta": beta, "xn": xn, "w1": w1, "b1": b1, "pre": pre, "h1": h1, "shares": shares}


@functools.lru_cache(maxsize=None)
def ffn_case(B, M, C, dtype):
    c = dict(lnl1_case(M, C, dtype))
    w2, b2 = lattice((C, 4 * C), PM1, 140 + C), lattice((C,), PM2, 150 + C)
    hmax = int(c["h1"].double().abs().max())
    check_accumulation(4 * C, (hmax,), PM1, addend_steps=2 + 8)
    kstep_live = (c["pre"] > 0).double().reshape(M, -1, 32).sum(2)
    assert float(kstep_live.min()) >= 4, "a 32-wide k-step of fc2 with (almost) no live hidden channel: dropping it would not show"
    c.update(w2=w2, b2=b2, branch=c["h1"].double() @ w2.t() + b2)
    return c


def ffn_out(c, B, scale):
    s = torch.ones(B, dtype=torch.float64) if scale is None else torch.tensor(scale, dtype=torch.float64)
    M = c["x"].shape[0]
    return c["x"] + s.repeat_interleave(M // B)[:, None] * c["branch"]


# ---------------------------------------------------------------------------------------------------------------------------
# LN1 -> roll -> window partition -> + modulator -> q | k | v^T (uf_ln_qkv_fwd)
# ---------------------------------------------------------------------------------------------------------------------------
# (B, H, W, C, heads, shift, modulator): head widths 16 / 32 / 64, every C; 8 x 24 with B = 3 is 9 windows (a half-filled second 128-row block never
# occurs below 65536 rows: the 64-row form runs, one window per block)
LNQKV_CASES = [(1, 16, 16, 16, 1, 4, True), (3, 8, 24, 32, 1, 4, True), (1, 16, 16, 32, 2, 0, False), (1, 16, 16, 64, 2, 4, True), (3, 8, 24, 64, 1, 0, True),
               (1, 16, 16, 128, 4, 4, True), (1, 16, 16, 128, 2, 0, False), (1, 16, 16, 256, 8, 4, True), (1, 8, 8, 512, 16, 4, True), (1, 8, 8, 512, 8, 0, True)]


@functools.lru_cache(maxsize=None)
def lnqkv_case(B, H, W, C, heads, shift, use_mod, dtype):
    M = B * H * W
    x, s = balanced_rows(M, C, 200 + C + H)
    gamma, beta = ln_params(C, 210 + C, dtype)
    mod = modulator_rows(C, 220 + C) if use_mod else None
    tok = X.window_tokens(B, H, W, shift)
    mod_rows = None if mod is None else mod.repeat(M // 64, 1)
    xn = xn_lattice(x[tok], s[tok], gamma, beta, mod_rows, dtype)                 # window-row order
    w, b = sparse_pm1(3 * C, C, 230 + C), lattice((3 * C,), PM2, 240 + C)
    P = xn @ w.t() + b
    check_accumulation(3, (int(xn.abs().max()),), PM1, addend_steps=2)
    check_representable(P, dtype)
    q, k, vt = X.ref_qkv(P, M, C, heads)
    return {"x": x, "s": s, "gamma": gamma, "beta": beta, "mod": mod, "tok": tok, "xn": xn, "w": w, "b": b, "P": P, "q": q, "k": k, "vt": vt}


# ---------------------------------------------------------------------------------------------------------------------------
# the same producer for a ConvProjection (uf_ln_convqkv_fwd) with a LIVE LayerNorm (tests/test_gpu_convproj.py has the case with weight 0, all types)
# ---------------------------------------------------------------------------------------------------------------------------
# (B, H, W, C, heads, shift): more than one head, head widths 16 / 32 / 64
CONVQKV_CASES = [(1, 16, 16, 32, 2, 4), (3, 8, 24, 64, 4, 0), (1, 16, 16, 64, 2, 4), (1, 16, 16, 128, 2, 4), (1, 8, 8, 256, 8, 4), (1, 8, 8, 512, 16, 0)]
CONV_TAPS = tuple(t / 2 for t in range(-4, 5))           # the nine distinct multiples of 1/2 in [-2, 2], as the lattice of tests/test_gpu_convproj.py


@functools.lru_cache(maxsize=None)
def convqkv_case(B, H, W, C, heads, shift, dtype):
    """xn = s gamma + modulator with |gamma| = 1, bias 0 and an even modulator in {0, +-2}: |xw| <= 3, the stencil + bias + ReLU stays within 31 (62 halves) and
    the pointwise rows (three entries of +-1) within 94 (188 halves): T values in bf16's 8 significant bits.  The stencil is zero padded at the WINDOW border."""
    assert dtype != F32
    M = B * H * W
    n = M // 64
    x, s = balanced_rows(M, C, 250 + C + H)
    gamma, beta = pick((-1, 1), (C,), 251 + C), torch.zeros(C, dtype=torch.float64)
    mod = pick((-2, 0, 2), (64, C), 252 + C)
    tok = X.window_tokens(B, H, W, shift)
    xn = xn_lattice(x[tok], s[tok], gamma, beta, mod.repeat(n, 1), dtype)
    g = gen(253 + C)
    taps = torch.tensor(CONV_TAPS, dtype=torch.float64)[torch.rand(3, C, 9, generator=g).argsort(2)]          # (3, C, 9): tap = ky * 3 + kx
    bdw = pick((-1, 0, 1), (3, C), 254 + C)
    wpw, bpw = sparse_pm1(3 * C, C, 255 + C), pick((-1, 0, 1), (3 * C,), 256 + C)
    img = xn.reshape(n, 64, C).transpose(1, 2).reshape(n, C, 8, 8)
    outs = []
    for j in range(3):
        pj = F.relu(F.conv2d(img, taps[j].reshape(C, 1, 3, 3), bdw[j], padding=1, groups=C))
        check_representable(pj, dtype, step=0.5)                                                              # P is stored as T
        assert float((pj > 0).double().mean()) > 0.25 and float((pj == 0).double().mean()) > 0.25            # both sides of the ReLU
        outs.append(pj.reshape(n, C, 64).transpose(1, 2).reshape(M, C) @ wpw[j * C:(j + 1) * C].t() + bpw[j * C:(j + 1) * C])
    P = torch.cat(outs, 1)
    check_representable(P, dtype, step=0.5)
    check_accumulation(10, (3,), (4,), addend_steps=2)
    q, k, vt = X.ref_qkv(P, M, C, heads)
    return {"x": x, "gamma": gamma, "beta": beta, "mod": mod, "dw9": taps.transpose(1, 2).contiguous(), "bdw": bdw, "wpw": wpw, "bpw": bpw, "q": q, "k": k, "vt": vt}


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise 3x3 -> GELU -> linear2 -> residual (uf_dwconv_linear2_fwd)
# ---------------------------------------------------------------------------------------------------------------------------
TAPS = (-4, -3, -2, -1, 1, 2, 3, 4, 5)                   # the nine taps of a channel are a permutation of these: all distinct
H1_VALUES = (1, 2, 3)
# (B, H, W, C): 8 x 8 is all border, 16 x 16 has an inner seam in both directions, 8 x 24 with B = 3 is 9 tiles
LEFF2_MAPS = [(1, 8, 8), (2, 16, 16), (3, 8, 24)]
LEFF2_CASES = [(B, H, W, C) for C in (32, 64, 128, 256, 512) for (B, H, W) in LEFF2_MAPS] + [(1, 16, 16, 16)]
LEFF2_VARIANTS = [None, "leff2=1", "leff2=2"]            # "persist=" changes nothing below: it takes effect only with more tiles than resident workgroups
# More tiles than resident workgroups (launch_v in csrc/uf_leff2.hip: 2-byte C <= 128 holds 3 workgroups per CU = 768, f32 one = 256), 832 tiles:
# at C = 32 the default launch walks ("persist=0": one tile per workgroup); at C = 64 the default does not and "persist=1" makes it
LEFF2_WALK_CASES = [((13, 64, 64, 32), (None, "persist=0")), ((13, 64, 64, 64), ("persist=1", None))]


@functools.lru_cache(maxsize=None)
def leff2_case(B, H, W, C, dtype):
    hid = 4 * C
    g = gen(300 + C + H)
    h1 = lattice((B, H, W, hid), H1_VALUES, 301 + C + W)
    taps = torch.tensor(TAPS, dtype=torch.float64)[torch.rand(hid, 9, generator=g).argsort(1)]             # (hid, 9), tap = ky * 3 + kx
    assert all(len(set(r.tolist())) == 9 for r in taps[:8])
    pos, neg = sum(t for t in TAPS if t > 0), -sum(t for t in TAPS if t < 0)
    hi, lo = max(H1_VALUES) * pos - min(H1_VALUES) * 0, max(H1_VALUES) * neg                               # at a border any subset of taps is missing
    up = torch.randint(2, (hid,), generator=g).bool()
    jitter = torch.randint(3, (hid,), generator=g).double()
    bdw = torch.where(up, POS_MIN + lo + jitter, NEG_MAX - hi - jitter)
    pre = F.conv2d(h1.permute(0, 3, 1, 2), taps.reshape(hid, 1, 3, 3), bdw, padding=1, groups=hid).permute(0, 2, 3, 1)      # (B, H, W, hid)
    check_accumulation(9, H1_VALUES, TAPS, addend_steps=int(bdw.abs().max()))
    shares = check_saturated(pre)
    g2 = gelu_saturated(pre, dtype)
    w2, b2 = lattice((C, hid), PM1, 310 + C), lattice((C,), PM2, 311 + C)
    x = lattice((B * H * W, C), PM2, 312 + C + H)
    check_accumulation(hid, (int(pre.abs().max()),), PM1, addend_steps=4)
    kstep_live = up.double().reshape(-1, 32).sum(1)
    assert float(kstep_live.min()) >= 4, "a 32-wide k-step of linear2 with (almost) no live hidden channel"
    out = x + g2.double().reshape(-1, hid) @ w2.t() + b2
    return {"h1": h1, "taps": taps, "w9": taps.t().contiguous(), "bdw": bdw, "pre": pre, "g2": g2, "w2": w2, "b2": b2, "x": x, "out": out, "shares": shares, "up": up}


def leff2_out(c, h1=None, pad_value=0.0, gelu=True, seam_shift=False, seam_channels=None, drop_kstep=None, drop_channel=None, dtype=BF16):
    """the reference of leff2_case again under one fault (stand-ins of tests/test_saturated_reference.py):
    pad_value: what a tap outside the image reads; seam_shift: the halo column right of the tile seam x = 8 read one pixel further right (in the channels
    ``seam_channels``, a slice; None: all); gelu = False: the activation skipped; drop_kstep: one 32-wide k-step of linear2 left out; drop_channel: one term"""
    h1 = c["h1"] if h1 is None else h1
    B, H, W, hid = h1.shape
    hp = F.pad(h1.permute(0, 3, 1, 2), (1, 1, 1, 1), value=pad_value)
    pre = F.conv2d(hp, c["taps"].reshape(hid, 1, 3, 3), c["bdw"], groups=hid)
    if seam_shift:                                                       # output column 7 takes its right neighbours from column 9 instead of 8
        hs = hp.clone()
        hs[:, :, :, 9] = hp[:, :, :, 10]
        ch = slice(None) if seam_channels is None else seam_channels
        pre[:, ch, :, 7] = F.conv2d(hs, c["taps"].reshape(hid, 1, 3, 3), c["bdw"], groups=hid)[:, ch, :, 7]
    pre = pre.permute(0, 2, 3, 1)
    g2 = gelu_doc64(pre, dtype).to(dtype).double() if gelu else pre
    g2, w2 = g2.reshape(-1, hid), c["w2"]
    if drop_kstep is not None or drop_channel is not None:
        keep = torch.ones(hid, dtype=torch.bool)
        if drop_kstep is not None:
            keep[32 * drop_kstep:32 * drop_kstep + 32] = False
        else:
            keep[drop_channel] = False
        g2, w2 = g2[:, keep], w2[:, keep]
    return c["x"] + g2 @ w2.t() + c["b2"]


# ---------------------------------------------------------------------------------------------------------------------------
# window attention core (uf_window_attention_fwd), directly on q | k | v^T
# ---------------------------------------------------------------------------------------------------------------------------
# v^T rows: one sign per (window, head, channel) times a magnitude of 1 or 3.  Odd: no zero entry, and a mean over n keys is a multiple of 1 / n.  One sign
# per row: no sum over a subset of keys is zero, so what the masked keys' float32 subnormals add (flushed or not) never decides a result
V_VALUES = (1, 3)
KINDS = ("onehot", "uniform", "table")
# (B, H, W, heads, head_dim, shift, kind).  B = 3 on 8 x 24 is 9 windows: with heads = 1 the pair count is not a multiple of the 4 pairs per workgroup
ATTN_CASES = ([(1, 16, 16, hd_heads[1], hd_heads[0], shift, "onehot") for hd_heads in ((16, 2), (32, 1), (32, 4), (64, 2)) for shift in (0, 4)]
              + [(3, 8, 24, 1, hd, 4, "onehot") for hd in (16, 32, 64)]
              + [(1, 16, 16, 64 // hd, hd, 4, "uniform") for hd in (16, 32, 64)] + [(3, 8, 24, 1, 32, 4, "uniform"), (1, 16, 16, 2, 32, 0, "uniform")]
              + [(1, 16, 16, 64 // hd, hd, 0, "table") for hd in (16, 32, 64)] + [(3, 8, 24, 3, 32, 0, "table")])


def signed_codes(hd):
    h = hadamard(hd)
    return torch.cat([h, -h], 0)                                           # (2 hd, hd): code c and its negative c + hd (mod 2 hd)


def shift_mask64(H, W, shift):
    """(nW, 64, 64) float64 in {0, -100}: the SW-MSA mask of the reference (region ids of query and key differ)"""
    nWc, nW = W // 8, (H // 8) * (W // 8)
    t = torch.arange(64)
    out = torch.zeros(nW, 64, 64, dtype=torch.float64)
    if shift == 0:
        return out
    for wi in range(nW):
        hh, ww = (wi // nWc) * 8 + t // 8, (wi % nWc) * 8 + t % 8
        region = torch.where(hh < H - 8, 0, torch.where(hh < H - shift, 1, 2)) * 3 + torch.where(ww < W - 8, 0, torch.where(ww < W - shift, 1, 2))
        out[wi] = torch.where(region[:, None] != region[None, :], -100.0, 0.0)
    return out


def _involution(groups, g):
    """fixed-point-free involution of 0..63 that maps every group of tokens (even sizes) onto itself"""
    pi = torch.empty(64, dtype=torch.long)
    for grp in groups:
        p = grp[torch.randperm(len(grp), generator=g)]
        pi[p[0::2]], pi[p[1::2]] = p[1::2], p[0::2]
    assert bool((pi[pi] == torch.arange(64)).all()) and bool((pi != torch.arange(64)).all())
    return pi


def _quadrants():
    t = torch.arange(64)
    return [t[((t // 8 >= 4) == bool(qy)) & ((t % 8 >= 4) == bool(qx))] for qy in (0, 1) for qx in (0, 1)]


def table_bias(heads, seed, peak=120.0):
    """(heads, 64, 64) relative-position bias gathered from a (225, heads) table that holds ``peak`` at ONE relative offset per head (never (0, 0),
    never symmetric) and 0 elsewhere -> (bias, table)"""
    g = gen(seed)
    table = torch.zeros(225, heads, dtype=torch.float64)
    offs = []
    for h in range(heads):
        while True:
            dy, dx = (int(v) for v in torch.randint(-3, 4, (2,), generator=g))
            if (dy, dx) != (0, 0) and (dy, dx) not in offs and (-dy, -dx) not in offs:
                break
        offs.append((dy, dx))
        table[(dy + 7) * 15 + dx + 7, h] = peak
    return table[X.rpb_index(8)].permute(2, 0, 1).contiguous(), table


def attn_doc64(q, k, vt, bias, mask, dtype):
    """softmax(q k^T + bias + mask) v in float64 with the documented rounding points: the unnormalised e rounded to T as an MFMA operand, o rounded
    to T.  q, k (n, heads, 64, hd), vt (n, heads, hd, 64) float64 -> (logits, e as T, sum, o float64 before its rounding, (n * 64, heads * hd))"""
    n, heads = q.shape[:2]
    s = q @ k.transpose(2, 3) + bias[None] + mask[torch.arange(n) % mask.shape[0]][:, None]
    e = torch.exp(s - s.max(3, keepdim=True).values)
    eT = e.to(dtype)
    o = (eT.double() @ vt.transpose(2, 3)) / e.sum(3, keepdim=True)
    return s, eT, e.sum(3), o.permute(0, 2, 1, 3).reshape(n * 64, -1)


@functools.lru_cache(maxsize=None)
def attn_case(B, H, W, heads, hd, shift, kind, dtype):
    nW = (H // 8) * (W // 8)
    n = B * nW
    g = gen(400 + hd + heads + shift + H)
    codes = signed_codes(hd)
    A = 128 // hd                                                          # a match scores A a hd >= 128, every other key 0 or -128 a
    mask = shift_mask64(H, W, shift)
    vt = pick(V_VALUES, (n, heads, hd, 64), 410 + hd + heads) * pick((-1, 1), (n, heads, hd, 1), 411 + hd + heads)
    q = torch.zeros(n, heads, 64, hd, dtype=torch.float64)
    k = torch.zeros_like(q)
    target = torch.full((n, heads, 64), -1, dtype=torch.long)             # the key a one-hot query selects (-1: none)
    quads, everything = _quadrants(), [torch.arange(64)]
    for w_ in range(n):
        for h in range(heads):
            # keys: a signed code times an amplitude.  head_dim 16 has 32 codes for 64 tokens: two tokens of one quadrant share a code and its amplitude
            if hd == 16:
                cperm = torch.randperm(32, generator=g)
                tcode = torch.empty(64, dtype=torch.long)
                for qi, grp in enumerate(quads):
                    p = grp[torch.randperm(16, generator=g)]
                    tcode[p] = cperm[8 * qi:8 * qi + 8].repeat(2)
            else:
                tcode = torch.randperm(2 * hd, generator=g)[:64]
            amp = torch.tensor((1.0, 2.0, 4.0), dtype=torch.float64)[torch.randint(3, (2 * hd,), generator=g)]
            k[w_, h] = codes[tcode] * amp[tcode][:, None]
            if kind == "onehot":
                pi = _involution(quads if (shift or hd == 16) else everything, g)
                q[w_, h] = A * codes[tcode[pi]]
                target[w_, h] = pi
    if kind == "onehot":                                                   # table entries within the margin; head_dim 16 shares winners, which must tie: a constant
        bias = torch.ones(heads, 64, 64, dtype=torch.float64) if hd == 16 else pick((-2, -1, 0, 1, 2), (225, heads), 420 + heads)[X.rpb_index(8)].permute(2, 0, 1).contiguous()
    elif kind == "uniform":
        bias = torch.full((heads, 64, 64), 3.0, dtype=torch.float64)
    else:
        bias, _ = table_bias(heads, 430 + heads + hd)
        assert shift == 0
    s, eT, esum, o = attn_doc64(q, k, vt, bias, mask, dtype)
    # conditions, on the reference alone
    e64 = eT.double()
    top = s.max(3, keepdim=True).values
    winners = s == top
    rest = torch.where(winners, torch.full_like(s, -1e9), s).max(3).values
    lead = top[..., 0] - rest
    n_win = winners.sum(3)
    # a key that loses is 104 behind, or (uniform case) behind the -100 shift mask: e then stays a float32 subnormal, covered by the next line and by v != 0
    assert bool(((lead >= (100.0 if kind == "uniform" else MARGIN)) | (n_win == 64)).all()), f"a non-winner within {float(lead.min())} of the winner"
    assert bool(((e64 == 1.0) | (e64 < 1e-40)).all()) and bool((e64[winners] == 1.0).all())
    if dtype != F32:
        assert bool(((e64 == 1.0) | (e64 == 0.0)).all())
    assert torch.equal(esum.float().double(), n_win.double()), "the float32 sum is not the number of winners"
    assert set(n_win.unique().tolist()) <= {1, 2, 16, 32, 64}
    exact = (winners.double() @ vt.transpose(2, 3) / n_win[..., None]).permute(0, 2, 1, 3).reshape(n * 64, -1)
    assert torch.equal(o.to(dtype).double(), exact), "the documented softmax does not round to the lattice value"
    check_representable(exact, dtype, step=1.0 / 64)
    check_accumulation(hd, (A,), (4,), addend_steps=103)
    if kind == "onehot":
        assert set(n_win.unique().tolist()) == ({2} if hd == 16 else {1})
        assert bool(winners.gather(3, target[..., None]).all()), "the selected key is not a winner"
    if kind == "uniform" and shift:
        assert {16, 32, 64} <= set(n_win.unique().tolist()) or (H // 8 == 1 and {16, 32} <= set(n_win.unique().tolist()))
    if kind == "table":
        assert {1, 64} <= set(n_win.unique().tolist())
    return {"q": q, "k": k, "vt": vt, "bias": bias, "mask": mask, "o": exact, "n_win": n_win, "lead": lead, "target": target, "n": n}


# ---------------------------------------------------------------------------------------------------------------------------
# the fused window kernel (uf_lewin_attn_fwd, uf_lewin_block_fwd, uf_lewin_attn_train_fwd): head_dim 32, C = 32 heads
# ---------------------------------------------------------------------------------------------------------------------------
LOG2E32 = torch.tensor(1.4426950408889634, dtype=F32)
QSCALE_PLAIN32 = torch.tensor(1.0 / math.sqrt(32.0), dtype=F32)
QSCALE32 = QSCALE_PLAIN32 * LOG2E32                       # what the fused kernel multiplies q with: the softmax runs in the log2 domain
MASK2 = float(torch.tensor(-100.0, dtype=F32) * LOG2E32)
Q_GAIN = 48                                              # Wq = Q_GAIN diag(h_r): a match leads by 32 * 48 * 32^-0.5 log2(e) = 392 in the log2 domain before the cross terms
LEAD2 = 160.0                                            # asserted lead in the log2 domain: 150 + slack for the rounding of q to T
BLOCK_KINDS = ("onehot", "self", "uniform", "table")
BLOCK_TAPS = (-4, -3, -2, -1, 0, 1, 2, 3, 4)             # nine distinct taps whose stencil of h1 <= 10 stays inside the bf16 integers (one tap of a channel is zero)
PROJ_GAIN = 2                                            # kind "self": Wproj Wv = 2 I


def _partner(code, r):
    """code index (row + 32 * negated) of the elementwise product with Hadamard row r: Sylvester rows multiply by xor of their indices"""
    return ((code % 32) ^ r) + 32 * (code // 32)


def place_codes(groups, r, single_head, g, fixed=None):
    """One head of one window: the signed-code index (0 .. 63: row + 32 * negated) of each of the 64 window positions.  Codes c and c * h_r (the key a
    query holding c selects) lie in the same group of positions (a mask region), so the selected key is never masked.  With several heads all 64 codes are
    used once; ``fixed`` {position: code} pins the two unbalanced codes (rows 0) where the neighbouring head cancels them.  A single head has only the
    62 balanced codes: 60 of them (closed under the pairing) once, and two further pairs twice -- a query that selects one of those has two equal winners."""
    for _ in range(200):                                                   # a retry happens only when both pinned positions fall into ONE slot pair (below)
        if r:
            slots = []
            for grp in groups:
                p = grp[torch.randperm(len(grp), generator=g)].tolist()
                slots += [(p[i], p[i + 1]) for i in range(0, len(p), 2)]
            reps = [c for c in range(64) if c < _partner(c, r)]
            if single_head:
                reps = [c for c in reps if c % 32 not in (0, r)]
                reps = reps + [reps[int(i)] for i in torch.randperm(len(reps), generator=g)[:2]]
            items = [(c, _partner(c, r)) for c in reps]
        else:
            slots = [(int(p),) for grp in groups for p in grp]
            cs = list(range(64))
            if single_head:
                cs = [c for c in cs if c % 32 != 0]
                cs = cs + [cs[int(i)] for i in torch.randperm(len(cs), generator=g)[:2]]
            items = [(c,) for c in cs]
        assert len(items) == len(slots)
        order = torch.randperm(len(items), generator=g).tolist()
        items = [items[i] if int(torch.randint(2, (1,), generator=g)) else items[i][::-1] for i in order]
        for pos, code in (fixed or {}).items():
            si = next(i for i, s in enumerate(slots) if pos in s)
            ii = next(i for i, it in enumerate(items) if code in it)
            items[si], items[ii] = items[ii], items[si]
            if items[si][slots[si].index(pos)] != code:
                items[si] = items[si][::-1]
        out = torch.full((64,), -1, dtype=torch.long)
        for s, it in zip(slots, items):
            for pos, code in zip(s, it):
                out[pos] = code
        # pinning the second code moves the first one away when both pinned positions share a slot pair (probability 1 / 15 with quadrants): draw again
        if all(int(out[pos]) == code for pos, code in (fixed or {}).items()):
            assert bool((out >= 0).all())
            return out
    raise AssertionError("no placement found")


def block_rows(n, heads, r, shift_regions, seed):
    """(n, 64, C) +-1 patterns in window order: per head a signed Hadamard code placed by ``place_codes`` (a different placement per window and head)"""
    g = gen(seed)
    codes = signed_codes(32)
    groups = _quadrants() if shift_regions else [torch.arange(64)]
    s = torch.zeros(n, 64, heads * 32, dtype=torch.float64)
    idx = torch.zeros(n, heads, 64, dtype=torch.long)
    for w in range(n):
        for h in range(heads):
            fixed = None
            if heads > 1 and h % 2 == 1:                                   # the two unbalanced codes cancel against the neighbouring head
                prev = idx[w, h - 1]
                fixed = {int((prev == 0).nonzero()[0]): 32, int((prev == 32).nonzero()[0]): 0}
            idx[w, h] = place_codes(groups, r[h], heads == 1, g, fixed)
            s[w, :, 32 * h:32 * h + 32] = codes[idx[w, h]]
    assert bool((s.sum(2) == 0).all()), "rows must be balanced"
    return s, idx


def signed_permutation(C, seed):
    g = gen(seed)
    w = torch.zeros(C, C, dtype=torch.float64)
    w[torch.arange(C), torch.randperm(C, generator=g)] = torch.randint(2, (C,), generator=g).double() * 2 - 1
    return w


@functools.lru_cache(maxsize=None)
def block_case(B, H, W, C, shift, kind, use_mod, dtype):
    """One LeWin block on saturated inputs -> every operand (reference parameter names) and every documented intermediate.
    kinds: "onehot" (Wq = 48 diag(h_r), Wk = I: every query selects the key that holds its code times h_r), "self" (r = 0: every query selects itself;
    Wproj Wv = 2 I, so the new rows stay balanced and LN2 is live), "uniform" (Wq = 0, constant table: the shift mask alone decides), "table" (Wq = 0,
    one table entry of 120 per head).  LN2 is live in "self" only; elsewhere its weight is 0 and z = bias."""
    heads, M, hid = C // 32, B * H * W, 4 * C
    n = M // 64
    seed = 500 + C + H + shift + BLOCK_KINDS.index(kind) * 7 + int(use_mod)
    g = gen(seed)
    tok = X.window_tokens(B, H, W, shift)
    attend = kind in ("onehot", "self")
    if attend:
        assert dtype != F32, "f32 keeps xn unrounded: the row patterns do not survive the LayerNorm"
        assert not (use_mod and heads == 1), "a single head has duplicated codes, whose cross terms with a modulator would not tie"
        r = [0] * heads if kind == "self" else [int(v) for v in torch.randint(1, 32, (heads,), generator=g)]
        s_win, code_idx = block_rows(n, heads, r, bool(shift), seed + 1)
        s_win = s_win.reshape(M, C)
        sign = torch.ones(C, dtype=torch.float64) if kind == "self" else pick((-1, 1), (C,), seed + 2)
        gamma1, beta1 = sign, torch.zeros(C, dtype=torch.float64)
        mod = None
        if use_mod:                                                            # one entry of +-2 per (window position, head): xn stays odd, the cross terms stay small
            mod = torch.zeros(64, C, dtype=torch.float64)
            col = torch.randint(32, (64, heads), generator=g) + 32 * torch.arange(heads)
            mod.scatter_(1, col, pick((-2, 2), (64, heads), seed + 3))
        wq, wk = torch.zeros(C, C, dtype=torch.float64), torch.diag(sign)
        for h in range(heads):
            sl = slice(32 * h, 32 * h + 32)
            wq[sl, sl] = Q_GAIN * torch.diag(hadamard(32)[r[h]] * sign[sl])
        bq, bk = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    else:
        assert not (kind == "table" and shift), "a table entry of 120 does not beat the -100 mask by the margin"
        _, s_win = balanced_rows(M, C, seed + 1)
        gamma1, beta1 = ln_params(C, seed + 2, dtype)
        mod = modulator_rows(C, seed + 3) if use_mod else None
        if dtype == F32:                                                       # xn = bias + modulator > 0 and (below) v = one entry of xn: no mean over a mask region is zero
            beta1, mod = beta1.abs(), None if mod is None else mod.abs()
        wq, bq = torch.zeros(C, C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        wk, bk = sparse_pm1(C, C, seed + 4), lattice((C,), PM2, seed + 5)
    amp = pick((1, 2, 4), (M, 1), seed + 6)
    x = torch.zeros(M, C, dtype=torch.float64)
    x[tok] = s_win * amp                                                       # x in token order; s_win, amp, xn in window-row order
    mod_rows = None if mod is None else mod.repeat(n, 1)
    xn = xn_lattice(x[tok], s_win, gamma1, beta1, mod_rows, dtype)
    if kind == "self":
        wv, bv = signed_permutation(C, seed + 7), torch.zeros(C, dtype=torch.float64)
        wp, bp = PROJ_GAIN * wv.t().contiguous(), torch.zeros(C, dtype=torch.float64)
    elif attend:
        wv, bv = sparse_pm1(C, C, seed + 7), pick((-2, 0, 2), (C,), seed + 8)
        wp, bp = sparse_pm1(C, C, seed + 9), lattice((C,), PM2, seed + 10)
    else:                                                                      # means over 16 / 32 / 64 keys must stay T values: v is one entry of xn
        wv, bv = sparse_pm1(C, C, seed + 7, nnz=1), torch.zeros(C, dtype=torch.float64)
        if dtype == F32:
            wv = wv.abs()
        wp, bp = sparse_pm1(C, C, seed + 9), lattice((C,), PM2, seed + 10)
    if kind == "table":
        bias, table = table_bias(heads, seed + 11)
    else:
        table = torch.ones(225, heads, dtype=torch.float64) if kind == "uniform" else (torch.zeros(225, heads, dtype=torch.float64) if (attend and heads == 1) else pick((-2, -1, 0, 1, 2), (225, heads), seed + 11))
        bias = table[X.rpb_index(8)].permute(2, 0, 1).contiguous()
    # ---- q | k | v: exact integers; q is then scaled (one float32 multiply) and rounded to T, which only a saturated softmax sees
    wqkv, bqkv = torch.cat([wq, wk, wv], 0), torch.cat([bq, bk, bv], 0)
    P = xn @ wqkv.t() + bqkv
    assert torch.equal(P.float().double(), P)
    check_representable(P[:, C:], dtype)
    if dtype != F32:
        assert bool((P[:, 2 * C:].abs() % 2 == 1).all()), "v must be odd"
    heads_of = lambda t: t.reshape(n, 64, heads, 32).permute(0, 2, 1, 3)      # noqa: E731  (M, C) -> (n, heads, 64, 32)
    q2 = heads_of((P[:, :C].float() * QSCALE32).to(dtype).double())
    q_plain = (P[:, :C].float() * QSCALE_PLAIN32).to(dtype)                    # the side store of the training form
    k, v = heads_of(P[:, C:2 * C]), heads_of(P[:, 2 * C:])
    mask = shift_mask64(H, W, shift)
    s2 = q2 @ k.transpose(2, 3) + (bias.float() * LOG2E32).double()[None] + torch.where(mask < 0, MASK2, 0.0)[torch.arange(n) % mask.shape[0]][:, None]
    e = torch.exp2(s2 - s2.max(3, keepdim=True).values)
    eT = e.to(dtype).double()
    o_doc = (eT @ v) / e.sum(3, keepdim=True)
    # conditions: saturated softmax
    top = s2.max(3, keepdim=True).values
    winners = eT == 1.0
    n_win = winners.sum(3)
    assert bool(((eT == 1.0) | (eT < 1e-40)).all()) and (dtype == F32 or bool(((eT == 1.0) | (eT == 0.0)).all()))
    assert torch.equal(e.sum(3).float().double(), n_win.double())
    # every unmasked key that loses is LEAD2 behind; a masked one (-144 in the log2 domain: a float32 subnormal e) is covered by the line above and by v != 0
    masked = (mask < 0)[torch.arange(n) % mask.shape[0]][:, None].expand_as(s2)
    lead = (top - torch.where(winners | masked, torch.full_like(s2, -1e9), s2).max(3, keepdim=True).values)[..., 0]
    assert bool((lead >= LEAD2).all()), float(lead.min())
    o_exact = (winners.double() @ v) / n_win[..., None]
    assert torch.equal(o_doc.to(dtype).double(), o_exact), "the documented softmax does not round to the lattice value"
    assert torch.equal(o_exact.to(dtype).double(), o_exact)                     # representable: the store of o rounds nothing
    if dtype == F32 and shift:
        assert bool((o_exact != 0).all()), "a zero mean: what the masked keys' subnormals add would decide it"
    if attend:
        allowed = {1, 2} if heads == 1 else {1}
        assert set(n_win.unique().tolist()) <= allowed and 1 in n_win.unique().tolist()
        if kind == "self":
            assert bool(winners.diagonal(dim1=2, dim2=3).all())
        else:
            assert not bool(winners.diagonal(dim1=2, dim2=3).any())
    elif kind == "uniform":
        assert set(n_win.unique().tolist()) == ({64} if not shift else ({16, 32, 64} if H > 8 and W > 8 else {16, 32}))
    else:
        assert {1, 64} <= set(n_win.unique().tolist())
    o = o_exact.permute(0, 2, 1, 3).reshape(M, C)                              # window-row order, heads merged
    y = o @ wp.t() + bp
    check_accumulation(C, (int(xn.abs().max()),), (Q_GAIN,), addend_steps=4)
    # ---- LN2 -> linear1 (-> GELU): x1 is balanced in "self" only
    if kind == "self":
        gamma2, beta2 = pick((-1, 1), (C,), seed + 12), torch.zeros(C, dtype=torch.float64)
    else:
        gamma2, beta2 = torch.zeros(C, dtype=torch.float64), pick((-1, 1), (C,), seed + 12)
    w1 = sparse_pm1(hid, C, seed + 13, nnz=1)
    up1 = torch.randint(2, (hid,), generator=g).bool()
    b1 = torch.where(up1, 9.0, -16.0).double()
    taps = torch.tensor(BLOCK_TAPS, dtype=torch.float64)[torch.rand(hid, 9, generator=g).argsort(1)]
    up2 = torch.randint(2, (hid,), generator=g).bool()
    bdw = torch.where(up2, POS_MIN + 100.0, NEG_MAX - 100.0).double() + torch.randint(3, (hid,), generator=g).double() * torch.where(up2, 1.0, -1.0)
    w2, b2 = lattice((C, hid), PM1, seed + 14), lattice((C,), PM2, seed + 15)
    c = {"tok": tok, "x": x, "xn": xn, "gamma1": gamma1, "beta1": beta1, "mod": mod, "wq": wq, "wk": wk, "wv": wv, "bq": bq, "bk": bk, "bv": bv, "table": table,
         "wp": wp, "bp": bp, "gamma2": gamma2, "beta2": beta2, "w1": w1, "b1": b1, "taps": taps, "bdw": bdw, "w2": w2, "b2": b2,
         "P": P, "q_plain": q_plain, "o": o, "y": y, "n_win": n_win, "lead": lead, "bias": bias, "heads": heads}
    return c


def block_attn_out(c, B, drop=None):
    """rows after the attention half, token order: x[tok] + drop[image] * y[row]"""
    M = c["x"].shape[0]
    d = torch.ones(B, dtype=torch.float64) if drop is None else torch.tensor(drop, dtype=torch.float64)
    out = c["x"].clone()
    out[c["tok"]] += d[c["tok"] // (M // B)][:, None] * c["y"]
    return out


def block_ffn_half(c, x1, B, H, W, dtype, drop=None):
    """the LeFF half on the rows x1 (token order, float64): -> (z, a1, h1, out), z = LN2 rounded to T, a1 = linear1 pre-activation, h1 = GELU(a1) as T"""
    M, C = x1.shape
    hid = 4 * C
    if bool((c["gamma2"] != 0).any()):
        a = x1.abs().max(1, keepdim=True).values
        z = xn_lattice(x1, x1 / a, c["gamma2"], c["beta2"], None, dtype)
    else:
        z = c["beta2"].expand(M, C).clone()
        assert torch.equal(ln_doc64(x1, c["gamma2"], c["beta2"]), z)
    a1 = z @ c["w1"].t() + c["b1"]
    check_saturated(a1)
    h1 = gelu_saturated(a1, dtype)
    pre = F.conv2d(h1.double().reshape(B, H, W, hid).permute(0, 3, 1, 2), c["taps"].reshape(hid, 1, 3, 3), c["bdw"], padding=1, groups=hid).permute(0, 2, 3, 1)
    check_saturated(pre)
    g2 = gelu_saturated(pre, dtype)
    check_accumulation(hid, (int(pre.abs().max()),), PM1, addend_steps=64)
    d = torch.ones(B, dtype=torch.float64) if drop is None else torch.tensor(drop, dtype=torch.float64)
    out = x1 + d.repeat_interleave(M // B)[:, None] * (g2.double().reshape(M, hid) @ c["w2"].t() + c["b2"])
    return z, a1, h1, out


def block_state_dict(c, C):
    """the block's parameters under the reference's names (float64; the caller casts and moves them)"""
    hid = 4 * C
    sd = {"norm1.weight": c["gamma1"], "norm1.bias": c["beta1"], "attn.qkv.to_q.weight": c["wq"], "attn.qkv.to_q.bias": c["bq"],
          "attn.qkv.to_kv.weight": torch.cat([c["wk"], c["wv"]], 0), "attn.qkv.to_kv.bias": torch.cat([c["bk"], c["bv"]], 0),
          "attn.relative_position_bias_table": c["table"], "attn.proj.weight": c["wp"], "attn.proj.bias": c["bp"],
          "norm2.weight": c["gamma2"], "norm2.bias": c["beta2"], "mlp.linear1.0.weight": c["w1"], "mlp.linear1.0.bias": c["b1"],
          "mlp.dwconv.0.weight": c["taps"].reshape(hid, 1, 3, 3), "mlp.dwconv.0.bias": c["bdw"], "mlp.linear2.0.weight": c["w2"], "mlp.linear2.0.bias": c["b2"]}
    if c["mod"] is not None:
        sd["modulator.weight"] = c["mod"]
    return sd


# (B, H, W, C, shift, kind, modulator).  Forms of the fused kernel (launch_attn_block in csrc/uf_attnblk.hip): "attn=0 / 1 / 2" at C <= 128, "attn=4 / 5" at C <= 64,
# "attn=3" at C = 256 with more than 256 windows, and C = 256 switches from 8 to 4 waves above 256 windows (5 maps of 64 x 64 = 320 windows).
# 8 x 24 with B = 3 is 9 windows; 16 x 16 has every mask region
def block_cases(dtype):
    cases = []
    for C in (32, 64, 128, 256, 512):
        if dtype == F32 and C > 256:
            continue
        single = C == 32
        for shift in (0, 4):
            if dtype != F32:
                cases.append((1, 16, 16, C, shift, "onehot", (not single) and shift == 4))
                cases.append((3, 8, 24, C, 4 - shift, "self", False))
        cases.append((1, 16, 16, C, 0, "table", True))
        cases.append((3, 8, 24, C, 0, "table", False))
        cases.append((1, 16, 16, C, 4, "uniform", True))
        cases.append((3, 8, 24, C, 4, "uniform", False))
    if dtype != F32:                                                           # f32 has one launch shape at C = 256
        cases.append((5, 64, 64, 256, 4, "onehot", True))
    return cases


def block_variants(C, n_windows, dtype):
    if dtype == F32:
        return [None]
    v = [None]
    if C <= 128:
        v += ["attn=0", "attn=1", "attn=2"]
    if C <= 64:
        v += ["attn=4", "attn=5"]
    if C == 256 and n_windows > 256:
        v += ["attn=3"]
    return v


def block_attn_eval(c, B, H, W, shift, dtype, gather_shift=None, scatter_shift=None, mod_roll=0, bias=None, use_mask=True, swap_heads=False):
    """the attention half of ``block_case`` evaluated again in float64 with the documented roundings and, optionally, one fault (stand-ins of
    tests/test_saturated_reference.py): rows gathered / scattered with another roll, the modulator row of another window position, another bias, the
    shift mask ignored, two heads' channels swapped in the merged output.  No saturation condition is asserted here: a fault may break them."""
    M, C = c["x"].shape
    heads, n = C // 32, M // 64
    tok_g = X.window_tokens(B, H, W, shift if gather_shift is None else gather_shift)
    tok_s = X.window_tokens(B, H, W, shift if scatter_shift is None else scatter_shift)
    xn = ln_doc64(c["x"][tok_g], c["gamma1"], c["beta1"])
    if c["mod"] is not None:
        xn = xn + c["mod"].roll(mod_roll, 0).repeat(n, 1)
    xn = xn.to(dtype).double()
    P = xn @ torch.cat([c["wq"], c["wk"], c["wv"]], 0).t() + torch.cat([c["bq"], c["bk"], c["bv"]], 0)
    heads_of = lambda t: t.reshape(n, 64, heads, 32).permute(0, 2, 1, 3)      # noqa: E731
    q2 = heads_of((P[:, :C].float() * QSCALE32).to(dtype).double())
    k, v = heads_of(P[:, C:2 * C].to(dtype).double()), heads_of(P[:, 2 * C:].to(dtype).double())
    mask = shift_mask64(H, W, shift if use_mask else 0)
    b = c["bias"] if bias is None else bias
    s2 = q2 @ k.transpose(2, 3) + (b.float() * LOG2E32).double()[None] + torch.where(mask < 0, MASK2, 0.0)[torch.arange(n) % mask.shape[0]][:, None]
    e = torch.exp2(s2 - s2.max(3, keepdim=True).values)
    o = ((e.to(dtype).double() @ v) / e.sum(3, keepdim=True)).to(dtype).double()
    if swap_heads:
        o = o.flip(1)
    y = o.permute(0, 2, 1, 3).reshape(M, C) @ c["wp"].t() + c["bp"]
    out = c["x"].clone()
    out[tok_s] += y
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# 4 x 4-window attention core (uf_window4_attention_fwd): raster rows q | k | v, the kernel applies head_dim^-0.5, P stays float32
# ---------------------------------------------------------------------------------------------------------------------------
# (B, H, W, heads, head_dim, kind): one head, a head count that fills one workgroup's head group and one that does not divide into groups; 4 x 12 with B = 3 is 9 windows
ATTN4_CASES = [(B, H, W, heads, hd, kind) for kind in KINDS for (B, H, W, heads, hd) in ((1, 8, 8, 2, 16), (3, 4, 12, 1, 32), (1, 8, 8, 5, 32), (2, 8, 4, 8, 16))]
Q_GAIN4 = 32                                             # a match scores 32 a sqrt(head_dim) >= 128


def window4_rows(B, H, W):
    """(n_windows, 16) raster row of token t = 4 y + x of window w (image-major, then row-major over the windows)"""
    return torch.arange(B * H * W).reshape(B, H // 4, 4, W // 4, 4).permute(0, 1, 3, 2, 4).reshape(-1, 16)


def rpb4_dense(tab):
    """(heads, 49) table -> (heads, 16, 16): entry (yq - yk + 3) * 7 + (xq - xk + 3)"""
    t = torch.arange(16)
    ent = ((t[:, None] // 4) - (t[None, :] // 4) + 3) * 7 + ((t[:, None] % 4) - (t[None, :] % 4) + 3)
    return tab[:, ent]


@functools.lru_cache(maxsize=None)
def attn4_case(B, H, W, heads, hd, kind, dtype):
    n, C = B * (H // 4) * (W // 4), heads * hd
    g = gen(700 + hd + heads + H + KINDS.index(kind))
    codes = signed_codes(hd)
    scale = float(torch.tensor(1.0 / math.sqrt(hd), dtype=F32))
    v = pick(V_VALUES, (n, heads, 16, hd), 710 + hd + heads) * pick((-1, 1), (n, heads, 1, hd), 711 + hd + heads)
    q = torch.zeros(n, heads, 16, hd, dtype=torch.float64)
    k = torch.zeros_like(q)
    target = torch.full((n, heads, 16), -1, dtype=torch.long)
    for w_ in range(n):
        for h in range(heads):
            tcode = torch.randperm(2 * hd, generator=g)[:16]                   # 16 tokens, 32 or 64 signed codes: every token its own
            amp = torch.tensor((1.0, 2.0, 4.0), dtype=torch.float64)[torch.randint(3, (16,), generator=g)]
            k[w_, h] = codes[tcode] * amp[:, None]
            if kind == "onehot":
                p = torch.randperm(16, generator=g)
                pi = torch.empty(16, dtype=torch.long)
                pi[p[0::2]], pi[p[1::2]] = p[1::2], p[0::2]
                q[w_, h] = Q_GAIN4 * codes[tcode[pi]]
                target[w_, h] = pi
    tab = torch.zeros(heads, 49, dtype=torch.float64)
    if kind == "onehot":
        tab = pick((-2, -1, 0, 1, 2), (heads, 49), 720 + heads)
    elif kind == "uniform":
        tab += 3.0
    else:                                                                      # one entry of 120 per head, at an offset of its own, never (0, 0)
        offs = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3) if (dy, dx) != (0, 0)]
        for h, i in enumerate(torch.randperm(len(offs), generator=g)[:heads].tolist()):
            tab[h, (offs[i][0] + 3) * 7 + offs[i][1] + 3] = 120.0
    bias = rpb4_dense(tab)
    s, eT, esum, o = attn_doc64(q * scale, k, v.transpose(2, 3), bias, torch.zeros(1, 16, 16, dtype=torch.float64), F32)
    e64 = eT.double()
    winners = e64 == 1.0
    n_win = winners.sum(3)
    assert bool(((e64 == 1.0) | (e64 == 0.0)).all()), "an unsaturated probability"
    lead = (s.max(3, keepdim=True).values - torch.where(winners, torch.full_like(s, -1e9), s).max(3, keepdim=True).values)[..., 0]
    assert bool(((lead >= MARGIN + 4) | (n_win == 16)).all()), float(lead.min())
    exact = (winners.double() @ v / n_win[..., None]).permute(0, 2, 1, 3).reshape(n, 16, C)
    assert torch.equal(o.reshape(n, 16, C).to(dtype).double(), exact) and torch.equal(exact.to(dtype).double(), exact)
    check_accumulation(hd, (Q_GAIN4,), (4,), addend_steps=3)
    want = {"onehot": {1}, "uniform": {16}}.get(kind)
    got = set(n_win.unique().tolist())
    assert got == want if want else {1, 16} <= got
    if kind == "onehot":
        assert bool(winners.gather(3, target[..., None]).all())
    rows = window4_rows(B, H, W)
    merge = lambda t: t.permute(0, 2, 1, 3).reshape(n, 16, C)                 # noqa: E731
    qkv = torch.zeros(B * H * W, 3 * C, dtype=torch.float64)
    qkv[rows.reshape(-1)] = torch.cat([merge(q), merge(k), merge(v)], 2).reshape(n * 16, 3 * C)
    out = torch.zeros(B * H * W, C, dtype=torch.float64)
    out[rows.reshape(-1)] = exact.reshape(n * 16, C)
    return {"qkv": qkv, "tab": tab, "bias": bias, "o": out, "q": q, "k": k, "v": v, "scale": scale, "n_win": n_win, "C": C}
