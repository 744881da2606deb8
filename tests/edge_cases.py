"""Helpers of the edge tests (tests/test_gpu_edges.py, tests/test_edges_reference.py).  Not a conftest: plain functions.

Part A: ``PoisonedView`` -- a live (rows, C) view inside a larger allocation whose every other element holds one NaN bit pattern,
so that a kernel reading outside its view produces NaN and a kernel writing outside it destroys a pattern that can be found again.

Part B: input generators for the hard classes, float64 references, and emulations = the same formulas in the kernels' arithmetic
(float32 statistics and accumulation, rounding to the operand type T at the points oracle/bf16_budget.py names).  The emulation is
CPU code and never the kernel; the GPU gate is ``kernel worst row <= 4 x emulation worst row`` (floor: 2 ulp of the output type).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Tuple

import torch

from oracle.bf16_budget import Budget

Tensor = torch.Tensor
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TAG = {F32: "f32", BF16: "bf16", F16: "f16"}

# ---------------------------------------------------------------------------------------------------------------------------
# Part A: poisoned memory
# ---------------------------------------------------------------------------------------------------------------------------
POISON = {4: 0x7FC0BEEF, 2: 0x7FCB}          # quiet NaN with a known payload, as f32 and as bf16 / f16
INT = {4: torch.int32, 2: torch.int16}
GUARD_ROWS = 8


class PoisonedView:
    """(rows + G) x ld elements of ``dtype``; ``view`` = rows [G/2, G/2 + rows), columns [col, col + C).  Modes:
         plain    ld = C, no guard rows: the contiguous call every strided call is compared with
         guard    ld = C with guard rows (operands whose entry point takes no leading dimension)
         strided  ld = C + 16, col = 8
         cat      ld = 2C, col = C: the right half of a concat buffer, as the encoder runs (cat_left: col = 0, the Upsample half)
    ld and col are multiples of 8 elements whenever C is: 16-byte aligned pointers for 2- and 4-byte types."""

    def __init__(self, rows: int, C: int, dtype=F32, mode: str = "strided", device="cpu", ld: Optional[int] = None, col: Optional[int] = None):
        G = 0 if mode == "plain" else GUARD_ROWS
        dld, dcol = {"plain": (C, 0), "guard": (C, 0), "strided": (C + 16, 8), "cat": (2 * C, C), "cat_left": (2 * C, 0)}[mode]
        self.ld, self.col = (dld if ld is None else ld), (dcol if col is None else col)
        assert self.ld >= self.col + C
        self.rows, self.C, self.G, self.dtype = rows, C, G, dtype
        self.size = torch.empty(0, dtype=dtype).element_size()
        self.pattern = POISON[self.size]
        self.bits = torch.full((rows + G, self.ld), self.pattern, dtype=INT[self.size], device=device)
        self.buf = self.bits.view(dtype)
        self.view = self.buf[G // 2:G // 2 + rows, self.col:self.col + C]

    def fill(self, src: Tensor) -> "PoisonedView":
        self.view.copy_(src.reshape(self.rows, self.C).to(self.dtype))
        return self

    def ptr(self) -> int:
        return self.view.data_ptr()

    def live_bits(self) -> Tensor:
        return self.bits[self.G // 2:self.G // 2 + self.rows, self.col:self.col + self.C].clone()

    def live(self) -> Tensor:
        return self.view.clone()

    def guard_intact(self) -> bool:
        outside = torch.ones_like(self.bits, dtype=torch.bool)
        outside[self.G // 2:self.G // 2 + self.rows, self.col:self.col + self.C] = False
        return bool((self.bits[outside] == self.pattern).all())


def poisoned_bytes(nbytes: int, guard: int, fill: int, device) -> Tuple[Tensor, Tensor]:
    """A workspace of ``nbytes`` filled with the byte ``fill`` + ``guard`` bytes of 0xA5 behind it: (whole buffer, guard slice)."""
    buf = torch.full((nbytes + guard,), fill, dtype=torch.uint8, device=device)
    buf[nbytes:] = 0xA5
    return buf, buf[nbytes:]


# ---------------------------------------------------------------------------------------------------------------------------
# Part B: metric and gate
# ---------------------------------------------------------------------------------------------------------------------------
MARGIN = 4.0


def unit(dtype) -> float:
    """rounding unit (half an ulp of 1) of a type"""
    return torch.finfo(dtype).eps / 2


def row_err(got: Tensor, exact: Tensor) -> Tensor:
    """per row: max|got - exact| / max(|exact| over the row, tiny); non-finite results count as infinite error"""
    got, exact = got.double().reshape(-1, got.shape[-1]), exact.double().reshape(-1, exact.shape[-1])
    d = (got - exact).abs()
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, float("inf")))
    return d.amax(-1) / exact.abs().amax(-1).clamp_min(1e-30)


def gate(emu_worst: float, out_dtype) -> float:
    return max(MARGIN * emu_worst, 2 * torch.finfo(out_dtype).eps)


def rnd(dtype) -> Callable[[Tensor], Tensor]:
    return (lambda x: x) if dtype == F32 else (lambda x: x.to(dtype).float())


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm rows
# ---------------------------------------------------------------------------------------------------------------------------
LN_ROWS = 128
LN_CS = (16, 32, 64, 256, 512)
LN_CLASSES = ("mean1e3_std1", "mean100_std1e-2", "constant", "outlier1e4", "tiny1e-6")


def ln_rows(cls: str, C: int, rows: int = LN_ROWS) -> Tensor:
    g = torch.Generator().manual_seed(1000 + C + LN_CLASSES.index(cls))
    z = torch.randn(rows, C, generator=g, dtype=torch.float64)
    if cls == "mean1e3_std1":
        x = 1e3 + z
    elif cls == "mean100_std1e-2":
        x = 100 + 1e-2 * z
    elif cls == "constant":
        x = (3 * z[:, :1]).expand(rows, C)
    elif cls == "outlier1e4":
        x = z.clone()
        x[torch.arange(rows), torch.arange(rows) * 7 % C] = 1e4
    elif cls == "tiny1e-6":
        x = 1e-6 * z
    else:
        raise KeyError(cls)
    return x.float().contiguous()


def ln_affine(C: int) -> Tuple[Tensor, Tensor]:
    g = torch.Generator().manual_seed(77 + C)
    return (1 + 0.1 * torch.randn(C, generator=g)).float(), (0.1 * torch.randn(C, generator=g)).float()


def ln_condition(x: Tensor) -> float:
    """amplification of a relative perturbation of the inputs: max|x| / sqrt(var + eps), worst row"""
    xd = x.double()
    return float((xd.abs().amax(-1) / (xd.var(-1, unbiased=False) + 1e-5).sqrt()).max())


def ln_ref(x: Tensor, gamma: Tensor, beta: Tensor) -> Tensor:
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / (var + 1e-5).sqrt() * gamma + beta


def tree_sum(x: Tensor) -> Tensor:
    """row sums by halving, the order of the kernels' xor-shuffle reductions (C a power of two): adding equal halves is exact, so a
    constant row has an exact mean and a zero centred row, as on the GPU -- a flat left-to-right float32 sum does not"""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x


def ln_emu(x: Tensor, gamma: Tensor, beta: Tensor, dtype, switches=("xn",)) -> Tensor:
    """two-pass float32 statistics (mean, then centred variance), float32 affine, result rounded to T (switch ``xn`` / ``z``).
    ``dtype`` None: everything in float64 with no rounding (all switches off)."""
    if dtype is None:
        return ln_ref(x, gamma, beta)
    x, gamma, beta = x.float(), gamma.float(), beta.float()
    C = x.shape[-1]
    mu = tree_sum(x) * (1.0 / C)
    v = x - mu
    rstd = 1.0 / torch.sqrt(tree_sum(v * v) * (1.0 / C) + 1e-5)
    y = v * rstd * gamma + beta
    return y if dtype == F32 else Budget(switches, TAG[dtype]).r("xn", y)


def ln_bwd_ref(x: Tensor, gamma: Tensor, dy: Tensor, dt=torch.float64):
    """closed form of nn.LayerNorm's backward in ``dt``: (dx, dgamma, dbeta)"""
    x, gamma, dy = x.to(dt), gamma.to(dt), dy.to(dt)
    C = x.shape[-1]
    mu = tree_sum(x) * (1.0 / C)
    v = x - mu
    rstd = 1.0 / torch.sqrt(tree_sum(v * v) * (1.0 / C) + 1e-5)
    xh = v * rstd
    gdy = dy * gamma
    dx = (gdy - gdy.mean(-1, keepdim=True) - xh * (gdy * xh).mean(-1, keepdim=True)) * rstd
    return dx, (dy * xh).sum(0), dy.sum(0)


def linear_ref(a: Tensor, w: Tensor, b: Tensor) -> Tensor:
    return a.double() @ w.double().t() + b.double()


def linear_emu(a: Tensor, w: Tensor, b: Tensor) -> Tensor:
    """T operands (already rounded), exact products, float32 accumulation"""
    return a.float() @ w.float().t() + b.float()


def gemm_weights(N: int, K: int, dtype, seed: int) -> Tuple[Tensor, Tensor]:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype), 0.1 * torch.randn(N, generator=g)


# ---------------------------------------------------------------------------------------------------------------------------
# GELU family
# ---------------------------------------------------------------------------------------------------------------------------
GELU_A, GELU_B = -2.3022081985, -0.10294324           # uf_common.h gelu_bf2
GELU_CLASSES = ("wide40", "core4")
GELU_ROW = 64


def gelu_grid(cls: str, dtype) -> Tensor:
    """pre-activations snapped to T, (rows, 64) with every row spanning the whole range (row r holds grid points r, r + R, ...):
    wide40 = [-40, 40] plus +-0, the two neighbours of -8.4 (gelu_and_grad_t changes form there) and +-65504 (largest finite f16);
    core4 = [-4, 4], where GELU is not yet x or 0."""
    R = 64
    lim = {"wide40": 40.0, "core4": 4.0}[cls]
    pts = torch.linspace(-lim, lim, R * GELU_ROW - 8, dtype=torch.float64)
    extra = [0.0, -0.0, 0.0, -0.0] if cls == "core4" else [0.0, -0.0, 65504.0, -65504.0]
    extra += [-8.4, -8.4, -8.4, -8.4]
    x = torch.cat([pts, torch.tensor(extra, dtype=torch.float64)]).float()
    if dtype != F32:
        x = x.to(dtype).float()
    x = x.reshape(GELU_ROW, R).t().contiguous()
    step = torch.finfo(dtype).eps * 8.0           # one ulp of T at 8.4: the neighbours of -8.4 on either side
    x[R - 1, GELU_ROW - 1] = float(torch.tensor(-8.4 - step).to(dtype))
    x[R - 2, GELU_ROW - 1] = float(torch.tensor(-8.4 + step).to(dtype))
    return x


def gelu_ref(x: Tensor, dtype) -> Tensor:
    """float64: erf form for f32 operands, the documented sigmoid form x / (1 + 2^(x (A + B x^2))) for bf16 / f16"""
    x = x.double()
    if dtype == F32:
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))
    return x * torch.sigmoid(-math.log(2.0) * x * (GELU_A + GELU_B * x * x))


def gelu_grad_ref(x: Tensor, dtype) -> Tensor:
    x = x.double()
    if dtype == F32:
        return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    u = x * (GELU_A + GELU_B * x * x)
    s = torch.sigmoid(-math.log(2.0) * u)
    du = GELU_A + 3 * GELU_B * x * x
    return s - x * s * (1 - s) * math.log(2.0) * du       # d/dx [x s(u)], s = 1 / (1 + 2^u)


def gelu_emu(x: Tensor, dtype) -> Tensor:
    """the kernels' arithmetic: float32 throughout, result rounded to T.  None: float64, no rounding."""
    if dtype is None:
        return gelu_ref(x, BF16)
    x = x.float()
    if dtype == F32:
        return 0.5 * x * (1 + torch.erf(x * 0.70710678118654752440))
    u = x * (x * x * GELU_B + GELU_A)
    return rnd(dtype)(x * (1.0 / (torch.exp2(u) + 1.0)))


def gelu_grad_emu(x: Tensor, dy: Tensor, dtype) -> Tensor:
    if dtype is None:
        return dy.double() * gelu_grad_ref(x, BF16)
    x, dy = x.float(), dy.float()
    if dtype == F32:
        return dy * (0.5 * (1 + torch.erf(x * 0.70710678118654752440)) + x * torch.exp(-0.5 * x * x) * 0.39894228040143267794)
    u = torch.clamp(x * (x * x * GELU_B + GELU_A), max=80.0)
    e = torch.exp2(u)
    sg = 1.0 / (e + 1.0)
    return rnd(dtype)(dy * (sg + x * e * sg * sg * (1.5957691216 + 0.2140610 * x * x)))


# ---------------------------------------------------------------------------------------------------------------------------
# attention core: 2x2 windows of a 16x16 map
# ---------------------------------------------------------------------------------------------------------------------------
ATT_CLASSES = ("one_hot", "uniform", "bias30", "shift_user_mask", "masked_keys_win")
ATT_H = ATT_W = 16
ATT_NW = 4


def shift_mask(H: int, W: int, shift: int) -> Tensor:
    """SW-MSA mask (nW, 64, 64) in {0, -100} (reference model.py:924-942), float64"""
    img = torch.zeros(H, W)
    cnt = 0
    for hs in (slice(0, -8), slice(-8, -shift), slice(-shift, None)):
        for ws in (slice(0, -8), slice(-8, -shift), slice(-shift, None)):
            img[hs, ws] = cnt
            cnt += 1
    mw = img.reshape(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64)
    d = mw[:, None, :] - mw[:, :, None]
    return torch.where(d != 0, -100.0, 0.0).double()


def attention_case(cls: str, heads: int, hd: int, dtype) -> Dict[str, object]:
    """q (scaled), k (nW, heads, 64, hd), vt (nW, heads, hd, 64) already of type T; bias f32 (heads, 64, 64); user mask f32
    (nW, 64, 64) or None; shift.  |q|, |k| <= 64."""
    g = torch.Generator().manual_seed(500 + 10 * heads + hd + ATT_CLASSES.index(cls))
    nW = ATT_NW
    rn = lambda *s: torch.randn(*s, generator=g)                                # noqa: E731
    q, k, v = rn(nW, heads, 64, hd), rn(nW, heads, 64, hd), rn(nW, heads, 64, hd)
    bias = rn(heads, 64, 64)
    mask, shift = None, 0
    u = torch.ones(hd) / hd ** 0.5
    if cls == "one_hot":
        c = 40 + 20 * torch.rand(nW, heads, 64, 1, generator=g)
        a = 0.75 * torch.arange(64.0)[torch.randperm(64, generator=g)].reshape(1, 1, 64, 1)
        q, k = c * u + 0.01 * q, a * u + 0.01 * k
    elif cls == "uniform":
        q = torch.zeros_like(q)
        bias = torch.full_like(bias, 0.375)
    elif cls == "bias30":
        bias = 30.0 * torch.where(bias > 0, 1.0, -1.0)
    elif cls == "shift_user_mask":
        shift = 4
        m = (torch.rand(nW, 64, generator=g) < 0.4).float()
        m[:, 0] = 0
        mask = torch.where(m[:, :, None] * m[:, None, :] != 0, -100.0, 0.0)
    elif cls == "masked_keys_win":
        sel = (torch.arange(64) % 2 == 1).float()                                # odd keys masked by the user mask, and 160 above the rest
        q, k = 16 * u + 0.01 * q, (10 * sel).reshape(1, 1, 64, 1) * u + 0.01 * k
        bias = 0.1 * bias
        mask = (-100.0 * sel).reshape(1, 1, 64).expand(nW, 64, 64).contiguous()
    else:
        raise KeyError(cls)
    return {"q": q.to(dtype), "k": k.to(dtype), "vt": v.transpose(-1, -2).contiguous().to(dtype), "bias": bias.float().contiguous(),
            "mask": None if mask is None else mask.float().contiguous(), "shift": shift, "heads": heads, "hd": hd}


def attention_logits(case, dt=torch.float64) -> Tensor:
    """(nW, heads, 64, 64): q k^T + bias + shift mask + user mask, all added as the reference adds them"""
    q, k = case["q"].to(dt), case["k"].to(dt)
    s = q @ k.transpose(-1, -2) + case["bias"].to(dt).unsqueeze(0)
    if case["shift"]:
        s = s + shift_mask(ATT_H, ATT_W, case["shift"]).to(dt).unsqueeze(1)
    if case["mask"] is not None:
        s = s + case["mask"].to(dt).unsqueeze(1)
    return s


def attention_ref(case) -> Tensor:
    """float64 softmax(logits) v -> (nW * 64, heads * hd), heads merged"""
    p = torch.softmax(attention_logits(case), -1)
    o = p @ case["vt"].double().transpose(-1, -2)
    return o.transpose(1, 2).reshape(ATT_NW * 64, -1)


def attention_emu(case, dtype) -> Tensor:
    """float32 logits, max and sum; the UNNORMALISED probabilities rounded to T (``p``); 1/sum applied to the float32 product; the
    result rounded to T (``o``).  None: float64, no rounding."""
    if dtype is None:
        s = attention_logits(case)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = (e @ case["vt"].double().transpose(-1, -2)) / e.sum(-1, keepdim=True)
        return o.transpose(1, 2).reshape(ATT_NW * 64, -1)
    b = Budget(("p", "o") if dtype != F32 else (), TAG.get(dtype, "bf16") if dtype != F32 else "bf16")
    s = attention_logits(case, torch.float32)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    o = (b.r("p", e) @ case["vt"].float().transpose(-1, -2)) / e.sum(-1, keepdim=True)
    return b.r("o", o.transpose(1, 2).reshape(ATT_NW * 64, -1))


def attention_condition(case) -> float:
    """an absolute logit error d moves a probability by a factor e^d; float32 logits carry eps32 * max|logit|"""
    return 1.0 + float(attention_logits(case).abs().max())


def attention_bwd(case, do: Tensor, dtype, dt=None):
    """(dq, dk, dv, dbias) of the attention core from dO (nW*64, heads*hd): dq wrt the scaled q as stored, dv (nW, heads, 64, hd),
    dbias (heads, 64, 64) summed over windows.  ``dtype`` None: float64, no rounding (the reference).  Else the kernels' arithmetic:
    float32 logits, softmax, dP and dS; the NORMALISED P and dS rounded to T as operands of the three output products (they are chained
    into MFMA operands, uf_bwd.hip window_attn_bwd2_kernel); dbias from the float32 dS; dq, dk, dv rounded to T."""
    dt = dt or (torch.float64 if dtype is None else torch.float32)      # dt = float64 with a dtype: the emulation's path, switches off
    r = (lambda x: x) if dtype in (None, F32) else rnd(dtype)
    nW, heads, hd = ATT_NW, case["heads"], case["hd"]
    q, k, v = case["q"].to(dt), case["k"].to(dt), case["vt"].to(dt).transpose(-1, -2)
    do = do.to(dt).reshape(nW, 64, heads, hd).permute(0, 2, 1, 3)
    s = attention_logits(case, dt)
    dp = do @ v.transpose(-1, -2)
    if dtype is None:
        p = torch.softmax(s, -1)
        dot = (p * dp).sum(-1, keepdim=True)
    else:       # exp as 2^(x log2 e) in float32, P = e * (1 / sum), and the row sums in the kernel's order (lane_sum)
        e = torch.exp2((s - s.amax(-1, keepdim=True)) * torch.tensor(math.log2(math.e), dtype=dt))
        first = dtype == F32 or hd == 64
        p = e * (1.0 / lane_sum(e, first))
        dot = lane_sum(p * dp, first)
    ds = p * (dp - dot)
    dsr, pr = r(ds), r(p)
    return r(dsr @ k), r(dsr.transpose(-1, -2) @ q), r(pr.transpose(-1, -2) @ do), ds.sum(0)


def lane_sum(x: Tensor, first: bool) -> Tensor:
    """sum over the 64 keys of a query row in the kernels' order.  window_attn_bwd2_kernel (2-byte types, head_dim 16 / 32): key
    16 t + 4 g + r lives in lane group g, which adds its 16 values one after the other (t outer, r inner); the four groups are then
    combined pairwise (xor 16, xor 32).  window_attn_bwd_kernel (``first``: f32, and head_dim 64): key 16 t + l lives in lane l, which
    adds its 4 values in t order; the 16 lanes are combined as a tree of neighbours (DPP quad_perm, half mirror, mirror).
    The row's dot = sum(P dP) is ONE float32 value that every dS of the row inherits, so on rows whose dS cancels to nearly nothing the
    order of this sum decides the error -- an emulation with another order draws another sample of it, not a smaller error."""
    lead = x.shape[:-1]
    if first:
        x = x.reshape(*lead, 4, 16)
        acc = ((x[..., 0, :] + x[..., 1, :]) + x[..., 2, :]) + x[..., 3, :]
        while acc.shape[-1] > 1:
            acc = acc[..., 0::2] + acc[..., 1::2]
        return acc
    x = x.reshape(*lead, 4, 4, 4).transpose(-3, -2).reshape(*lead, 4, 16)       # (..., g, 16 values in (t, r) order)
    acc = x[..., 0]
    for i in range(1, 16):
        acc = acc + x[..., i]
    return ((acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])).unsqueeze(-1)


# 4x4 windows (the bottleneck of a model built for 64x64 patches): raster q|k|v rows of an 8x8 map, no masks
ATT4_CLASSES = ("one_hot", "uniform", "bias30")
ATT4_H = ATT4_W = 8


def attention4_case(cls: str, heads: int, hd: int, dtype) -> Dict[str, object]:
    """qkv T (H*W, 3C) raster rows (UNSCALED q, the kernel applies hd^-0.5), rpb4 f32 (heads, 49) with entry (dy+3)*7 + dx+3"""
    g = torch.Generator().manual_seed(700 + 10 * heads + hd + ATT4_CLASSES.index(cls))
    nW, C = (ATT4_H // 4) * (ATT4_W // 4), heads * hd
    rn = lambda *s: torch.randn(*s, generator=g)                                # noqa: E731
    q, k, v = rn(nW, heads, 16, hd), rn(nW, heads, 16, hd), rn(nW, heads, 16, hd)
    rpb4 = rn(heads, 49)
    u = torch.ones(hd) / hd ** 0.5
    if cls == "one_hot":
        c = 40 + 20 * torch.rand(nW, heads, 16, 1, generator=g)
        a = 4.0 * torch.arange(16.0)[torch.randperm(16, generator=g)].reshape(1, 1, 16, 1)
        q, k = c * u + 0.01 * q, a * u + 0.01 * k
        rpb4 = 0.1 * rpb4
    elif cls == "uniform":
        q = torch.zeros_like(q)
        rpb4 = torch.full_like(rpb4, 0.375)
    elif cls == "bias30":
        rpb4 = 30.0 * torch.where(rpb4 > 0, 1.0, -1.0)
    else:
        raise KeyError(cls)

    def raster(t):                       # (nW, heads, 16, hd) -> (H*W, C): window_reverse at 4, heads merged
        t = t.permute(0, 2, 1, 3).reshape(ATT4_H // 4, ATT4_W // 4, 4, 4, C)
        return t.permute(0, 2, 1, 3, 4).reshape(ATT4_H * ATT4_W, C)
    qkv = torch.cat([raster(q), raster(k), raster(v)], -1).to(dtype)
    return {"qkv": qkv, "rpb4": rpb4.float().contiguous(), "heads": heads, "hd": hd}


def _attention4(case, dt, r):
    heads, hd = case["heads"], case["hd"]
    C, nW = heads * hd, (ATT4_H // 4) * (ATT4_W // 4)

    def windows(t):                      # (H*W, C) -> (nW, heads, 16, hd)
        t = t.reshape(ATT4_H // 4, 4, ATT4_W // 4, 4, heads, hd).permute(0, 2, 4, 1, 3, 5)
        return t.reshape(nW, heads, 16, hd)
    qkv = case["qkv"].to(dt)
    q, k, v = windows(qkv[:, :C]), windows(qkv[:, C:2 * C]), windows(qkv[:, 2 * C:])
    c = torch.arange(4)
    ys, xs = (t.reshape(-1) for t in torch.meshgrid(c, c, indexing="ij"))
    ent = (ys[:, None] - ys[None, :] + 3) * 7 + (xs[:, None] - xs[None, :] + 3)
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5 + case["rpb4"].to(dt)[:, ent].unsqueeze(0)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    o = (r("p", e) @ v) / e.sum(-1, keepdim=True)                               # (nW, heads, 16, hd)
    o = o.permute(0, 2, 1, 3).reshape(ATT4_H // 4, ATT4_W // 4, 4, 4, C).permute(0, 2, 1, 3, 4).reshape(ATT4_H * ATT4_W, C)
    return r("o", o), torch.softmax(s, -1)


def attention4_ref(case) -> Tuple[Tensor, Tensor]:
    """float64 (output (H*W, C) raster rows, probabilities (nW, heads, 16, 16))"""
    return _attention4(case, torch.float64, lambda name, x: x)


def attention4_emu(case, dtype) -> Tensor:
    if dtype is None:
        return attention4_ref(case)[0]
    b = Budget(("p", "o") if dtype != F32 else (), TAG[dtype] if dtype != F32 else "bf16")
    return _attention4(case, torch.float32, b.r)[0]


def attention_bwd_condition(case, do: Tensor):
    """per-row condition numbers of (dq, dk, dv, dbias), float64: the sum of the magnitudes that enter a row over the largest
    magnitude that comes out.  dS = P (dP - dot) is formed from terms of size P (|dP| + |dot|); a relative perturbation e of P, dS or
    the logits moves a row of dq by at most e * sum_j P_j (|dP_j| + |dot|) |k_j|, which is this number times the row's largest |dq|.
    Rows whose dS cancels (nearly one-hot P) have a large one: there a relative row error of order 1 is rounding, not a fault."""
    nW, heads, hd = ATT_NW, case["heads"], case["hd"]
    q, k, v = case["q"].double(), case["k"].double(), case["vt"].double().transpose(-1, -2)
    do = do.double().reshape(nW, 64, heads, hd).permute(0, 2, 1, 3)
    p = torch.softmax(attention_logits(case), -1)
    dp = do @ v.transpose(-1, -2)
    dot = (p * dp).sum(-1, keepdim=True)
    a = p * (dp.abs() + dot.abs())                                         # magnitude entering dS
    ds = p * (dp - dot)
    tiny = 1e-300
    cq = (a @ k.abs()).amax(-1) / (ds @ k).abs().amax(-1).clamp_min(tiny)
    ck = (a.transpose(-1, -2) @ q.abs()).amax(-1) / (ds.transpose(-1, -2) @ q).abs().amax(-1).clamp_min(tiny)
    cv = (p.transpose(-1, -2) @ do.abs()).amax(-1) / (p.transpose(-1, -2) @ do).abs().amax(-1).clamp_min(tiny)
    cb = a.sum(0).amax(-1) / ds.sum(0).abs().amax(-1).clamp_min(tiny)
    conds = tuple(c.reshape(-1).clamp_min(1.0) for c in (cq, ck, cv, cb))
    # an ABSOLUTE operand error d (f16: P and dS below 2^-14 are rounded on the subnormal grid, d = 2^-25) moves a row by
    # d * sum |partner operand|: that sum over the row's largest output magnitude
    ones = torch.ones_like(p)
    aq = (ones @ k.abs()).amax(-1) / (ds @ k).abs().amax(-1).clamp_min(tiny)
    ak = (ones @ q.abs()).amax(-1) / (ds.transpose(-1, -2) @ q).abs().amax(-1).clamp_min(tiny)
    av = (ones @ do.abs()).amax(-1) / (p.transpose(-1, -2) @ do).abs().amax(-1).clamp_min(tiny)
    amps = tuple(a_.reshape(-1) + 1.0 / o_.reshape(-1) for a_, o_ in
                 ((aq, (ds @ k).abs().amax(-1).clamp_min(tiny)), (ak, (ds.transpose(-1, -2) @ q).abs().amax(-1).clamp_min(tiny)),
                  (av, (p.transpose(-1, -2) @ do).abs().amax(-1).clamp_min(tiny)))) + (torch.zeros_like(conds[3]),)
    return conds, amps


# ---------------------------------------------------------------------------------------------------------------------------
# a whole LeWin block on LayerNorm classes (the LN1 / LN2 inside the fused kernels): oracle/bf16_budget.py's block with every
# rounding point of the type switched on, in float32, against the same block in float64 with none (the type's GELU form in both)
# ---------------------------------------------------------------------------------------------------------------------------
BLOCK_SWITCHES = ("w", "xn", "qkv", "p", "o", "z", "h1", "g2", "gelu")


def block_params(sd: Dict[str, Tensor], dtype) -> Dict[str, Tensor]:
    """a block's state_dict with the GEMM weights already T-valued (the reference is the float64 block on those weights)"""
    gemm = ("to_q.weight", "to_kv.weight", "proj.weight", "linear1.0.weight", "linear2.0.weight")
    return {k: (rnd(dtype)(v.float()) if k.endswith(gemm) else v) for k, v in sd.items()}


def block_ref(x: Tensor, p: Dict[str, Tensor], heads: int, dtype) -> Tensor:
    from oracle import bf16_budget as BB
    pd = {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}
    return BB._block(x.double(), pd, "", heads, 0, Budget(("gelu",) if dtype != F32 else (), "bf16"))


def block_emu(x: Tensor, p: Dict[str, Tensor], heads: int, dtype) -> Tensor:
    from oracle import bf16_budget as BB
    if dtype is None:                                                        # switches off: float64, erf GELU -- as block_ref(F32)
        return block_ref(x, p, heads, F32)
    pf = {k: (v.float() if v.is_floating_point() else v) for k, v in p.items()}

    def ln_tree(x, w, b, eps=1e-5):                                          # the statistics of ln_emu (halving-tree sums)
        C = x.shape[-1]
        v = x - tree_sum(x) * (1.0 / C)
        return v * (1.0 / torch.sqrt(tree_sum(v * v) * (1.0 / C) + eps)) * w + b
    keep, BB.O.layer_norm = BB.O.layer_norm, ln_tree
    try:
        return BB._block(x.float(), pf, "", heads, 0, Budget(BLOCK_SWITCHES if dtype != F32 else (), TAG[dtype] if dtype != F32 else "bf16"))
    finally:
        BB.O.layer_norm = keep
