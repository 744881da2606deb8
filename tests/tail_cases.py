"""Helpers of the training-tail audit (tests/test_gpu_tail_exact.py, tests/test_tail_reference.py).  Not a conftest: plain functions.

The 14 entry points of uf_train.hip are streaming kernels whose arithmetic is a short fixed sequence of float32 operations, so most of them have
a BIT reference: the same sequence in numpy, one IEEE operation per line, nothing fused but the one fmaf the kernel spells out (Part A).  Reductions (loss, MSE, SSIM) are gated at 1 ulp
of float32 against float64.  Part B is the arena: one flat allocation per operand family filled with a NaN pattern, tensors placed at chosen
element offsets with guard gaps, so that placement (16-byte alignment decides the kernel's path) is under the test's control, an over-read
yields NaN and an over-write destroys a pattern that is looked for afterwards.  Part C: the comparison functions and the report; Part D: case
lists and data; Part E: stand-in faulty kernels, which the CPU companion feeds to the SAME comparison functions on the SAME case data.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

f32, f64 = np.float32, np.float64
POISON = 0x7FC0BEEF                      # the quiet NaN of tests/edge_cases.py
FLT_MAX = f32(3.4028234663852886e38)
UF_OK, UF_ERR_SHAPE, UF_ERR_ALIGN, UF_ERR_NULL = 0, -1, -3, -6
AW_MAX, AW_CHUNK = 40, 8192              # tensors per launch, elements per workgroup (uf_train.hip)


def A(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=f32)


# ---------------------------------------------------------------------------------------------------------------------------
# Part A: emulations.  Every line is one float32 operation on float32 operands (fma32, defined in Part E, is one operation too).
# ---------------------------------------------------------------------------------------------------------------------------
def adamw_consts(lr: float, b1: float, b2: float, eps: float, wd: float, step: int, grad_scale: float) -> Dict[str, np.float32]:
    """the kernel's scalar arguments, rounded from double once, as adamw_any rounds them"""
    bc1, bc2 = 1.0 - math.pow(b1, step), 1.0 - math.pow(b2, step)
    return dict(decay=f32(1.0 - lr * wd), omb1=f32(1.0 - b1), omb2=f32(1.0 - b2), b2=f32(b2), step=f32(lr / bc1), bc2s=f32(math.sqrt(bc2)),
                eps=f32(eps), gs=f32(grad_scale))


def adamw_emu(p, g, m, v, c) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """one step of the kernel's ``upd`` on float32 arrays: returns (p, m, v)"""
    p, g, m, v = A(p), A(g), A(m), A(v)
    g = g * c["gs"]
    p = p * c["decay"]
    gm = g - m
    m = fma32(c["omb1"], gm, m)          # the kernel spells this one fmaf out (torch's lerp is fused as well)
    vb = v * c["b2"]
    gg = g * g
    gg = c["omb2"] * gg
    v = vb + gg
    den = np.sqrt(v)
    den = den / c["bc2s"]
    den = den + c["eps"]
    q = m / den
    q = c["step"] * q
    p = p - q
    return p, m, v


def scaled_consts(lr, b1, b2, eps, wd, grad_scale, state, pair=None) -> Optional[Dict[str, np.float32]]:
    """uf_adamw_step_scaled: None when found_inf is set; else the constants with gs * state[1] and the two step constants at t = state[4] + 1
    (``pair`` = (stepf, bc2s) overrides the host values: the device computes them with its own double pow / sqrt)"""
    state = A(state)
    if state[2] != 0:
        return None
    c = adamw_consts(lr, b1, b2, eps, wd, 1, grad_scale)
    c["gs"] = c["gs"] * state[1]
    t = float(state[4]) + 1.0
    c["step"], c["bc2s"] = f32(lr / (1.0 - math.pow(b1, t))), f32(math.sqrt(1.0 - math.pow(b2, t)))
    if pair is not None:
        c["step"], c["bc2s"] = pair
    return c


def neighbours(x: np.float32) -> List[np.float32]:
    return [x, np.nextafter(x, f32(-np.inf)), np.nextafter(x, f32(np.inf))]


def scaled_pairs(c) -> List[Tuple[np.float32, np.float32]]:
    """{host value, its two float32 neighbours}^2, the host pair first"""
    return [(s, b) for s in neighbours(c["step"]) for b in neighbours(c["bc2s"])]


def charbonnier_emu(y, t, eps: float, grad_scale: float):
    """(dy, loss float32, the float64 mean before its rounding).  dy in float32, one operation per line.  The loss term is taken in float64 from the
    float32 inputs, as the kernel takes it (the difference is exact there; eps^2 is the float32 product the kernel is handed): the float64 total, * 1/n,
    rounded to float32 once."""
    y, t = A(y).reshape(-1), A(t).reshape(-1)
    n = y.size
    eps2 = f32(eps) * f32(eps)
    gs = f32(grad_scale) / f32(n)
    d = y - t
    dd = d * d
    s = dd + eps2
    r = np.sqrt(s)
    num = gs * d
    dy = num / r
    d64 = y.astype(f64) - t.astype(f64)
    dd64 = d64 * d64
    s64 = dd64 + f64(eps2)
    r64 = np.sqrt(s64)
    mean = float(r64.sum()) * (1.0 / n)
    return dy, f32(mean), mean


def mixup_emu(x, lam, perm):
    x, lam = A(x), A(lam)
    B = x.shape[0]
    l = lam.reshape(B, *([1] * (x.ndim - 1)))
    y = x[np.asarray(perm)]
    a = l * x
    b = f32(1) - l
    c = b * y
    return a + c


def found_inf_emu(grads: Sequence[np.ndarray], state) -> np.ndarray:
    s = A(state).copy()
    for g in grads:
        if g.size and not bool(np.all(np.abs(A(g)) <= FLT_MAX)):      # false for inf and for nan
            s[2] = 1.0
    return s


def scaler_update_emu(state, growth: float, backoff: float, interval: int) -> np.ndarray:
    s = A(state).copy()
    scale, tracker = s[0], s[3]
    with np.errstate(over="ignore", divide="ignore"):
        if s[2] != 0:
            scale = scale * f32(backoff)
            tracker = f32(0)
        else:
            s[4] = s[4] + f32(1)
            tracker = tracker + f32(1)
            if tracker >= f32(interval):
                scale = scale * f32(growth)
                tracker = f32(0)
        s[0], s[1], s[2], s[3] = scale, f32(1) / scale, f32(0), tracker
    return s


def clamp01(x: np.ndarray) -> np.ndarray:
    """torch.clamp(x, 0, 1): NaN stays NaN"""
    x = A(x)
    return np.where(x < 0, f32(0), np.where(x > 1, f32(1), x)).astype(f32)


def mse_ref(a, b, clamp: bool) -> np.ndarray:
    """per image, in float64: the sum of the float32 squares of the float32 differences, / per"""
    a, b = A(a), A(b)
    if clamp:
        a, b = clamp01(a), clamp01(b)
    n = a.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (a - b).reshape(n, -1)
        sq = d * d
        return sq.astype(f64).sum(1) * (1.0 / sq.shape[1])


def ssim_sanitize(x: np.ndarray) -> np.ndarray:
    """pixels whose quantisation is undefined in the reference (NaN, inf, |255 v| >= 2^31) quantise to 0, as uf_batch_ssim documents"""
    x = A(x).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(x * f32(255))
        x[~(np.abs(q) < f32(2147483520.0))] = 0
    return x


def ssim_ref(a: np.ndarray, b: np.ndarray) -> float:
    import torch
    from oracle import uformer_oracle as O
    return O.ssim(torch.from_numpy(ssim_sanitize(a)), torch.from_numpy(ssim_sanitize(b)))


def pad_ref(img: np.ndarray, Xh: int, Xw: int, off=lambda X, h: (X - h) // 2):
    B, C, h, w = img.shape
    y0, x0 = off(Xh, h), off(Xw, w)
    canvas, mask = np.zeros((B, C, Xh, Xw), f32), np.zeros((B, 1, Xh, Xw), f32)
    canvas[:, :, y0:y0 + h, x0:x0 + w] = img
    mask[:, :, y0:y0 + h, x0:x0 + w] = 1
    return canvas, mask


def crop_ref(canvas: np.ndarray, h: int, w: int, clamp: bool) -> np.ndarray:
    Xh, Xw = canvas.shape[-2:]
    y0, x0 = (Xh - h) // 2, (Xw - w) // 2
    out = A(canvas[:, :, y0:y0 + h, x0:x0 + w])
    return clamp01(out) if clamp else out


def clamp_meta(meta: np.ndarray, N: int, H: int, W: int, ps: int) -> np.ndarray:
    """crop_aug_kernel's policy: idx into [0, N), r0 into [0, H - ps], c0 into [0, W - ps], k & 7"""
    m = np.array(meta, dtype=np.int64).reshape(-1, 4)
    m[:, 0] = np.clip(m[:, 0], 0, N - 1)
    m[:, 1] = np.clip(m[:, 1], 0, H - ps)
    m[:, 2] = np.clip(m[:, 2], 0, W - ps)
    m[:, 3] &= 7
    return m.astype(np.int32)


def crop_augment_ref(frames_chw: np.ndarray, meta: np.ndarray, ps: int, transform=None) -> np.ndarray:
    """frames (N, C, H, W) float32 (uint8 frames: pass float32(v) / float32(255)); meta already valid"""
    import torch
    from oracle import uformer_oracle as O
    fn = transform or O.crop_augment
    fr = torch.from_numpy(A(frames_chw))
    return torch.stack([fn(fr[i], r, c, ps, k) for i, r, c, k in np.asarray(meta).tolist()]).numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# Part B: the arena (torch: it lives on the device under test; "cpu" for the companion)
# ---------------------------------------------------------------------------------------------------------------------------
GAP = 8                                  # guard words in front of, between and behind tensors (>= 2 vector widths)


def layout(lengths: Sequence[int], mods: Sequence[int], gap: int = GAP) -> Tuple[List[int], int]:
    """element offsets with offset % 4 == mod for each tensor and >= gap guard words around each: (offsets, arena words)"""
    offs, cur = [], gap
    for n, mod in zip(lengths, mods):
        cur += (mod - cur) % 4
        offs.append(cur)
        cur += n + gap
    return offs, cur + (-cur) % 4


class Arena:
    def __init__(self, words: int, device="cpu"):
        import torch
        self.bits = torch.full((words,), POISON, dtype=torch.int32, device=device)
        self.f = self.bits.view(torch.float32)
        self.live = torch.zeros(words, dtype=torch.bool, device=device)
        self.base = self.bits.data_ptr()
        assert self.base % 16 == 0

    def place(self, off: int, values) -> "object":
        """copy ``values`` (numpy, any dtype of 4 bytes is taken as float32 values) to elements [off, off + n): returns the live view"""
        import torch
        v = torch.from_numpy(A(values).reshape(-1))
        n = v.numel()
        assert 0 <= off and off + n <= self.bits.numel() and not bool(self.live[off:off + n].any())
        self.f[off:off + n].copy_(v)
        self.live[off:off + n] = True
        return self.f[off:off + n]

    def write(self, off: int, values) -> None:
        import torch
        v = torch.from_numpy(A(values).reshape(-1))
        assert bool(self.live[off:off + v.numel()].all())
        self.f[off:off + v.numel()].copy_(v)

    def ptr(self, off: int) -> int:
        return self.base + 4 * off

    def read(self, off: int, n: int) -> np.ndarray:
        return self.f[off:off + n].cpu().numpy().copy()

    def guards_intact(self) -> bool:
        return bool((self.bits[~self.live] == POISON).all())

    def snapshot(self):
        return self.bits.clone()

    def unchanged(self, snap) -> bool:
        import torch
        return bool(torch.equal(self.bits, snap))


# ---------------------------------------------------------------------------------------------------------------------------
# Part C: comparisons and the report
# ---------------------------------------------------------------------------------------------------------------------------
RECORDS: Dict[str, Dict[str, object]] = {}
ZERO_GATED = ("uf_adamw_step", "uf_adamw_step_scaled", "uf_grad_scaler_check", "uf_grad_scaler_update", "uf_charbonnier_fwd_bwd:dy", "uf_expand2square",
              "uf_expand_canvas", "uf_crop_clamp", "uf_crop_clamp_canvas", "uf_crop_augment_c", "uf_mixup")
ULP_GATED = ("uf_charbonnier_fwd_bwd:loss", "uf_batch_mse", "uf_batch_ssim")


def record(entry: Optional[str], elements: int, differing: int, ulp: float) -> None:
    if entry is None:
        return
    r = RECORDS.setdefault(entry, {"cases": 0, "elements": 0, "differing": 0, "worst_ulp": 0.0})
    r["cases"] += 1
    r["elements"] += int(elements)
    r["differing"] += int(differing)
    r["worst_ulp"] = max(r["worst_ulp"], float(ulp))


def bits(a) -> np.ndarray:
    return A(a).reshape(-1).view(np.uint32)


def _ordered(a) -> np.ndarray:
    k = A(a).reshape(-1).view(np.int32).astype(np.int64)
    return np.where(k < 0, -(k & 0x7FFFFFFF), k)


def ulp_distance(got, want) -> np.ndarray:
    """float32 grid steps between got and want (+0 and -0 coincide); NaN against NaN is 0, NaN against a number is 2^32"""
    g, w = A(got).reshape(-1), A(want).reshape(-1)
    d = np.abs(_ordered(g) - _ordered(w)).astype(f64)
    gn, wn = np.isnan(g), np.isnan(w)
    d[gn & wn] = 0
    d[gn ^ wn] = 2.0 ** 32
    return d


def diff_bits(entry: Optional[str], got, want) -> int:
    """GATE ZERO: the number of elements whose 32 bits differ"""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    n = int((g != w).sum())
    record(entry, g.size, n, float(ulp_distance(got, want).max()) if n else 0.0)
    return n


def diff_values(entry: Optional[str], got, want) -> int:
    """gate zero by VALUE plus NaN mask (clamped outputs: the sign of zero and the payload of a NaN are not pinned by torch.clamp)"""
    g, w = A(got).reshape(-1), A(want).reshape(-1)
    assert g.shape == w.shape, (g.shape, w.shape)
    gn, wn = np.isnan(g), np.isnan(w)
    n = int(((gn != wn) | (~gn & ~wn & (g != w))).sum())
    record(entry, g.size, n, float(ulp_distance(g, w).max()) if n else 0.0)
    return n


def worst_ulp(entry: Optional[str], got, want64) -> float:
    """1-ULP GATE: distance of the float32 ``got`` from the float64 ``want64`` in units of the float32 spacing at want64 (a correctly rounded result is
    <= 0.5; non-finite expectations must match in kind)"""
    g, w = A(got).reshape(-1).astype(f64), np.asarray(want64, dtype=f64).reshape(-1)
    assert g.shape == w.shape, (g.shape, w.shape)
    fin = np.isfinite(w)
    with np.errstate(invalid="ignore", over="ignore"):
        w32 = w.astype(f32)
    sp = np.spacing(np.abs(np.where(fin, w32, f32(1)))).astype(f64)
    with np.errstate(invalid="ignore"):
        u = np.where(fin, np.abs(g - w) / sp, np.where((np.isnan(g) & np.isnan(w)) | (g == w), 0.0, np.inf))
    u = np.where(np.isnan(u), np.inf, u)
    worst = float(u.max()) if u.size else 0.0
    record(entry, g.size, int((u > 1.0).sum()), worst)
    return worst


SCALED_PAIRS: List[Dict[str, object]] = []     # which (stepf, bc2s) candidate each scaled-AdamW launch matched
WALL: Dict[str, float] = {}


def write_report() -> None:
    """RECORDS to $UF_REPORT_DIR/parity_tail.json when that variable names a directory (as tests/test_gpu_edges.py does)"""
    out = os.environ.get("UF_REPORT_DIR")
    if not out or not os.path.isdir(out):
        return
    with open(os.path.join(out, "parity_tail.json"), "w") as f:
        json.dump({"entry_points": RECORDS, "zero_gated": list(ZERO_GATED), "ulp_gated": list(ULP_GATED), "scaled_adamw_constant_pairs": SCALED_PAIRS,
                   "wall_seconds": WALL}, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------------------------------------
# Part D: case lists and data
# ---------------------------------------------------------------------------------------------------------------------------
HYPER = dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8)        # train/train_denoise.py:77
ADAMW_LENGTHS = (1, 3, 4, 5, 8191, 8192, 8193, 16387)
ADAMW_PLACEMENTS = {"aligned": (0, 0, 0, 0), "g1": (0, 1, 0, 0), "g2": (0, 2, 0, 0), "g3": (0, 3, 0, 0), "p1": (1, 0, 0, 0), "p1g2m3": (1, 2, 3, 0)}
# name -> (grad_scale, weight_decay, data): see adamw_data
ADAMW_SETTINGS = {"gs1_wd": (1.0, 0.02, "plain"), "gs0.25_wd": (0.25, 0.02, "plain"), "gs_third_nowd": (1.0 / 3.0, 0.0, "plain"), "zero_grad": (1.0, 0.02, "zero"),
                  "mixed_signs": (1.0, 0.02, "mixed")}


def adamw_setting_data(lengths, seed, setting: str, steps: int = 3):
    kind = ADAMW_SETTINGS[setting][2]
    return adamw_data(lengths, seed, zero_grad=kind == "zero", steps=steps, mixed_signs=kind == "mixed")
SMALL_LENGTHS = (1, 3, 4, 5, 7, 64, 130, 257)
# the seeds of the GPU file's AdamW data: the CPU companion draws the SAME data
ADAMW_SEEDS = {"placements": 11, "same_bits": 12, "counts": 21, "scaled": 31}


def _cycle(n: int, big_at: int = -1) -> List[int]:
    return [8193 if i == big_at else SMALL_LENGTHS[i % len(SMALL_LENGTHS)] for i in range(n)]


# name -> lengths; 0 = a zero-length entry, passed with NULL pointers
ADAMW_COUNTS = {
    "count1": [5],
    "count40": _cycle(40, 17),
    "count41": _cycle(41, 40),                                  # the 41st tensor alone in the second launch, and longer than a chunk
    "count81": _cycle(81, 43),                                  # three launches; a multi-chunk tensor in the second
    "first_empty": [0, 5, 0, 0, 8193, 0, 3],
    "empties_interleaved_77_of_90": [0 if i % 7 == 3 else n for i, n in enumerate(_cycle(90, 50))],   # 13 empties among 90 entries, 77 live: two launch groups
    "40_then_empties": _cycle(40, 5) + [0, 0, 0, 0, 0],          # the second launch group finds c == 0
    "all_empty": [0, 0, 0],
}
SCALED_STEPS = (0, 1, 9, 999, 100000)
SCALED_SCALES = (65536.0, 1000.0)


def adamw_data(lengths: Sequence[int], seed: int, zero_grad: bool = False, steps: int = 3, mixed_signs: bool = False):
    """per tensor: p, m, v and one g per step.  g ~ N(0,1) x 10^(i % 5 - 3), the spread of a real model's gradients; m, v as after some training.
    Zero-length entries get empty arrays.

    Two conditions hold for ALL the data, so that the emulation can be held to 1 ulp of torch.optim.AdamW, whose CPU kernels fuse and order the same
    formulas differently: (a) |p| >= 0.05.  torch's addcdiv forms p + (-step)(m / denom) with the product unrounded; the emulation rounds step * q
    first.  The two differ by at most half an ulp of step * q, which is below half an ulp of the result while |step * q| <= |p|; step * q stays
    under 1e-2 here (step <= 2e-3, |q| < 5).  A weight within 1e-2 of zero would leave that regime (a first draw with p ~ N(0,1) held one: p = 3.9e-6,
    2 ulp from torch).  (b) v >= 0.3 scale^2, the running mean of g^2: it dwarfs (1 - b2) g^2, so the order in which torch's addcmul multiplies
    (value * g) * g against the kernel's value * (g * g) cannot move v by more than an ulp.

    In the default data m and every g of an element also share a sign: nothing cancels in m.  ``mixed_signs`` gives m and g independent signs:
    m + (1 - b1)(g - m) cancels, which is where a fused and an unfused first moment part by thousands of ulp."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(lengths):
        sc = 10.0 ** (i % 5 - 3)
        sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        p = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.05 + np.abs(rng.standard_normal(n)))).astype(f32)
        if mixed_signs:
            m = (rng.standard_normal(n) * 0.1 * sc).astype(f32)
            gs = [(rng.standard_normal(n) * sc).astype(f32) for _ in range(steps)]
        else:
            m = (sgn * np.abs(rng.standard_normal(n)) * 0.1 * sc).astype(f32)
            gs = [(sgn * np.abs(rng.standard_normal(n)) * sc).astype(f32) for _ in range(steps)]
        v = ((0.3 + 0.3 * rng.standard_normal(n) ** 2) * sc * sc).astype(f32)
        if zero_grad:
            gs = [np.zeros(n, f32) for _ in range(steps)]
        out.append(dict(p=p, m=m, v=v, g=gs))
    return out


def adamw_run_emu(data, wd: float, grad_scale: float, steps: int = 3, first_step: int = 1, upd=adamw_emu):
    """the emulated trajectory: list over steps of list over tensors of (p, m, v)"""
    cur = [(d["p"], d["m"], d["v"]) for d in data]
    traj = []
    for s in range(steps):
        c = adamw_consts(HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, first_step + s, grad_scale)
        cur = [upd(p, d["g"][s], m, v, c) for (p, m, v), d in zip(cur, data)]
        traj.append(cur)
    return traj


SCALER_TABLE = [   # (state[0..7], growth, backoff, interval)
    ([65536.0, 1 / 65536.0, 0, 0, 0, 0, 0, 0], 2.0, 0.5, 2000),                 # clean, far from growth
    ([65536.0, 1 / 65536.0, 1, 5, 7, 0, 0, 0], 2.0, 0.5, 2000),                 # found: back off, tracker reset, count kept
    ([1024.0, 1 / 1024.0, 0, 2, 10, 0, 0, 0], 2.0, 0.5, 3),                     # tracker at interval - 1: grows
    ([1024.0, 1 / 1024.0, 0, 1, 10, 0, 0, 0], 2.0, 0.5, 3),                     # one short of it
    ([1000.0, 1 / 1000.0, 0, 0, 0, 0, 0, 0], 1.5, 0.5, 1),                      # non power of two, growth 1.5, interval 1: 1 / 1500 correctly rounded
    ([1500.0, 1 / 1500.0, 0, 0, 1, 0, 0, 0], 1.5, 0.5, 1),                      # 2250
    ([3375.0, 1 / 3375.0, 1, 0, 3, 0, 0, 0], 1.5, 0.3, 1),                      # backoff 0.3 (not a float32): 3375 * float32(0.3)
    ([1000.0, 1 / 1000.0, float("nan"), 1, 3, 0, 0, 0], 2.0, 0.5, 4),           # a NaN flag counts as set (NaN != 0)
    ([3.0, 1 / 3.0, 2.0, 1, 3, 0, 0, 0], 2.0, 0.5, 4),                          # any non-zero flag
    ([1e-3, 1e3, 0, 3, 16777215.0, 0, 0, 0], 1.5, 0.5, 4),                      # tiny scale; count just under 2^24
    ([65536.0, 1 / 65536.0, 0, 1999, 123456, 11.0, -12.0, 13.5], 2.0, 0.5, 2000),   # the default interval's last step; words 5..7 are not the kernel's
    ([3.0e38, 1 / 3.0e38, 0, 0, 0, 0, 0, 0], 2.0, 0.5, 1),                      # growth overflows to inf, 1 / inf = 0: as the emulation
]

CHARB_NS = (1, 2, 3, 4, 5, 7, 1027, 4 * 2048 * 256 + 7)
CHARB_SETTINGS = tuple((eps, gs) for eps in (1e-3, 1e-6, 0.5) for gs in (1.0, 65536.0, 1.0 / 3.0))
CHARB_DATA = ("gauss", "equal", "d1e-8", "d1e4")


def charb_data(kind: str, n: int, seed: int = 5):
    rng = np.random.default_rng(seed + n)
    t = rng.random(n).astype(f32)
    if kind == "gauss":
        y = (t + rng.standard_normal(n) * 0.1).astype(f32)
    elif kind == "equal":
        y = t.copy()
    elif kind == "d1e-8":                                        # below float32's resolution at t ~ 0.5: give the difference its own scale
        t = (t * f32(1e-7)).astype(f32)
        y = (t + np.where(rng.random(n) < 0.5, -1, 1) * f32(1e-8)).astype(f32)
    elif kind == "d1e4":
        y = (t + np.where(rng.random(n) < 0.5, -1, 1) * f32(1e4)).astype(f32)
    else:
        raise KeyError(kind)
    return y, t


MSE_SHAPES = [(n, C, 12, 12) for n in (1, 64, 65, 130) for C in (1, 3, 4)] + [(2, 1, 64, 64), (2, 1, 1, 4097), (1, 3, 1700, 1700)]


def mse_data(shape):
    """images a little outside [0, 1] (the clamp matters) and a noisy copy"""
    rng = np.random.default_rng(sum(shape))
    a = (rng.random(shape) * 1.4 - 0.2).astype(f32)
    b = (a + rng.standard_normal(shape).astype(f32) * f32(0.05)).astype(f32)
    return a, b


def mse_oracle64(a, b, clamp: bool) -> np.ndarray:
    """the float64 oracle of myPSNR's mean squared error: clamp, then difference, square and mean all in float64 (exact squares)"""
    a, b = A(a), A(b)
    if clamp:
        a, b = clamp01(a), clamp01(b)
    d = (a.astype(f64) - b.astype(f64)).reshape(a.shape[0], -1)
    return (d * d).mean(1)


SSIM_HW = ((11, 11), (11, 43), (27, 11), (26, 26), (27, 27), (43, 27))
SSIM_DATA = ("noisy", "identical", "constant", "inverted", "wrap", "nonfinite")


def ssim_pair(kind: str, C: int, H: int, W: int, seed: int):
    rng = np.random.default_rng(seed)
    a = rng.random((C, H, W)).astype(f32)
    b = np.clip(a + rng.standard_normal((C, H, W)).astype(f32) * f32(0.1), 0, 1).astype(f32)
    if kind == "identical":
        b = a.copy()
    elif kind == "constant":
        a, b = np.full_like(a, 0.4), np.full_like(a, 0.6)
    elif kind == "inverted":
        b = (f32(1) - a).astype(f32)
    elif kind == "wrap":
        a.reshape(-1)[::5] = -0.3
        b.reshape(-1)[::7] = 1.7
    elif kind == "nonfinite":
        for i, val in enumerate((np.nan, np.inf, -np.inf, 1e30)):
            a.reshape(-1)[3 + 11 * i] = val
            b.reshape(-1)[5 + 13 * i] = val
    return a, b


# (B, C, h, w, Xh, Xw): odd X - h and X - w, h == X, w = 1, every C, and one canvas beyond 2048 x 1024 elements (the grid-stride loop wraps)
PAD_SHAPES = [(2, 1, 5, 8, 8, 13), (2, 3, 7, 1, 10, 4), (2, 4, 6, 6, 6, 9), (2, 6, 3, 5, 8, 8), (2, 3, 9, 9, 9, 9), (1, 3, 600, 801, 896, 896)]


def pad_image(B, C, h, w, seed=3) -> np.ndarray:
    rng = np.random.default_rng(seed + h * w)
    img = (rng.random((B, C, h, w)) * 1.6 - 0.3).astype(f32)
    flat = img.reshape(-1)
    for i, val in enumerate((np.nan, np.inf, -np.inf, -0.0)):
        flat[(7 * i + 1) % flat.size] = val
    return img


def index_frames(N: int, C: int, H: int, W: int) -> np.ndarray:
    """float32 frames (N, C, H, W) whose value is the element's own flat index: a wrong source pixel cannot go unnoticed"""
    assert N * C * H * W < 2 ** 24
    return np.arange(N * C * H * W, dtype=f32).reshape(N, C, H, W)


AUG_FRAME = (3, 50, 57)                  # N, H, W: not square
AUG_PS = (1, 2, 7, 48)


def aug_meta(N: int, H: int, W: int, ps: int) -> np.ndarray:
    """16 entries: every transform twice, crop origins that reach both borders"""
    rows = []
    for i in range(16):
        r0 = (0, H - ps, (5 * i) % (H - ps + 1))[i % 3]
        c0 = (W - ps, 0, (7 * i) % (W - ps + 1))[i % 3]
        rows.append([i % N, r0, c0, i % 8])
    return np.array(rows, dtype=np.int32)


def bad_meta(N: int, H: int, W: int, ps: int) -> np.ndarray:
    """one bad field per entry: idx in {-1, N}, r0 / c0 off by <= 4, k in {-1, 11}"""
    r, c = (H - ps) // 2, (W - ps) // 2
    return np.array([[-1, r, c, 1], [N, r, c, 2], [0, -4, c, 3], [N - 1, H - ps + 4, c, 4], [1, r, -3, 5], [N - 1, r, W - ps + 4, 6], [1, -1, c, 0],
                     [1, r, c, -1], [0, r, c, 11]], dtype=np.int32)


def meta_extent(meta_row, C: int, H: int, W: int, ps: int) -> Tuple[int, int]:
    """(lowest, highest) element offset from frame 0 that an UNCLAMPED kernel would read for this entry (either layout: both are dense (N, .) stacks)"""
    idx, r0, c0, _ = (int(v) for v in meta_row)
    lo = (idx * C * H + r0) * W + c0                             # channel 0, first crop row and column
    hi = ((idx * C + C - 1) * H + r0 + ps - 1) * W + c0 + ps - 1
    lo_hwc = ((idx * H + r0) * W + c0) * C
    hi_hwc = ((idx * H + r0 + ps - 1) * W + c0 + ps - 1) * C + C - 1
    return min(lo, lo_hwc), max(hi, hi_hwc)


MIXUP_SHAPES = [(1, 1), (2, 3), (16, 12288), (16, 3), (3, 700000)]     # (B, per_sample); the last is beyond 2048 x 1024 elements
MIXUP_LAMS = (0.0, 1.0, 0.5, 0.3)


def mixup_perms(B: int) -> Dict[str, np.ndarray]:
    ident = np.arange(B)
    fixed = ident.copy()
    if B > 2:
        fixed[[0, B - 1]] = fixed[[B - 1, 0]]                    # two swapped, the rest fixed points
    return {"identity": ident, "reversal": ident[::-1].copy(), "fixed_points": fixed}


def mixup_guarded(x: np.ndarray) -> Tuple[np.ndarray, int]:
    """x (B, per) between one guard sample either side, as the GPU file places it: (flat values of B + 2 samples, element offset of sample 0)"""
    B, per = x.shape
    rng = np.random.default_rng(B + per)
    return np.concatenate([rng.standard_normal(per).astype(f32), A(x).reshape(-1), rng.standard_normal(per).astype(f32)]), per


def perm_extent(p: int, per: int, data_off: int) -> Tuple[int, int]:
    """(first, last) element of the guarded allocation that an UNCLAMPED kernel reads for partner index p"""
    return data_off + p * per, data_off + p * per + per - 1


def mixup_data(B: int, per: int, seed: int = 9):
    rng = np.random.default_rng(seed + B)
    x = rng.standard_normal((B, per)).astype(f32)
    lam = np.array([MIXUP_LAMS[i % 4] for i in range(B)], dtype=f32) if B > 1 else np.array([0.3], f32)
    return x, lam


# ---------------------------------------------------------------------------------------------------------------------------
# Part E: stand-in faulty kernels (numpy).  Each is what a plausible slip in uf_train.hip would compute.
# ---------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c) -> np.ndarray:
    """float32(a * b + c) with ONE rounding.  The float64 product of two float32 is exact; the float64 sum is made round-to-odd (TwoSum gives its exact
    residual), so that the final rounding to float32 cannot round twice."""
    a, b, c = (np.asarray(x, dtype=f32).astype(f64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        s = a * b
        t = s + c
        bb = t - s
        e = (s - (t - bb)) + (c - bb)
        inexact = np.isfinite(t) & (e != 0)
        over = inexact & ((e > 0) != (t > 0))                    # |t| is above the exact sum: step back towards zero first
        t = np.where(over, np.nextafter(t, 0.0), t)
        k = np.ascontiguousarray(t).view(np.int64) | inexact.astype(np.int64)
        return k.view(f64).astype(f32)


def adamw_fused_p(p, g, m, v, c):
    """the vector path before the fix: p = fma(p, decay, -round(step * q)) -- the weight decay product is never rounded"""
    _, m2, v2 = adamw_emu(p, g, m, v, c)
    den = np.sqrt(v2)
    den = den / c["bc2s"]
    den = den + c["eps"]
    q = m2 / den
    q = c["step"] * q
    return fma32(p, c["decay"], -q), m2, v2


def adamw_skip_last(p, g, m, v, c):
    pn, mn, vn = adamw_emu(p, g, m, v, c)
    if pn.size:
        pn[-1], mn[-1], vn[-1] = A(p)[-1], A(m)[-1], A(v)[-1]
    return pn, mn, vn


def adamw_chunk_twice(p, g, m, v, c):
    """the last 8192-chunk of a tensor updated twice (two workgroups mapped to it)"""
    pn, mn, vn = adamw_emu(p, g, m, v, c)
    if pn.size:
        lo = (pn.size - 1) // AW_CHUNK * AW_CHUNK
        pn[lo:], mn[lo:], vn[lo:] = adamw_emu(pn[lo:], A(g)[lo:], mn[lo:], vn[lo:], c)
    return pn, mn, vn


def adamw_wrong_first_chunk(lengths: Sequence[int], traj_step, prev):
    """the first tensor of the SECOND launch group is given the first_chunk of the one after it: its chunk 0 is skipped whenever it has more than
    one chunk, and otherwise the workgroup meant for it updates nothing.  Returns the step's (p, m, v) list with that tensor's first chunk stale."""
    live = [i for i, n in enumerate(lengths) if n > 0]
    out = list(traj_step)
    if len(live) > AW_MAX:
        i = live[AW_MAX]
        p, m, v = (x.copy() for x in traj_step[i])
        p[:AW_CHUNK], m[:AW_CHUNK], v[:AW_CHUNK] = prev[i][0][:AW_CHUNK], prev[i][1][:AW_CHUNK], prev[i][2][:AW_CHUNK]
        out[i] = (p, m, v)
    return out


def found_inf_blind_last_chunk(grads: Sequence[np.ndarray], state) -> np.ndarray:
    cut = [g[:(g.size - 1) // AW_CHUNK * AW_CHUNK] if g.size else g for g in grads]
    return found_inf_emu(cut, state)


def clamp01_nan_to_zero(x: np.ndarray) -> np.ndarray:
    """fminf(fmaxf(v, 0), 1): the kernels before the fix"""
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(A(x), f32(0)), f32(1))


def ssim_drop_last_row(a: np.ndarray, b: np.ndarray) -> float:
    """a tile that leaves out the last row of the (H - 10) x (W - 10) map but keeps the divisor"""
    H = a.shape[-2]
    rows = H - 10
    return ssim_ref(a[:, :H - 1], b[:, :H - 1]) * (rows - 1) / rows if rows > 1 else 0.0


def _augment_with(rot_of_k, flip_first: bool):
    import torch

    def fn(frame, r, c, ps, k):
        x = frame[:, r:r + ps, c:c + ps]
        if flip_first and k >= 4:
            x = x.flip(-2)
        y = torch.rot90(x, k=rot_of_k(k), dims=[-1, -2])
        return y.flip(-2) if (k >= 4 and not flip_first) else y
    return fn


def aug_swapped_1_3():
    return _augment_with(lambda k: {1: 3, 3: 1}.get(k & 3, k & 3), False)


def aug_flip_first():
    return _augment_with(lambda k: k & 3, True)


def pad_offset_up(X: int, h: int) -> int:
    return (X - h + 1) // 2
