"""Exact integer-lattice checks of the linear kernels (helpers; no GPU needed).

The argument.  Draw every operand from a small set of non-zero integers, optionally times a power of two.  Every product is then an
integer multiple of one lattice step, and as long as every partial sum stays below 2^24 steps it is exactly representable in
float32 -- whatever the order the terms are added in, whatever the MFMA shape, fragment layout or split of the reduction.  A correct
kernel that accumulates in float32 must therefore return the float64 result TO THE BIT; where it stores type T it must return that
result rounded once to T, round-to-nearest-even.  The gate is zero and follows from the arithmetic, not from a measurement.

Two conditions make this hold; both are asserted on the float64 REFERENCE only, never on a kernel's output:
  1. ``check_accumulation``: the largest |partial sum| a lattice and a contraction length can produce is below 2^24 steps;
  2. ``check_representable``: for an output (or an intermediate) stored as T, max |reference| is at most 256 steps for bf16 (8 significand
     bits: every integer up to 256 is a bf16) and 2048 for f16 (11 bits).  Rounding is then the identity and a one-step fault cannot
     hide in it.  The rounding cases exceed 256 on purpose (257 -> 256, 259 -> 260) and check the rounding mode instead.

The parameter lists of tests/test_gpu_exact.py live here, so that tests/test_exact_reference.py (CPU) checks the two conditions on
exactly the cases the GPU file runs.
"""
import functools
import json
import os

import torch
import torch.nn.functional as F

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
MODES = [F32, BF16, F16]
TAG = {F32: "f32", BF16: "bf16", F16: "f16"}
ACC_STEPS = 2 ** 24                                   # integers up to 2^24 are float32 values
OUT_STEPS = {F32: 2 ** 24, BF16: 256, F16: 2048}      # integers up to 2^p are T values, p = significand bits of T
PM1 = (-1, 1)
PM2 = (-2, -1, 1, 2)
SCALES = (0.0, 0.5, 1.0, 2.0)                         # per-image DropPath scales: powers of two (and zero) keep the lattice
SLOPE = 0.01                                          # nn.LeakyReLU() default, a float32 constant in the kernels
SENTINEL = -12345.0

UF_ERR_SHAPE, UF_ERR_UNSUPPORTED, UF_ERR_ALIGN = -1, -2, -3


# ---------------------------------------------------------------------------------------------------------------------------
# lattice generators, the bound, the two conditions
# ---------------------------------------------------------------------------------------------------------------------------
def lattice(shape, values, seed, k=0):
    """float64 tensor drawn (seeded) from ``values`` * 2**-k.  No value is zero: a dropped or doubled term always moves a sum by at
    least one lattice step."""
    v = torch.tensor(values, dtype=torch.float64)
    assert bool((v != 0).all()), "lattice values must be non-zero"
    idx = torch.randint(len(values), tuple(shape), generator=torch.Generator().manual_seed(seed))
    return v[idx] * 2.0 ** -k


def max_partial_steps(K, a_values, b_values=(1,), addend_steps=0):
    """largest |partial sum|, in lattice steps, of K products of one value from each set (+ addends such as a bias or a residual)"""
    return K * max(abs(v) for v in a_values) * max(abs(v) for v in b_values) + addend_steps


def check_accumulation(K, a_values, b_values=(1,), addend_steps=0):
    """condition 1: float32 accumulation is exact in any order"""
    b = max_partial_steps(K, a_values, b_values, addend_steps)
    assert b < ACC_STEPS, f"partial sums of up to {b} lattice steps are not exact in float32"
    return b


def check_representable(ref64, dtype, step=1.0):
    """condition 2: every reference value is a T value (integers of at most OUT_STEPS[T] steps), so storing it as T rounds nothing"""
    m = float(ref64.abs().max()) / step
    assert m <= OUT_STEPS[dtype], f"reference reaches {m} lattice steps > {OUT_STEPS[dtype]} for {TAG[dtype]}"
    assert torch.equal(ref64.to(dtype).double(), ref64)
    return m


def act_values(K):
    """activation lattice of a T-output contraction of length K against PM1 weights: the richest set whose sums stay bf16 values
    ({-2,-1,1,2} reaches 188 at K = 512 but 386 at K = 2048; {-1,1} reaches 214 there)"""
    return PM2 if K <= 512 else PM1


# ---------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------
RECORDS = {}            # name -> {"elements": n, "differing": n}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def assert_exact(name, got, ref64, out_dtype, tile=(128, 64)):
    """``got`` (tensor of ``out_dtype``, any device) must hold the bits of ``ref64`` after the single allowed rounding to ``out_dtype``
    (``ref64`` may already be of ``out_dtype``: a reference that ends in float32 operations).  Records {elements, differing} under
    ``name`` ("entry_point/case") for the report, and on failure names the first differing element: flat index, and
    (tile, row, column) for ``tile`` = (rows, columns) of the kernel's block tile over the last two dimensions."""
    got = got.detach().cpu()
    assert got.dtype == out_dtype, f"{name}: output dtype {got.dtype}, expected {out_dtype}"
    want = ref64.detach().cpu().to(out_dtype)                   # round-to-nearest-even, once
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    gb, wb = _bits(got), _bits(want)
    diff = gb != wb
    n_diff = int(diff.sum())
    rec = RECORDS.setdefault(name, {"elements": 0, "differing": 0})
    rec["elements"] += got.numel()
    rec["differing"] += n_diff
    if torch.equal(gb, wb):
        return
    flat = int(diff.reshape(-1).nonzero()[0])
    cols = got.shape[-1] if got.dim() >= 2 else got.numel()
    r, c = divmod(flat, cols)
    tiles_n = (cols + tile[1] - 1) // tile[1]
    where = f"flat {flat} = tile {(r // tile[0]) * tiles_n + c // tile[1]} (tile row {r // tile[0]}, tile column {c // tile[1]}), row {r % tile[0]}, column {c % tile[1]}"
    raise AssertionError(f"{name}: {n_diff} of {got.numel()} elements differ from the float64 reference rounded to {TAG[out_dtype]}; first at {where}: "
                         f"got {float(got.reshape(-1)[flat])!r}, expected {float(want.reshape(-1)[flat])!r} (float64 {float(ref64.reshape(-1)[flat])!r})")


def report():
    """per-entry-point figures of the report: cases run, elements compared, elements differing"""
    out = {}
    for name, rec in sorted(RECORDS.items()):
        e = out.setdefault(name.split("/")[0], {"cases": 0, "elements": 0, "differing": 0})
        e["cases"] += 1
        e["elements"] += rec["elements"]
        e["differing"] += rec["differing"]
    return out


def dump_report(fname="parity_exact.json"):
    """writes report() to $UF_REPORT_DIR/parity_exact.json when that variable names a directory (as tests/test_gpu_edges.py does)"""
    out = os.environ.get("UF_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, fname), "w") as f:
            json.dump(report(), f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------------
def to_rows(x):
    """(B,C,H,W) -> token rows (B*H*W, C)"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def from_rows(r, B, H, W):
    return r.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def window_tokens(B, H, W, shift):
    """token index of every window-order row: torch.roll(-shift) + window_partition(8) of the raster order"""
    idx = torch.arange(B * H * W).reshape(B, H, W)
    idx = torch.roll(idx, shifts=(-shift, -shift), dims=(1, 2))
    return idx.reshape(B, H // 8, 8, W // 8, 8).permute(0, 1, 3, 2, 4).reshape(-1)


def leaky_f32(pre64):
    """LeakyReLU of an exact pre-activation as the kernels compute it: one float32 multiply by float32(0.01)"""
    a = pre64.float()
    assert torch.equal(a.double(), pre64)
    return torch.where(a > 0, a, a * torch.tensor(SLOPE, dtype=torch.float32))


def rpb_index(win):
    """relative_position_index of a win x win window: entry (dy + win - 1) * (2 win - 1) + dx + win - 1, (dy, dx) = query - key"""
    c = torch.arange(win)
    ys, xs = (t.reshape(-1) for t in torch.meshgrid(c, c, indexing="ij"))
    return (ys[:, None] - ys[None, :] + win - 1) * (2 * win - 1) + (xs[:, None] - xs[None, :] + win - 1)


# ---------------------------------------------------------------------------------------------------------------------------
# parameter lists (shared by the CPU and the GPU file) and float64 references
# ---------------------------------------------------------------------------------------------------------------------------
GEMM_M = [64, 130, 1000]
GEMM_N = [32, 96, 192]
GEMM_K = [16, 32, 96, 128, 512, 2048]
GEMM_CASES = [(M, N, K) for M in GEMM_M for N in GEMM_N for K in GEMM_K]
# images of the residual GEMM: plain rows (B, H, W) with B * H * W = M; windowed maps of whole 8 x 8 windows on the first M // 64 * 64 rows
RES_PLAIN = {64: (2, 4, 8), 130: (2, 5, 13), 1000: (4, 10, 25)}
RES_WINDOWED = {64: (1, 8, 8), 130: (2, 8, 8), 1000: (3, 8, 40)}
# (M, C, heads): head widths 16, 32, 64; M = 192 is two row tiles with a half-filled second one (uf_qkv_fwd takes whole 64-token windows only)
QKV_CASES = [(M, C, C // hd) for M in (64, 192) for hd in (16, 32, 64) for C in (16, 32, 96, 128, 512) if C % hd == 0 and (M == 64 or C <= 128)]
QKV_CASES.append((64, 2048, 32))
QKV_REJECTED_M = [130, 1000]
# one 128-row x 128-column tile configuration of the dense GEMM is chosen only from 512 such tiles on (launch_bn in csrc/uf_gemm.hip); uf_qkv_fwd always
# takes it, uf_linear_fwd only at a case of this size: 33 row tiles (the last one 4 rows) x 16 column tiles, two K tiles (both staging paths)
GEMM_WIDE_TILE_CASE = (4100, 2048, 128)


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K):
    """operands and float64 product of one dense GEMM case: A (M,K), W (N,K), bias (N), P = A W^T + bias"""
    av = act_values(K)
    A, W, b = lattice((M, K), av, 1000 + K + M), lattice((N, K), PM1, 2000 + K + N), lattice((N,), PM1, 3000 + N)
    bound = check_accumulation(K, av, PM1, addend_steps=1)
    return {"A": A, "W": W, "bias": b, "P": A @ W.t() + b, "bound": bound, "values": av}


def rounding_values(dtype):
    """lattice of a rounding case: 1, 3 and a quarter of the first integer spacing change of T -- a few terms reach past 2^p, where T holds
    only every second, fourth, ... integer (bf16: 257 -> 256 and 259 -> 260 under round-to-nearest-even; truncation gives 256 and 258)"""
    q = OUT_STEPS[dtype] // 4
    return (-q, -3, -1, 1, 3, q)


def cast_rounding_values(dtype):
    """values of an f32 -> T cast that T cannot hold: 2^p + 1 is a tie (to 2^p, the even neighbour), 2^p + 3 a tie that goes away from zero"""
    p = OUT_STEPS[dtype]
    return (-p - 3, -p - 1, -1, 1, p + 1, p + 3)


def rounding_profile(ref64, dtype):
    """what a rounding case must contain to tell the modes apart: values T cannot hold, some rounded AWAY from zero (truncation differs there)
    and some exact ties (round-half-away differs from round-half-even there)"""
    r = ref64.to(dtype).double()
    inexact = r != ref64
    away = r.abs() > ref64.abs()
    up, dn = torch.nextafter(r.to(dtype), torch.tensor(float("inf"), dtype=dtype)).double(), torch.nextafter(r.to(dtype), torch.tensor(float("-inf"), dtype=dtype)).double()
    tie = inexact & (((ref64 - r).abs() == (up - ref64).abs()) | ((ref64 - r).abs() == (ref64 - dn).abs()))
    return {"inexact": int(inexact.sum()), "away": int(away.sum()), "ties": int(tie.sum())}


@functools.lru_cache(maxsize=None)
def gemm_rounding_case(dtype, M=64, N=32, K=64):
    """a product whose float64 results exceed 2^p on purpose (condition 1 still holds): the store's rounding mode decides the bits"""
    rv = rounding_values(dtype)
    A, W, b = lattice((M, K), PM1, 91 + K), lattice((N, K), rv, 92 + N), lattice((N,), PM1, 93)
    return {"A": A, "W": W, "bias": b, "P": A @ W.t() + b, "bound": check_accumulation(K, PM1, rv, addend_steps=1)}


def ref_qkv(P, M, C, heads):
    """q | k | v^T in the layouts uf_qkv_fwd writes, from the float64 projection P (M, 3C); q is multiplied by float32(hd ** -0.5) in
    float32 (one IEEE multiply, then the store's rounding), which is exact for head widths 16 and 64"""
    hd = C // heads
    qs = torch.tensor(float(hd) ** -0.5, dtype=torch.float32)
    Pf = P.float()
    assert torch.equal(Pf.double(), P)
    q = (Pf[:, :C] * qs).reshape(M // 64, 64, heads, hd).permute(0, 2, 1, 3).contiguous()
    k = P[:, C:2 * C].reshape(M // 64, 64, heads, hd).permute(0, 2, 1, 3).contiguous()
    vt = P[:, 2 * C:].reshape(M // 64, 64, heads, hd).permute(0, 2, 3, 1).contiguous()
    return q, k, vt


def ref_residual(P, resid, scale, B, H, W, tokens=None):
    """out[tok] = resid[tok] + scale[image of tok] * P[row], tok = tokens[row] (window order) or row"""
    M = B * H * W
    tok = torch.arange(M) if tokens is None else tokens
    out = resid.clone()
    s = torch.ones(B, dtype=torch.float64) if scale is None else scale
    out[tok] = resid[tok] + s[tok // (H * W)][:, None] * P[:M]
    return out


# samplers, stem and head
SAMPLER_MAPS = [(8, 8), (16, 24), (8, 40)]
SAMPLER_C = [16, 32, 64, 256]
SAMPLER_B = [1, 3]
STEM_MAPS = SAMPLER_MAPS + [(13, 70)]
# uf_output_proj_fwd takes the width of the decoder's last stage, 2 E: every width it supports (16 has an instantiation of its own), and the
# first two it must reject
HEAD_C = [16, 32, 64, 128]
HEAD_C_REJECTED = [256, 512]
# the second form of Downsample (2-byte types, whole tiles of 8 x 16 / 4 x 16 / 4 x 8 output pixels) needs larger maps than the list above
DOWN_PATCH_CASES = [(1, 16, 32, 32), (2, 16, 32, 64), (1, 8, 32, 128), (1, 8, 16, 256)]


@functools.lru_cache(maxsize=None)
def sampler_case(B, H, W, C):
    x = lattice((B, C, H, W), PM2, 11 + C + H)
    wd, bd = lattice((2 * C, C, 4, 4), PM1, 12 + C), lattice((2 * C,), PM2, 13 + C)
    wu, bu = lattice((C, C // 2, 2, 2), PM1, 14 + C), lattice((C // 2,), PM2, 15 + C)
    check_accumulation(16 * C, PM2, PM1, addend_steps=2)
    return {"x": x, "wd": wd, "bd": bd, "down": F.conv2d(x, wd, bd, stride=2, padding=1), "wu": wu, "bu": bu, "up": F.conv_transpose2d(x, wu, bu, stride=2)}


@functools.lru_cache(maxsize=None)
def stem_case(B, H, W, E):
    img = lattice((B, 3, H, W), PM2, 21 + H, k=2)
    w_in, b_in = lattice((E, 3, 3, 3), PM2, 22 + E), lattice((E,), PM1, 23 + E)
    check_accumulation(27, PM2, PM2, addend_steps=4)            # in steps of 1/4
    return {"img": img, "w_in": w_in, "b_in": b_in, "stem": leaky_f32(F.conv2d(img, w_in, b_in, padding=1))}


@functools.lru_cache(maxsize=None)
def head_case(B, H, W, C2):
    img = lattice((B, 3, H, W), PM2, 21 + H, k=2)
    x = lattice((B, C2, H, W), PM2, 24 + C2 + W)
    w_out, b_out = lattice((3, C2, 3, 3), PM1, 25 + C2), lattice((3,), PM2, 26)
    check_accumulation(9 * C2, PM2, PM1, addend_steps=4 * 4)    # in steps of 1/4 (the image)
    head = F.conv2d(x, w_out, b_out, padding=1)
    return {"img": img, "x": x, "w_out": w_out, "b_out": b_out, "head": head, "head_img": head + img}


# depthwise stencil: (B, H, W, C); the last two leave the issue's list: W = 12 and 6 are not multiples of 8, which sends the launch to the
# strip kernel instead of the walking one (launch_dwconv in csrc/uf_elementwise.hip)
DWCONV_CASES = [(2, 16, 16, 64), (1, 8, 24, 128), (1, 40, 40, 16), (3, 8, 8, 512), (2, 4, 12, 16), (1, 8, 6, 32)]


@functools.lru_cache(maxsize=None)
def dwconv_case(B, H, W, C):
    x, w, b = lattice((B, C, H, W), PM2, 31 + C), lattice((C, 1, 3, 3), PM2, 32 + C, k=1), lattice((C,), PM1, 33 + C)
    dc = lattice((B, C, H, W), PM1, 34 + C)
    check_accumulation(9, PM2, PM2, addend_steps=2)             # steps of 1/2
    xp = F.pad(x, (1, 1, 1, 1))
    dw9 = torch.stack([(dc * xp[:, :, ky:ky + H, kx:kx + W]).sum((0, 2, 3)) for ky in range(3) for kx in range(3)])      # (9, C) tap-major
    check_accumulation(B * H * W, PM2, PM1)
    return {"x": x, "w": w, "bias": b, "plain": F.conv2d(x, w, None, padding=1, groups=C), "biased": F.conv2d(x, w, b, padding=1, groups=C),
            "dc": dc, "dw9": dw9, "dbias": dc.sum((0, 2, 3))}


# UNet implicit GEMMs
CONV_PAIRS = [(16, 16), (32, 64), (64, 96), (96, 32), (256, 128), (512, 512)]
CONV3_MAPS = [(17, 23), (16, 16), (6, 10)]
CONV4_MAPS = [(24, 40), (10, 6)]
CONV1_MAP = (10, 14)
CONV_B = [1, 3]


# the tile of 128 output pixels is 8 x 16, 16 x 8 or 32 x 4, the widest the output map fills (launch_conv_t in csrc/uf_conv.hip).  The maps above give the
# 3x3 kernel the first two, the 4x4 stride-2 kernel the first and the last and the 1x1 kernel the second only: (cin, cout, H, W) for the rest
CONV3_NARROW = [(32, 64, 8, 4), (96, 32, 4, 4), (16, 16, 33, 5)]
CONV1_OTHER = [(32, 64, 5, 20), (64, 96, 9, 4), (16, 16, 33, 3)]


def conv3_maps(cin, cout):
    return [(6, 10)] if (cin, cout) == (512, 512) else CONV3_MAPS


def conv3_cases():
    return [(ci, co, H, W, B) for (ci, co) in CONV_PAIRS for (H, W) in conv3_maps(ci, co) for B in CONV_B] + [c + (B,) for c in CONV3_NARROW for B in CONV_B]


def conv41_cases(cin, cout):
    """(k, H, W, B) of uf_conv4s2_fwd and uf_conv1x1_fwd for one channel pair"""
    maps = [(4, m) for m in CONV4_MAPS] + [(1, CONV1_MAP)] + [(1, (H, W)) for (ci, co, H, W) in CONV1_OTHER if (ci, co) == (cin, cout)]
    return [(k, H, W, B) for (k, (H, W)) in maps for B in CONV_B]


@functools.lru_cache(maxsize=None)
def conv_case(k, B, H, W, cin, cout):
    """k = 3: conv3x3 with every epilogue; k = 4: stride 2; k = 1.  aux / prev rows are integer lattices as well."""
    x = lattice((B, cin, H, W), PM2, 41 + cin + H + k)
    w, b = lattice((cout, cin, k, k), PM1, 42 + cin + cout + k), lattice((cout,), PM2, 43 + cout)
    check_accumulation(k * k * cin, PM2, PM1, addend_steps=2 + 4 + 4)
    d = {"x": x, "w": w, "bias": b}
    if k == 3:
        pre = F.conv2d(x, w, b, padding=1)
        aux, prev = lattice((B, cout, H, W), PM2, 44 + cout), lattice((B, cout, H, W), PM2, 45 + cout)
        lr = leaky_f32(pre)
        d.update(pre=pre, aux=aux, prev=prev, lrelu=lr, lrelu_aux=lr + aux.float(), lrelu_aux_acc=(lr + aux.float()) + prev.float(),
                 pre_acc=pre + prev, lrelu_acc=lr + prev.float())
        # input gradient of a conv cin -> cout: dy (B, cout) -> (B, cin), times LeakyReLU'(a) taken from the sign of the stored output a
        dy, a = lattice((B, cout, H, W), PM2, 46 + cout), lattice((B, cin, H, W), PM2, 47 + cin)
        g = F.conv_transpose2d(dy, w, padding=1).float()
        prev_in = lattice((B, cin, H, W), PM2, 48 + cin)
        dg = g * torch.where(a > 0, torch.tensor(1.0), torch.tensor(SLOPE, dtype=torch.float32))
        d.update(dy=dy, a=a, prev_in=prev_in, dgrad=dg, dgrad_acc=dg + prev_in.float())
    elif k == 4:
        d["out"] = F.conv2d(x, w, b, stride=2, padding=1)
    else:
        d["out"] = F.conv2d(x, w, b)
    return d


IM2COL_CASES = [  # (k, stride, pad, nchw, B, H, W, Cin)
    (4, 2, 1, 0, 2, 8, 12, 16), (2, 2, 0, 0, 2, 8, 12, 32), (3, 1, 1, 0, 1, 7, 9, 8), (3, 1, 1, 1, 2, 7, 9, 3), (4, 2, 1, 0, 1, 6, 10, 4)]


def ref_im2col(x, k, stride, pad):
    """(B,C,H,W) -> (B*Ho*Wo, k*k*C) with column (ky*k + kx)*C + c"""
    B, C = x.shape[:2]
    u = F.unfold(x, k, padding=pad, stride=stride)                    # (B, C*k*k, L), rows (c, ky, kx)
    return u.reshape(B, C, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * C)


def ref_col2im(cols, B, H, W, C, k, stride, pad):
    u = cols.reshape(B, -1, k * k, C).permute(0, 3, 2, 1).reshape(B, C * k * k, -1)
    return F.fold(u, (H, W), k, padding=pad, stride=stride)           # (B,C,H,W)


# backward contractions and reductions
WGRAD_M = [64, 130, 4096]
WGRAD_CASES = [(M, N, K) for M in WGRAD_M for N in GEMM_N for K in GEMM_K if K <= 512]


@functools.lru_cache(maxsize=None)
def wgrad_case(M, N, K):
    dy, x = lattice((M, N), PM2, 51 + M + N), lattice((M, K), PM1, 52 + M + K)
    check_accumulation(M, PM2, PM1)
    return {"dy": dy, "x": x, "dW": dy.t() @ x, "db": dy.sum(0)}


CONV3_BWD_CASES = [  # (nchw, B, H, W, Cin, Cout, masked)
    (0, 2, 8, 16, 32, 3, 0), (0, 1, 7, 9, 64, 3, 0), (1, 2, 8, 16, 3, 32, 0), (1, 2, 8, 16, 3, 32, 1), (1, 1, 7, 9, 3, 16, 1), (1, 1, 5, 6, 3, 64, 1)]
CONV3_BWD_SLOPE = 0.5          # the slope is an argument of uf_conv3x3_bwd: a power of two keeps dy * slope on the lattice (0.01 does not)


@functools.lru_cache(maxsize=None)
def conv3_bwd_case(nchw, B, H, W, cin, cout, masked):
    x, w, dy = lattice((B, cin, H, W), PM2, 61 + cin), lattice((cout, cin, 3, 3), PM1, 62 + cout), lattice((B, cout, H, W), PM2, 63 + cout)
    act = lattice((B, cout, H, W), PM2, 64 + cout)
    dyeff = dy * torch.where(act > 0, 1.0, CONV3_BWD_SLOPE) if masked else dy
    check_accumulation(max(9 * cout, B * H * W), PM2, PM2)      # steps of 1/2
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wr, br, padding=1).backward(dyeff)
    return {"x": x, "w": w, "dy": dy, "act": act, "dx": xr.grad, "dW": wr.grad, "db": br.grad}


# (B, H, W, Cin): (1, 16, 32, 32) and (4, 8, 32, 128) take the LDS-patch form of the input gradient in the 2-byte types (whole 8 x 16 / 4 x 16 tiles of output
# pixels and at least Cout of them), the others the patch-matrix route
DOWN_BWD_CASES = [(2, 8, 8, 32), (1, 16, 32, 32), (1, 8, 24, 16), (4, 8, 32, 128), (2, 4, 4, 256)]


@functools.lru_cache(maxsize=None)
def down_bwd_case(B, H, W, cin):
    cout = 2 * cin
    x, w, dy = lattice((B, cin, H, W), PM2, 71 + cin), lattice((cout, cin, 4, 4), PM1, 72 + cin), lattice((B, cout, H // 2, W // 2), PM1, 73 + cin)
    base = lattice((B, cin, H, W), PM2, 74 + cin)
    check_accumulation(max(16 * cout, B * H * W), PM2, PM1, addend_steps=2)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wr, br, stride=2, padding=1).backward(dy)
    # the input gradient is stored as T TAP BY TAP before the taps are added (csrc/uf_trainblk.hip: uf_linear_fwd rounds the patch matrix, down_dx_kernel
    # rounds every tap's accumulator): condition 2 applies to the patch matrix dy W
    taps = to_rows(dy) @ w.permute(0, 2, 3, 1).reshape(cout, -1)
    return {"x": x, "w": w, "dy": dy, "base": base, "dx": xr.grad, "dW": wr.grad, "db": br.grad, "taps": taps}


UP_BWD_CASES = [(2, 8, 8, 64, 32), (1, 4, 12, 512, 256), (3, 4, 4, 32, 16)]      # (B, H, W, Cin, Cout)


@functools.lru_cache(maxsize=None)
def up_bwd_case(B, H, W, cin, cout):
    x, w, d = lattice((B, cin, H, W), PM1, 81 + cin), lattice((cin, cout, 2, 2), PM1, 82 + cin), lattice((B, cout, 2 * H, 2 * W), PM1, 83 + cout)
    check_accumulation(max(4 * cout, 4 * B * H * W), PM1, PM1)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(xr, wr, br, stride=2).backward(d)
    return {"x": x, "w": w, "d": d, "dx": xr.grad, "dW": wr.grad, "db": br.grad}     # dx is stored as T before it is widened: condition 2 applies to it


STREAM_CASES = [(2, 8, 8, 32, 0, 0), (2, 8, 8, 32, 1, 0), (3, 16, 24, 64, 1, 4), (4, 5, 13, 16, 0, 0), (4, 8, 40, 256, 1, 4)]     # (B, H, W, C, windowed, shift)
MERGE_CASES = [(2, 1), (3, 4), (13, 8)]                                                                                         # (n_windows, heads), head width 32
RPB_HEADS = [1, 4, 8]
RPB4_CASES = [(1, 1), (6, 2), (37, 4)]                                                                                          # (n_windows, heads)
ROWS_SUM_CASES = [(4, 32), (130, 96), (1000, 192), (64, 2048)]


def largest_contraction():
    """the longest contraction (K) and the longest reduction (rows / pixels summed by a gradient) among the cases above"""
    ks = [K for (_, _, K) in GEMM_CASES + [GEMM_WIDE_TILE_CASE]] + [C for (_, C, _) in QKV_CASES] + [16 * C for C in SAMPLER_C] + [16 * c[3] for c in DOWN_PATCH_CASES]
    ks += [9 * C for C in HEAD_C] + [9 * max(ci, co) for (ci, co) in CONV_PAIRS] + [k * k * ci for (ci, co) in CONV_PAIRS for k in (4, 1)]
    ks += [9 * co for (_, _, _, _, _, co, _) in CONV3_BWD_CASES] + [32 * c[3] for c in DOWN_BWD_CASES] + [4 * c[4] for c in UP_BWD_CASES]
    rs = [M for (M, _, _) in WGRAD_CASES] + [M for (M, _) in ROWS_SUM_CASES] + [B * H * W for (B, H, W, _) in DWCONV_CASES + DOWN_BWD_CASES]
    rs += [4 * B * H * W for (B, H, W, _, _) in UP_BWD_CASES] + [c[1] * c[2] * c[3] for c in CONV3_BWD_CASES] + [16 * n for (n, _) in RPB4_CASES]
    return max(ks), max(rs)


LARGEST_K, LARGEST_REDUCTION = largest_contraction()
