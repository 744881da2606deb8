"""Thin torch-tensor wrappers over the C ABI (``include/uformer_hip.h``).

PyTorch is plumbing here: it owns device memory and the HIP stream; every wrapper hands its tensors to ``_launch``, which
extracts the raw pointers and calls ``libuformer_hip.so``.  No op has a CPU or eager fallback -- CPU tensors
raise.  Names follow the reference functions they replace (model.py:704-726 etc.).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import UF_BF16, UF_F16, UF_F32, UformerHipError

Tensor = torch.Tensor


def uf_dtype(dtype) -> int:
    if dtype in (UF_F32, UF_BF16, UF_F16) and not isinstance(dtype, torch.dtype):
        return int(dtype)
    if dtype == torch.float32:
        return UF_F32
    if dtype == torch.bfloat16:
        return UF_BF16
    if dtype == torch.float16:
        return UF_F16
    raise UformerHipError(f"unsupported operand dtype {dtype} (torch.float32, torch.bfloat16 or torch.float16)")


def torch_dtype(dt: int) -> torch.dtype:
    return {UF_BF16: torch.bfloat16, UF_F16: torch.float16}.get(dt, torch.float32)


def _dev(*ts: Tensor) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise UformerHipError("uformer_amd ops run on the GPU only (tensor is on %s); there is no CPU path" % t.device)
        if dev is not None and t.device != dev:
            raise UformerHipError("tensors on different devices")
        dev = t.device
    return dev


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _launch(name: str, dev, *args) -> None:
    """Call entry point ``name`` on ``dev``'s current stream: a Tensor argument goes as its address (None as NULL), anything else as it
    is, the stream last.  ``args`` holds every tensor until the call has returned, so a wrapper may build a converted operand
    (``_c``, ``_f32``, ``_pack_frag``) right in the argument list; it never takes an address itself."""
    with torch.cuda.device(dev):
        # hasattr, not isinstance: half the cost per scalar argument, and a step makes several hundred launches
        rc = getattr(_lib.load(), name)(*[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args], _stream())
    _lib.check(rc, name)


def _pack_frag(w: Tensor) -> Tensor:
    """Row-major nn.Linear weight -> the fragment-major layout the fused kernels stream (uf_pack_weight_fm)."""
    _dev(w)
    w = _c(w)
    N, K = w.shape
    out = torch.empty(_lib.load().uf_weight_fm_elems(N, K), dtype=w.dtype, device=w.device)
    _launch("uf_pack_weight_fm", w.device, w, out, N, K, uf_dtype(w.dtype))
    return out


def _c(t: Tensor, dtype: Optional[torch.dtype] = None) -> Tensor:
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()


def _f32(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else _c(t, torch.float32)


def _ws(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _workspace(query: str, device, *dims) -> Tuple[Tensor, int]:
    """(workspace tensor, its size in bytes as the entry point wants it) from the size query ``query(*dims)``; ``*_workspace(...)``
    fills the two C arguments."""
    nbytes = getattr(_lib.load(), query)(*dims)
    return _ws(nbytes, device), nbytes


# ---------------------------------------------------------------------------------------
# a1-a4 index ops
# ---------------------------------------------------------------------------------------
def window_partition(x: Tensor, win_size: int = 8, shift: int = 0) -> Tensor:
    """(B,H,W,C) -> (B*nW, 8, 8, C).  model.py:704-715; ``shift`` folds torch.roll (:957).  ``win_size`` 4 (no shift): the
    4x4 windows of a bottleneck built for 64x64 patches."""
    if win_size == 4 and shift == 0:
        return _window4_copy(x, reverse=False)
    if win_size != 8:
        raise UformerHipError("win_size must be 8 (or 4 without a shift)")
    _dev(x)
    B, H, W, Cc = x.shape
    x = _c(x)
    if x.element_size() not in (2, 4):
        raise UformerHipError("window ops support 2- and 4-byte elements")
    out = torch.empty((B * (H // 8) * (W // 8), 8, 8, Cc), dtype=x.dtype, device=x.device)
    _launch("uf_window_partition", x.device, x, out, B, H, W, Cc, shift, x.element_size())
    return out


def window_reverse(windows: Tensor, win_size: int, H: int, W: int, shift: int = 0) -> Tensor:
    """(B*nW, 8, 8, C) -> (B,H,W,C).  model.py:717-726; ``shift`` folds the roll back (:980).  ``win_size`` 4: see window_partition."""
    if win_size == 4 and shift == 0:
        return _window4_copy(windows, reverse=True, H=H, W=W)
    if win_size != 8:
        raise UformerHipError("win_size must be 8 (or 4 without a shift)")
    _dev(windows)
    windows = _c(windows)
    Cc = windows.shape[-1]
    nW = (H // 8) * (W // 8)
    B = windows.shape[0] // nW
    out = torch.empty((B, H, W, Cc), dtype=windows.dtype, device=windows.device)
    _launch("uf_window_reverse", windows.device, windows, out, B, H, W, Cc, shift, windows.element_size())
    return out


def _window4_copy(x: Tensor, reverse: bool, H: int = 0, W: int = 0) -> Tensor:
    """uf_window4_partition ((B,H,W,C) -> (B*nW,4,4,C)) or uf_window4_reverse ((B*nW,4,4,C) -> (B,H,W,C))."""
    _dev(x)
    x = _c(x)
    if x.element_size() not in (2, 4):
        raise UformerHipError("window ops support 2- and 4-byte elements")
    Cc = x.shape[-1]
    if reverse:
        nW = (H // 4) * (W // 4)
        if nW == 0 or H % 4 or W % 4 or x.shape[0] % nW:
            raise UformerHipError(f"window_reverse at 4: H={H} W={W} do not tile {tuple(x.shape)}")
        B = x.shape[0] // nW
        out = torch.empty((B, H, W, Cc), dtype=x.dtype, device=x.device)
        fn = "uf_window4_reverse"
    else:
        B, H, W, _ = x.shape
        out = torch.empty((B * (H // 4) * (W // 4), 4, 4, Cc), dtype=x.dtype, device=x.device)
        fn = "uf_window4_partition"
    _launch(fn, x.device, x, out, B, H, W, Cc, x.element_size())
    return out


def window4_attention(qkv: Tensor, rpb4: Tensor, B: int, H: int, W: int, heads: int) -> Tensor:
    """4x4-window attention on raster rows: qkv T (B*H*W, 3C) = the q|k|v projection outputs (unscaled), rpb4 f32 (heads, 49)
    (packing.pack_rpb_table4) -> o T (B*H*W, C), heads merged.  model.py:494-519 at win 4, no mask."""
    _dev(qkv, rpb4)
    qkv = _c(qkv)
    M, C3 = qkv.shape
    C = C3 // 3
    if M != B * H * W or C3 != 3 * C:
        raise UformerHipError(f"window4_attention: qkv {tuple(qkv.shape)} does not match B*H*W = {B * H * W}")
    out = torch.empty(M, C, dtype=qkv.dtype, device=qkv.device)
    _launch("uf_window4_attention_fwd", qkv.device, qkv, C3, _f32(rpb4), out, C, B, H, W, C, heads, uf_dtype(qkv.dtype))
    return out


def window4_attention_bwd(qkv: Tensor, rpb4: Tensor, do: Tensor, B: int, H: int, W: int, heads: int) -> Tuple[Tensor, Tensor]:
    """Backward of window4_attention: (dqkv T (B*H*W, 3C), dscore f32 (n_windows, heads, 16, 16))."""
    _dev(qkv, rpb4, do)
    qkv = _c(qkv)
    do = _c(do, qkv.dtype)
    M, C3 = qkv.shape
    C = C3 // 3
    if M != B * H * W or do.shape != (M, C):
        raise UformerHipError(f"window4_attention_bwd: qkv {tuple(qkv.shape)} / do {tuple(do.shape)} do not match B*H*W = {B * H * W}")
    dqkv = torch.empty_like(qkv)
    dscore = torch.empty(B * (H // 4) * (W // 4), heads, 16, 16, dtype=torch.float32, device=qkv.device)
    _launch("uf_window4_attention_bwd", qkv.device, qkv, C3, _f32(rpb4), do, C, dqkv, C3, dscore, B, H, W, C, heads, uf_dtype(qkv.dtype))
    return dqkv, dscore


def rpb4_table_grad(dscore: Tensor) -> Tensor:
    """(n_windows, heads, 16, 16) score gradient -> (49, heads) relative_position_bias_table gradient of a 4x4-window block."""
    _dev(dscore)
    dscore = _c(dscore, torch.float32)
    nW, heads = dscore.shape[0], dscore.shape[1]
    out = torch.empty(49, heads, dtype=torch.float32, device=dscore.device)
    _launch("uf_rpb4_table_grad", dscore.device, dscore, out, nW, heads)
    return out


def shift_mask(H: int, W: int, shift: int, device) -> Tensor:
    """SW-MSA mask (nW,64,64) in {0,-100}.  model.py:924-942."""
    out = torch.empty(((H // 8) * (W // 8), 64, 64), dtype=torch.float32, device=device)
    _launch("uf_shift_mask", out.device, out, H, W, shift)
    return out


# ---------------------------------------------------------------------------------------
# float ops
# ---------------------------------------------------------------------------------------
def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, *, B: int, H: int, W: int, dtype, windowed: bool = False,
              shift: int = 0, modulator: Optional[Tensor] = None) -> Tensor:
    """x f32 (B*H*W, C) rows -> T (rows, C); optionally roll+partition+modulator (model.py:952-969)."""
    _dev(x, gamma, beta, modulator)
    dt = uf_dtype(dtype)
    x = _c(x, torch.float32)
    Cc = x.shape[-1]
    out = torch.empty((B * H * W, Cc), dtype=torch_dtype(dt), device=x.device)
    _launch("uf_layernorm_fwd", x.device, x, Cc, _f32(gamma), _f32(beta), _f32(modulator), out, B, H, W, Cc, int(windowed), shift, dt)
    return out


def linear(a: Tensor, w: Tensor, bias: Tensor, act: int = 0) -> Tensor:
    """out = act(a @ w.T + bias); a T(M,K), w T(N,K) -- nn.Linear (model.py:426-427,489,657,661)."""
    _dev(a, w, bias)
    dt = uf_dtype(a.dtype)
    a, w = _c(a), _c(w, a.dtype)
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    _launch("uf_linear_fwd", a.device, a, w, _f32(bias), out, M, N, K, act, dt)
    return out


def linear_residual(a: Tensor, w: Tensor, bias: Tensor, resid: Tensor, scale: Optional[Tensor], B: int, H: int, W: int, windowed: bool = False,
                    shift: int = 0) -> Tensor:
    """resid + scale[image] * (a @ w.T + bias) as f32 (B*H*W, N) raster rows; ``a`` in window-row order when ``windowed`` (window_reverse and
    the roll back happen in the store).  The projection / linear2 of a block with its residual add and DropPath (model.py:975-987)."""
    _dev(a, w, bias, resid)
    dt = uf_dtype(a.dtype)
    a, w, resid = _c(a), _c(w, a.dtype), _c(resid, torch.float32)
    M, K = a.shape
    N = w.shape[0]
    if M != B * H * W or resid.numel() != M * N:
        raise UformerHipError(f"linear_residual: a {tuple(a.shape)} / resid {tuple(resid.shape)} do not match B*H*W = {B * H * W}, N = {N}")
    sc = _f32(scale)
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _launch("uf_linear_residual_fwd", a.device, a, w, _f32(bias), resid, out, sc, B, H, W, N, K, int(windowed), shift, dt)
    return out


def qkv(a: Tensor, wqkv: Tensor, bqkv: Tensor, heads: int):
    """LinearProjection.forward (model.py:431-442) -> q (scaled), k, v^T per (window, head)."""
    _dev(a, wqkv, bqkv)
    dt = uf_dtype(a.dtype)
    a, wqkv = _c(a), _c(wqkv, a.dtype)
    M, Cc = a.shape
    hd = Cc // heads
    q = torch.empty((M // 64, heads, 64, hd), dtype=a.dtype, device=a.device)
    k = torch.empty_like(q)
    vt = torch.empty((M // 64, heads, hd, 64), dtype=a.dtype, device=a.device)
    _launch("uf_qkv_fwd", a.device, a, wqkv, _f32(bqkv), q, k, vt, M, Cc, heads, dt)
    return q, k, vt


def ln_qkv(x: Tensor, gamma: Tensor, beta: Tensor, wqkv: Tensor, bqkv: Tensor, heads: int, *, B: int, H: int, W: int,
           shift: int = 0, modulator: Optional[Tensor] = None):
    """Fused LN1 -> roll -> partition -> +modulator -> q,k,v^T (model.py:952-969, :431-442).  x f32 (B*H*W, C)."""
    _dev(x, gamma, beta, wqkv, bqkv, modulator)
    dt = uf_dtype(wqkv.dtype)
    x = _c(x, torch.float32)
    M, Cc = x.shape
    hd = Cc // heads
    q = torch.empty((M // 64, heads, 64, hd), dtype=wqkv.dtype, device=x.device)
    k = torch.empty_like(q)
    vt = torch.empty((M // 64, heads, hd, 64), dtype=wqkv.dtype, device=x.device)
    _launch("uf_ln_qkv_fwd", x.device, x, Cc, _f32(gamma), _f32(beta), _f32(modulator), _pack_frag(wqkv), _f32(bqkv), q, k, vt,
            B, H, W, Cc, heads, shift, dt)
    return q, k, vt


def ln_conv_qkv(x: Tensor, gamma: Tensor, beta: Tensor, dw9: Tensor, bdw: Tensor, wpw: Tensor, bpw: Tensor, heads: int, *, B: int, H: int, W: int,
                shift: int = 0, modulator: Optional[Tensor] = None, C: Optional[int] = None):
    """Fused LN1 -> roll -> partition -> +modulator -> ConvProjection (model.py:952-969, :381-410): per 8x8 window and for each of q, k, v a
    depthwise 3x3 (zero padding at the WINDOW border) + bias + ReLU, then the pointwise 1x1 + bias; q (scaled), k, v^T as ``ln_qkv``
    (uf_ln_convqkv_fwd).  x f32 (B*H*W, ld) contiguous with the channels in columns [0, C) (``C`` default: ld); dw9 f32 (3, 9, C) tap-major and
    bdw f32 (3, C) for q | k | v (packing.pack_conv_projection); wpw T (3C, C) row-major (packed fragment-major here); bpw f32 (3C,)."""
    _dev(x, gamma, beta, dw9, bdw, wpw, bpw, modulator)
    dt = uf_dtype(wpw.dtype)
    x = _c(x, torch.float32)
    M, ld = x.shape
    Cc = ld if C is None else int(C)
    if tuple(wpw.shape) != (3 * Cc, Cc) or tuple(dw9.shape) != (3, 9, Cc) or tuple(bdw.shape) != (3, Cc) or bpw.numel() != 3 * Cc:
        raise UformerHipError(f"ln_conv_qkv: dw9 {tuple(dw9.shape)} / bdw {tuple(bdw.shape)} / wpw {tuple(wpw.shape)} / bpw {tuple(bpw.shape)} "
                              f"do not match C = {Cc}")
    hd = Cc // heads
    q = torch.empty((M // 64, heads, 64, hd), dtype=wpw.dtype, device=x.device)
    k = torch.empty_like(q)
    vt = torch.empty((M // 64, heads, hd, 64), dtype=wpw.dtype, device=x.device)
    _launch("uf_ln_convqkv_fwd", x.device, x, ld, _f32(gamma), _f32(beta), _f32(modulator), _f32(dw9), _f32(bdw), _pack_frag(wpw), _f32(bpw),
            q, k, vt, B, H, W, Cc, heads, shift, dt)
    return q, k, vt


def ln_linear_gelu(x: Tensor, gamma: Tensor, beta: Tensor, w1: Tensor, b1: Tensor) -> Tensor:
    """Fused LN2 -> linear1 -> GELU (model.py:987, :657-658).  x f32 (M, C); w1 T (N, C) -> T (M, N)."""
    _dev(x, gamma, beta, w1, b1)
    dt = uf_dtype(w1.dtype)
    x = _c(x, torch.float32)
    M, Cc = x.shape
    N = w1.shape[0]
    out = torch.empty((M, N), dtype=w1.dtype, device=x.device)
    _launch("uf_ln_linear_gelu_fwd", x.device, x, Cc, _f32(gamma), _f32(beta), _pack_frag(w1), _f32(b1), out, M, N, Cc, dt)
    return out


def ffn(x: Tensor, gamma: Tensor, beta: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, scale: Optional[Tensor] = None, B: int = 1,
        C: Optional[int] = None) -> Tensor:
    """The fused Mlp half of a block, IN PLACE on ``x``: x[m, :C] += scale[image of m] * (GELU(LN2(x[m, :C]) w1^T + b1) w2^T + b2)  (model.py:623-642,
    :987; uf_ffn_fwd).  x f32 (M, ld) contiguous rows on the GPU with the channels in columns [0, C) (``C`` default: ld); w1 T (4C, C), w2 T (C, 4C)
    row-major (packed fragment-major here); scale f32 (B,) per-image DropPath scales or None.  Returns x."""
    _dev(x, gamma, beta, w1, b1, w2, b2, scale)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 2:
        raise UformerHipError("ffn: x must be a contiguous f32 (M, ld) tensor (it is updated in place)")
    dt = uf_dtype(w1.dtype)
    M, ld = x.shape
    Cc = ld if C is None else int(C)
    if tuple(w1.shape) != (4 * Cc, Cc) or tuple(w2.shape) != (Cc, 4 * Cc):
        raise UformerHipError(f"ffn: w1 {tuple(w1.shape)} / w2 {tuple(w2.shape)} do not match C = {Cc}")
    _launch("uf_ffn_fwd", x.device, x, ld, _f32(gamma), _f32(beta), _pack_frag(w1), _f32(b1), _pack_frag(_c(w2, w1.dtype)), _f32(b2), _f32(scale),
            B, M, Cc, dt)
    return x


def cross_attn(x: Tensor, wq: Tensor, bq: Tensor, k: Tensor, vt: Tensor, wp: Tensor, bp: Tensor, C: Optional[int] = None) -> Tensor:
    """The cross-modulator attention of a decoder block, IN PLACE on ``x``: x[m, :C] += proj(softmax((x[m, :C] wq^T + bq) hd^-0.5 . k_h^T) v_h)
    (model.py:945-949, :549-595; uf_cross_attn_fwd).  x f32 (M, ld) contiguous rows on the GPU with the channels in columns [0, C) (``C`` default:
    ld), M a multiple of 64; wq, wp T (C, C) row-major (packed fragment-major here); k T (heads, 64, hd) unscaled and vt T (heads, hd, 64) =
    to_kv(cross_modulator.weight) (packing.pack_cross); bq, bp f32 (C,).  Returns x."""
    _dev(x, wq, bq, k, vt, wp, bp)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 2:
        raise UformerHipError("cross_attn: x must be a contiguous f32 (M, ld) tensor (it is updated in place)")
    dt = uf_dtype(wq.dtype)
    M, ld = x.shape
    Cc = ld if C is None else int(C)
    heads, nk, hd = k.shape
    if tuple(wq.shape) != (Cc, Cc) or tuple(wp.shape) != (Cc, Cc) or nk != 64 or heads * hd != Cc or tuple(vt.shape) != (heads, hd, 64):
        raise UformerHipError(f"cross_attn: wq {tuple(wq.shape)} / wp {tuple(wp.shape)} / k {tuple(k.shape)} / vt {tuple(vt.shape)} do not match C = {Cc}")
    # the struct holds addresses, not tensors: ``fields`` owns the operands until the call has returned
    fields = (_pack_frag(wq), _c(bq, torch.float32), _c(k, wq.dtype), _c(vt, wq.dtype), _pack_frag(_c(wp, wq.dtype)), _c(bp, torch.float32))
    cp = _lib.CrossParams()
    for name, tns in zip(("wq_fm", "bq", "k", "vt", "wp_fm", "bp"), fields):
        setattr(cp, name, _ptr(tns))
    cp.heads = int(heads)
    _launch("uf_cross_attn_fwd", x.device, cp, x, ld, M, Cc, dt)
    return x


def window_attention_core(q: Tensor, k: Tensor, vt: Tensor, bias_dense: Tensor, *, H: int, W: int, shift: int = 0,
                          mask: Optional[Tensor] = None) -> Tensor:
    """softmax(q k^T + bias + masks) v -> (n_windows*64, C).  model.py:498-519."""
    _dev(q, k, vt, bias_dense, mask)
    dt = uf_dtype(q.dtype)
    nwin, heads, _, hd = q.shape
    out = torch.empty((nwin * 64, heads * hd), dtype=q.dtype, device=q.device)
    mask = _f32(mask)
    _launch("uf_window_attention_fwd", q.device, _c(q), _c(k), _c(vt), _f32(bias_dense), mask, 0 if mask is None else mask.shape[0], out,
            nwin, heads, hd, H, W, shift, dt)
    return out


def dwconv3x3_gelu(x: Tensor, w9: Tensor, bias: Tensor) -> Tensor:
    """x T(B,H,W,C) channel-last; w9 f32 (9,C); LeFF dwconv + GELU (model.py:659-660)."""
    _dev(x, w9, bias)
    dt = uf_dtype(x.dtype)
    x = _c(x)
    B, H, W, Cc = x.shape
    out = torch.empty_like(x)
    _launch("uf_dwconv3x3_gelu_fwd", x.device, x, _f32(w9), _f32(bias), out, B, H, W, Cc, dt)
    return out


def dwconv3x3(x: Tensor, w9: Tensor, bias: Optional[Tensor] = None, gelu: bool = False) -> Tensor:
    """The depthwise 3x3 stencil with optional bias / GELU.  With ``w9.flip(0)`` (taps flipped), no bias and no GELU it is
    the input gradient of the convolution."""
    _dev(x, w9)
    dt = uf_dtype(x.dtype)
    x = _c(x)
    B, H, W, Cc = x.shape
    out = torch.empty_like(x)
    _launch("uf_dwconv3x3_fwd", x.device, x, _f32(w9), _f32(bias), out, B, H, W, Cc, 1 if gelu else 0, dt)
    return out


def dwconv3x3_pre_gelu(x: Tensor, w9: Tensor, bias: Tensor, gelu_in: bool = False) -> Tuple[Tensor, Tensor]:
    """(pre, GELU(pre)) of the depthwise stencil in one pass (training forward keeps both).  ``gelu_in``: x is the PRE-activation of the GELU in
    front of the convolution and the kernel activates it as it loads it (uf_dwconv3x3_gelu_in_pre_gelu_fwd) -- same bits as passing the stored
    activation."""
    _dev(x, w9, bias)
    x = _c(x)
    B, H, W, Cc = x.shape
    pre, act = torch.empty_like(x), torch.empty_like(x)
    _launch("uf_dwconv3x3_gelu_in_pre_gelu_fwd" if gelu_in else "uf_dwconv3x3_pre_gelu_fwd", x.device, x, _f32(w9), _f32(bias), pre, act,
            B, H, W, Cc, uf_dtype(x.dtype))
    return pre, act


def dwconv3x3_mul_dgelu(dy: Tensor, w9_flipped: Tensor, pre: Tensor) -> Tensor:
    """Gradient through the depthwise conv and the GELU in front of it: stencil(dy; flipped taps) * GELU'(pre)."""
    _dev(dy, w9_flipped, pre)
    dy, pre = _c(dy), _c(pre, dy.dtype)
    B, H, W, Cc = dy.shape
    out = torch.empty_like(dy)
    _launch("uf_dwconv3x3_mul_dgelu", dy.device, dy, _f32(w9_flipped), pre, out, B, H, W, Cc, uf_dtype(dy.dtype))
    return out


def linear_pre_gelu(a: Tensor, w: Tensor, bias: Tensor) -> Tuple[Tensor, Tensor]:
    """(a W^T + bias, GELU of it) in one pass; both T(M, N)."""
    _dev(a, w, bias)
    a, w = _c(a), _c(w, a.dtype)
    M, K = a.shape
    N = w.shape[0]
    pre = torch.empty((M, N), dtype=a.dtype, device=a.device)
    act = torch.empty_like(pre)
    _launch("uf_linear_pre_gelu_fwd", a.device, a, w, _f32(bias), pre, act, M, N, K, uf_dtype(a.dtype))
    return pre, act


def linear_mul_dgelu(dy: Tensor, w_t: Tensor, zero_bias: Tensor, pre: Tensor) -> Tensor:
    """(dy @ w_t.T) * GELU'(pre): input gradient of a Linear fed by a GELU; w_t (K_layer, N_layer) is the transposed weight."""
    _dev(dy, w_t, pre)
    dy, w_t, pre = _c(dy), _c(w_t, dy.dtype), _c(pre, dy.dtype)
    M, K = dy.shape
    N = w_t.shape[0]
    out = torch.empty((M, N), dtype=dy.dtype, device=dy.device)
    _launch("uf_linear_mul_dgelu", dy.device, dy, w_t, _f32(zero_bias), pre, out, M, N, K, uf_dtype(dy.dtype))
    return out


def gelu(a: Tensor) -> Tensor:
    """GELU(a) as a separate pass (nn.GELU, model.py:657-660); bf16 / f32."""
    _dev(a)
    dt = uf_dtype(a.dtype)
    a = _c(a)
    out = torch.empty_like(a)
    _launch("uf_gelu_fwd", a.device, a, out, a.numel(), dt)
    return out


def gelu_bwd(a: Tensor, dy: Tensor) -> Tensor:
    """dy * GELU'(a), erf form (backward of nn.GELU, model.py:657-660).  a, dy: same shape and dtype (bf16 / f32)."""
    _dev(a, dy)
    dt = uf_dtype(a.dtype)
    a, dy = _c(a), _c(dy, a.dtype)
    out = torch.empty_like(a)
    _launch("uf_gelu_bwd", a.device, a, dy, out, a.numel(), dt)
    return out


def layernorm_bwd(x: Tensor, gamma: Tensor, dy: Tensor):
    """Backward of nn.LayerNorm over the last dim of f32 rows: returns (dx, dgamma, dbeta).  model.py:881,888."""
    _dev(x, gamma, dy)
    Cc = x.shape[-1]
    x2, dy2 = _c(x, torch.float32).reshape(-1, Cc), _c(dy, torch.float32).reshape(-1, Cc)
    rows = x2.shape[0]
    dx = torch.empty_like(x2)
    dg = torch.empty(Cc, dtype=torch.float32, device=x.device)
    db = torch.empty(Cc, dtype=torch.float32, device=x.device)
    _launch("uf_layernorm_bwd", x.device, x2, Cc, _f32(gamma), dy2, Cc, dx, Cc, dg, db, rows, Cc,
            *_workspace("uf_layernorm_bwd_workspace_bytes", x.device, rows, Cc))
    return dx.reshape(x.shape), dg, db


def layernorm_bwd_fused(x: Tensor, gamma: Tensor, dy: Tensor, B: int, H: int, W: int, add: Optional[Tensor] = None, windowed: bool = False, shift: int = 0,
                        cast: Optional[dict] = None):
    """layernorm_bwd reading dy (bf16 or f32 rows, in WINDOW order when ``windowed``) where the block backward has it, with an optional
    second gradient ``add`` (f32) summed into dx: returns (dx f32 (B*H*W, C) raster rows, dgamma, dbeta).  ``cast`` = dict(scale=(B,) f32 or
    None, windowed=bool, shift=int): a fourth result, (dx * scale[image]) in dy's dtype, in window order when cast['windowed'] -- the operand
    of the next GEMM of the backward (what ``grad_fork(dx, ...)`` returns), written by the same kernel (uf_layernorm_bwd_cast)."""
    _dev(x, gamma, dy)
    Cc = x.shape[-1]
    x2, dy2 = _c(x, torch.float32).reshape(-1, Cc), _c(dy).reshape(-1, Cc)
    add2 = None if add is None else _c(add, torch.float32).reshape(-1, Cc)
    dx = torch.empty_like(x2)
    dg = torch.empty(Cc, dtype=torch.float32, device=x.device)
    db = torch.empty(Cc, dtype=torch.float32, device=x.device)
    ws = _workspace("uf_layernorm_bwd_workspace_bytes", x.device, x2.shape[0], Cc)
    common = (x2, Cc, _f32(gamma), dy2, Cc, int(dy2.dtype == torch.float32), add2, dx, Cc, dg, db, B, H, W, Cc, int(windowed), shift, uf_dtype(dy2.dtype))
    if cast is None:
        _launch("uf_layernorm_bwd_fused", x.device, *common, *ws)
        return dx, dg, db
    out = torch.empty(B * H * W, Cc, dtype=dy2.dtype, device=x.device)
    _launch("uf_layernorm_bwd_cast", x.device, *common, out, _f32(cast.get("scale")), int(bool(cast.get("windowed", False))), int(cast.get("shift", 0)), *ws)
    return dx, dg, db, out


def linear_wgrad(dy: Tensor, x: Tensor, with_bias: bool = True):
    """nn.Linear parameter gradients from the output gradient dy (..., N) and the layer input x (..., K), same dtype
    (bf16 / f32): returns (dW f32 (N,K), db f32 (N,) or None).  The input gradient is ``linear(dy, W.t())``."""
    _dev(dy, x)
    dt = uf_dtype(x.dtype)
    N, K = dy.shape[-1], x.shape[-1]
    dy2, x2 = _c(dy, x.dtype).reshape(-1, N), _c(x).reshape(-1, K)
    M = x2.shape[0]
    dW = torch.empty(N, K, dtype=torch.float32, device=x.device)
    db = torch.empty(N, dtype=torch.float32, device=x.device) if with_bias else None
    _launch("uf_linear_wgrad", x.device, dy2, N, x2, K, dW, db, M, N, K, dt, *_workspace("uf_linear_wgrad_workspace_bytes", x.device, M, N, K))
    return dW, db


def window_attention_bwd(q: Tensor, k: Tensor, vt: Tensor, bias: Tensor, do: Tensor, H: int, W: int, shift: int = 0,
                         mask: Optional[Tensor] = None):
    """Backward of window_attention_core: q (scaled), k (nW*heads,64,hd), vt (nW*heads,hd,64), bias f32 (heads,64,64),
    do (nW*64, heads*hd) -> (dq, dk, dvt, dbias f32 (heads,64,64) summed over windows).  model.py:494-519."""
    _dev(q, k, vt, bias, do)
    dt = uf_dtype(q.dtype)
    q, k, vt, do = _c(q), _c(k, q.dtype), _c(vt, q.dtype), _c(do, q.dtype)
    heads = bias.shape[0]
    hd = q.shape[-1]
    n_windows = q.numel() // (heads * 64 * hd)           # q may be (nW*heads, 64, hd) or (nW, heads, 64, hd)
    dq, dk, dvt = torch.empty_like(q), torch.empty_like(k), torch.empty_like(vt)
    dbias = torch.empty(heads, 64, 64, dtype=torch.float32, device=q.device)
    m = _f32(mask)
    _launch("uf_window_attention_bwd", q.device, q, k, vt, _f32(bias), m, m.shape[0] if m is not None else 0, do, do.shape[-1], dq, dk, dvt, dbias,
            n_windows, heads, hd, H, W, shift, dt, *_workspace("uf_window_attention_bwd_workspace_bytes", q.device, n_windows, heads))
    return dq, dk, dvt, dbias


def window_attention_bwd_qkv(q: Tensor, k: Tensor, vt: Tensor, bias: Tensor, do: Tensor, H: int, W: int, shift: int = 0,
                             mask: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """window_attention_bwd writing the merged gradient of the q|k|v projection output: (dqkv (nW*64, 3C), dbias (heads,64,64))."""
    _dev(q, k, vt, bias, do)
    dt = uf_dtype(q.dtype)
    q, k, vt, do = _c(q), _c(k, q.dtype), _c(vt, q.dtype), _c(do, q.dtype)
    heads = bias.shape[0]
    hd = q.shape[-1]
    n_windows = q.numel() // (heads * 64 * hd)
    dqkv = torch.empty(n_windows * 64, 3 * heads * hd, dtype=q.dtype, device=q.device)
    dbias = torch.empty(heads, 64, 64, dtype=torch.float32, device=q.device)
    m = _f32(mask)
    _launch("uf_window_attention_bwd_qkv", q.device, q, k, vt, _f32(bias), m, m.shape[0] if m is not None else 0, do, do.shape[-1], dqkv, dbias,
            n_windows, heads, hd, H, W, shift, dt, *_workspace("uf_window_attention_bwd_workspace_bytes", q.device, n_windows, heads))
    return dqkv, dbias


def dwconv3x3_wgrad(h: Tensor, dc: Tensor):
    """Tap (9,C) and bias (C,) gradients of the depthwise 3x3 from its input h and output gradient dc, both T(B,H,W,C)."""
    _dev(h, dc)
    dt = uf_dtype(h.dtype)
    h, dc = _c(h), _c(dc, h.dtype)
    B, H, W, Cc = h.shape
    dw9 = torch.empty(9, Cc, dtype=torch.float32, device=h.device)
    db = torch.empty(Cc, dtype=torch.float32, device=h.device)
    _launch("uf_dwconv3x3_wgrad", h.device, h, dc, dw9, db, B, H, W, Cc, dt, *_workspace("uf_dwconv3x3_wgrad_workspace_bytes", h.device, Cc, dt))
    return dw9, db


def dwconv3x3_bwd(dc: Tensor, w9_flipped: Tensor, pre: Tensor):
    """Whole backward of the LeFF depthwise conv behind its GELU, one pass over dc (model.py:657-660): returns (da = stencil(dc; flipped
    taps) * GELU'(pre) -- as dwconv3x3_mul_dgelu --, dw9 (9,C), db (C,) -- as dwconv3x3_wgrad(GELU(pre), dc))."""
    _dev(dc, w9_flipped, pre)
    dt = uf_dtype(dc.dtype)
    dc, pre = _c(dc), _c(pre, dc.dtype)
    B, H, W, Cc = dc.shape
    da = torch.empty_like(dc)
    dw9 = torch.empty(9, Cc, dtype=torch.float32, device=dc.device)
    db = torch.empty(Cc, dtype=torch.float32, device=dc.device)
    _launch("uf_dwconv3x3_bwd", dc.device, dc, _f32(w9_flipped), pre, da, dw9, db, B, H, W, Cc, dt,
            *_workspace("uf_dwconv3x3_bwd_workspace_bytes", dc.device, Cc, dt))
    return da, dw9, db


def dwconv_linear2(h1: Tensor, w9: Tensor, bdw: Tensor, w2: Tensor, b2: Tensor, x: Tensor) -> Tensor:
    """x + linear2(GELU(dwconv3x3(h1))) (model.py:674-683, :987).  h1 T(B,H,W,4C); x f32 (B*H*W, C); returns new x."""
    _dev(h1, w9, bdw, w2, b2, x)
    dt = uf_dtype(h1.dtype)
    h1 = _c(h1)
    B, H, W, hid = h1.shape
    out = _c(x, torch.float32).clone()
    Cc = out.shape[-1]
    _launch("uf_dwconv_linear2_fwd", h1.device, h1, _f32(w9), _f32(bdw), _pack_frag(_c(w2, h1.dtype)), _f32(b2), out, Cc, B, H, W, Cc, dt)
    return out


def lewin_attn_train_fwd(bp, x: Tensor, B: int, H: int, W: int, heads: int, dtype, drop_attn: Optional[Tensor] = None):
    """Training forward of the attention half + linear1 of a LeWin block in ONE launch (uf_lewin_attn_train_fwd; model.py:951-987, :657-658): the fused
    window kernel with side stores of what the backward reads.  bp: _lib.BlockParams (the fused pack); x f32 (B*H*W, C), untouched.
    Returns (x1 f32 (M, C), xn, q, k, vt, o, z, a1) in the layouts of layernorm(windowed) / qkv / window_attention_core / layernorm / linear."""
    _dev(x, drop_attn)
    x = _c(x, torch.float32)
    M, Cc = x.shape
    T, hd = torch_dtype(uf_dtype(dtype)), Cc // heads
    dev = x.device
    x1 = torch.empty_like(x)
    xn, o, z = (torch.empty((M, Cc), dtype=T, device=dev) for _ in range(3))
    q = torch.empty((M // 64, heads, 64, hd), dtype=T, device=dev)
    k = torch.empty_like(q)
    vt = torch.empty((M // 64, heads, hd, 64), dtype=T, device=dev)
    a1 = torch.empty((M, 4 * Cc), dtype=T, device=dev)
    _launch("uf_lewin_attn_train_fwd", dev, bp, x, Cc, x1, Cc, B, H, W, Cc, _f32(drop_attn), uf_dtype(dtype), xn, q, k, vt, o, z, a1)
    return x1, xn, q, k, vt, o, z, a1


def pack_weight_fm(w: Tensor) -> Tensor:
    """Row-major (N, K) weight of a 2- or 4-byte operand type -> the fragment-major layout of ``uf_pack_weight_fm`` (N a multiple of 16)."""
    return _pack_frag(w)


def downsample(x: Tensor, w_packed: Tensor, bias: Tensor, B: int, H: int, W: int, w_fm: Optional[Tensor] = None) -> Tensor:
    """x f32 (B*H*W, C) -> f32 (B*H/2*W/2, 2C).  Downsample.forward model.py:739-746.  ``w_fm``: ``pack_weight_fm(w_packed)`` if the caller has it
    (the LDS-patch form of the kernel then streams it; same bits either way)."""
    _dev(x, w_packed, bias)
    x = _c(x, torch.float32)
    Cc = x.shape[-1]
    out = torch.empty((B * (H // 2) * (W // 2), 2 * Cc), dtype=torch.float32, device=x.device)
    if w_fm is not None:
        _launch("uf_downsample_fm_fwd", x.device, x, Cc, _c(w_packed), _c(w_fm), _f32(bias), out, 2 * Cc, B, H, W, Cc, uf_dtype(w_packed.dtype))
    else:
        _launch("uf_downsample_fwd", x.device, x, Cc, _c(w_packed), _f32(bias), out, 2 * Cc, B, H, W, Cc, uf_dtype(w_packed.dtype))
    return out


def upsample(x: Tensor, w_packed: Tensor, bias: Tensor, B: int, H: int, W: int, out: Optional[Tensor] = None,
             ld_o: Optional[int] = None) -> Tensor:
    """x f32 (B*H*W, Cin) -> f32 (B*2H*2W, Cout).  Upsample.forward model.py:765-771."""
    _dev(x, w_packed, bias)
    x = _c(x, torch.float32)
    Cin = x.shape[-1]
    Cout = w_packed.shape[0] // 4
    if out is None:
        out = torch.empty((B * 4 * H * W, Cout), dtype=torch.float32, device=x.device)
        ld_o = Cout
    _launch("uf_upsample_fwd", x.device, x, Cin, _c(w_packed), _f32(bias), out, ld_o, B, H, W, Cin, Cout, uf_dtype(w_packed.dtype))
    return out


def input_proj(img: Tensor, w27: Tensor, bias: Tensor) -> Tensor:
    """img f32 NCHW -> tokens f32 (B*H*W, E).  InputProj.forward model.py:795-800."""
    _dev(img, w27, bias)
    img = _c(img, torch.float32)
    B, Cin, H, W = img.shape
    E = w27.shape[1]
    out = torch.empty((B * H * W, E), dtype=torch.float32, device=img.device)
    _launch("uf_input_proj_fwd", img.device, img, _f32(w27), _f32(bias), out, E, B, Cin, H, W, E)
    return out


def output_proj(x: Tensor, w: Tensor, bias: Tensor, B: int, H: int, W: int, img: Optional[Tensor] = None) -> Tensor:
    """tokens f32 (B*H*W, C2) -> f32 NCHW (B,Cout,H,W) (+ img of the same shape); ``w`` (Cout, 9, C2) from packing.pack_output_proj, Cout 1..4.
    OutputProj.forward model.py:828-836, :1305."""
    _dev(x, w, bias, img)
    x = _c(x, torch.float32)
    C2 = x.shape[-1]
    Cout = w.shape[0]
    if w.dim() != 3 or tuple(w.shape[1:]) != (9, C2) or bias.numel() != Cout:
        raise UformerHipError(f"output_proj: w {tuple(w.shape)} / bias {tuple(bias.shape)} do not match (Cout, 9, {C2}) / (Cout,)")
    if img is not None:
        img = _c(img, torch.float32)
        if tuple(img.shape) != (B, Cout, H, W):
            raise UformerHipError(f"output_proj: img {tuple(img.shape)} must have the output's shape {(B, Cout, H, W)}")
    out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    _launch("uf_output_proj_c_fwd", x.device, x, C2, _f32(w), _f32(bias), img, out, B, H, W, C2, Cout, int(img is not None))
    return out


# ---------------------------------------------------------------------------------------
# training-step tail, metrics, arbitrary-resolution wrapper, input pipeline
# ---------------------------------------------------------------------------------------
def charbonnier(y: Tensor, target: Tensor, eps: float = 1e-3, with_grad: bool = True, grad_scale: float = 1.0):
    """CharbonnierLoss.forward (losses.py:41-52) and d loss / d y in ONE pass: returns (loss f32 0-dim tensor, dy or None)."""
    _dev(y, target)
    y, target = _c(y, torch.float32), _c(target, torch.float32)
    n = y.numel()
    loss = torch.empty(1, dtype=torch.float32, device=y.device)
    dy = torch.empty_like(y) if with_grad else None
    _launch("uf_charbonnier_fwd_bwd", y.device, y, target, dy, loss, n, eps, grad_scale, *_workspace("uf_charbonnier_workspace_bytes", y.device, n))
    return loss.reshape(()), dy


def adamw_step(params, grads, exp_avg, exp_avg_sq, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.02,
               step: int = 1, grad_scale: float = 1.0) -> None:
    """One torch.optim.AdamW step over lists of f32 tensors, in place (train/train_denoise.py:77).  ``step`` counts from 1."""
    n = len(params)
    if not (len(grads) == len(exp_avg) == len(exp_avg_sq) == n):
        raise UformerHipError("adamw_step: list lengths differ")
    if n == 0:
        return
    dev = _dev(*params, *grads, *exp_avg, *exp_avg_sq)
    for group in (params, grads, exp_avg, exp_avg_sq):
        for t in group:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise UformerHipError("adamw_step: tensors must be contiguous float32")
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    numel = (ctypes.c_longlong * n)(*[p.numel() for p in params])
    _launch("uf_adamw_step", dev, arr(params), arr(grads), arr(exp_avg), arr(exp_avg_sq), numel, n, lr, betas[0], betas[1], eps,
            weight_decay, int(step), grad_scale)


def adamw_step_scaled(params, grads, exp_avg, exp_avg_sq, scaler_state: Tensor, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.02,
                      grad_scale: float = 1.0) -> None:
    """``adamw_step`` under a device-resident dynamic loss scale (uf_adamw_step_scaled): gradients x grad_scale / scale, nothing written when
    ``scaler_state[2]`` (found_inf) is set, bias corrections at step ``scaler_state[4] + 1``.  No host synchronisation."""
    n = len(params)
    if not (len(grads) == len(exp_avg) == len(exp_avg_sq) == n):
        raise UformerHipError("adamw_step_scaled: list lengths differ")
    if n == 0:
        return
    dev = _dev(*params, *grads, *exp_avg, *exp_avg_sq, scaler_state)
    for group in (params, grads, exp_avg, exp_avg_sq, [scaler_state]):
        for t in group:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise UformerHipError("adamw_step_scaled: tensors must be contiguous float32")
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    numel = (ctypes.c_longlong * n)(*[p.numel() for p in params])
    _launch("uf_adamw_step_scaled", dev, arr(params), arr(grads), arr(exp_avg), arr(exp_avg_sq), numel, n, lr, betas[0], betas[1], eps,
            weight_decay, grad_scale, scaler_state)


def grad_scaler_check(grads, scaler_state: Tensor) -> None:
    """scaler_state[2] = 1 if any gradient element is inf / nan (uf_grad_scaler_check)."""
    grads = [g for g in grads if g is not None]
    n = len(grads)
    if n == 0:
        return
    dev = _dev(*grads, scaler_state)
    for t in grads:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise UformerHipError("grad_scaler_check: gradients must be contiguous float32")
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in grads])
    numel = (ctypes.c_longlong * n)(*[t.numel() for t in grads])
    _launch("uf_grad_scaler_check", dev, arr, numel, n, scaler_state)


def grad_scaler_update(scaler_state: Tensor, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000) -> None:
    """GradScaler.update() on the device (uf_grad_scaler_update)."""
    _dev(scaler_state)
    _launch("uf_grad_scaler_update", scaler_state.device, scaler_state, growth_factor, backoff_factor, int(growth_interval))


def batch_mse(a: Tensor, b: Tensor, clamp01: bool = True) -> Tensor:
    """Per-image mean squared difference of (B,C,H,W) f32 images, clamped to [0,1] first (myPSNR, utils/image_utils.py:40-44)."""
    _dev(a, b)
    a, b = _c(a, torch.float32), _c(b, torch.float32)
    if a.shape != b.shape or a.dim() != 4:
        raise UformerHipError(f"batch_mse: shapes {tuple(a.shape)} / {tuple(b.shape)}")
    B, Cc, H, W = a.shape
    out = torch.empty(B, dtype=torch.float32, device=a.device)
    _launch("uf_batch_mse", a.device, a, b, out, B, Cc, H, W, int(clamp01), *_workspace("uf_image_metric_workspace_bytes", a.device, B, Cc, H, W))
    return out


def batch_ssim(a: Tensor, b: Tensor) -> Tensor:
    """Per-image SSIM of (B,C,H,W) f32 images in [0,1] as calculate_ssim computes it (utils/caculate_psnr_ssim.py:35-81)."""
    _dev(a, b)
    a, b = _c(a, torch.float32), _c(b, torch.float32)
    if a.shape != b.shape or a.dim() != 4:
        raise UformerHipError(f"batch_ssim: shapes {tuple(a.shape)} / {tuple(b.shape)}")
    B, Cc, H, W = a.shape
    out = torch.empty(B, dtype=torch.float32, device=a.device)
    _launch("uf_batch_ssim", a.device, a, b, out, B, Cc, H, W, *_workspace("uf_image_metric_workspace_bytes", a.device, B, Cc, H, W))
    return out


def expand2square(img: Tensor, factor: float = 128.0, with_mask: bool = True):
    """test/test_sidd.py:79-92 for a batch: (B,C,h,w) -> zero canvas (B,C,X,X) with the image centred, + (B,1,X,X) mask."""
    import math
    _dev(img)
    img = _c(img, torch.float32)
    B, Cc, h, w = img.shape
    X = int(math.ceil(max(h, w) / float(factor)) * factor)
    canvas = torch.empty((B, Cc, X, X), dtype=torch.float32, device=img.device)
    mask = torch.empty((B, 1, X, X), dtype=torch.float32, device=img.device) if with_mask else None
    _launch("uf_expand2square", img.device, img, canvas, mask, B, Cc, h, w, X)
    return canvas, mask


def crop_clamp(canvas: Tensor, h: int, w: int, clamp: bool = True) -> Tensor:
    """masked_select crop of the restored canvas back to (B,C,h,w) + clamp to [0,1] (test/test_sidd.py:108-109)."""
    _dev(canvas)
    canvas = _c(canvas, torch.float32)
    B, Cc, X, X2 = canvas.shape
    if X != X2:
        raise UformerHipError("crop_clamp: square canvas expected")
    out = torch.empty((B, Cc, h, w), dtype=torch.float32, device=canvas.device)
    _launch("uf_crop_clamp", canvas.device, canvas, out, B, Cc, h, w, X, int(clamp))
    return out


def expand_canvas(img: Tensor, Xh: int, Xw: int, with_mask: bool = True):
    """(B,C,h,w) -> zero canvas (B,C,Xh,Xw) with the image at ((Xh-h)//2, (Xw-w)//2) -- expand2square's placement rule on
    each axis -- + the (B,1,Xh,Xw) mask of ones over the image (or None)."""
    _dev(img)
    img = _c(img, torch.float32)
    B, Cc, h, w = img.shape
    if Xh < h or Xw < w:
        raise UformerHipError(f"expand_canvas: canvas {Xh}x{Xw} smaller than the image {h}x{w}")
    canvas = torch.empty((B, Cc, Xh, Xw), dtype=torch.float32, device=img.device)
    mask = torch.empty((B, 1, Xh, Xw), dtype=torch.float32, device=img.device) if with_mask else None
    _launch("uf_expand_canvas", img.device, img, canvas, mask, B, Cc, h, w, Xh, Xw)
    return canvas, mask


def crop_clamp_canvas(canvas: Tensor, h: int, w: int, clamp: bool = True) -> Tensor:
    """Inverse of expand_canvas: the (B,C,h,w) region at ((Xh-h)//2, (Xw-w)//2) of a (B,C,Xh,Xw) canvas, optionally clamped to [0,1]."""
    _dev(canvas)
    canvas = _c(canvas, torch.float32)
    B, Cc, Xh, Xw = canvas.shape
    out = torch.empty((B, Cc, h, w), dtype=torch.float32, device=canvas.device)
    _launch("uf_crop_clamp_canvas", canvas.device, canvas, out, B, Cc, h, w, Xh, Xw, int(clamp))
    return out


def crop_augment(frames: Tensor, meta: Tensor, ps: int, hwc: bool = False) -> Tensor:
    """frames: (N,C,H,W) or (N,H,W,C) (hwc) uint8 / f32 on the GPU, any channel count C; meta int32 (B,4) = [frame index, r0, c0, transform 0..7]
    -> (B,C,ps,ps) f32 patches (dataset/dataset_denoise.py:54-70; uint8 is divided by 255 like load_img)."""
    _dev(frames, meta)
    if frames.dtype not in (torch.uint8, torch.float32):
        raise UformerHipError("crop_augment: frames must be uint8 or float32")
    frames, meta = _c(frames), _c(meta, torch.int32)
    N = frames.shape[0]
    if frames.dim() != 4:
        raise UformerHipError(f"crop_augment: frames must be (N,C,H,W) or (N,H,W,C), got {tuple(frames.shape)}")
    H, W, Cc = (frames.shape[1], frames.shape[2], frames.shape[3]) if hwc else (frames.shape[2], frames.shape[3], frames.shape[1])
    B = meta.shape[0]
    out = torch.empty((B, Cc, ps, ps), dtype=torch.float32, device=frames.device)
    _launch("uf_crop_augment_c", frames.device, frames, int(frames.dtype == torch.uint8), int(hwc), out, meta, B, N, Cc, H, W, ps)
    return out


def _frame_dims(frames: Tensor, hwc: bool, what: str):
    if frames.dim() != 4:
        raise UformerHipError(f"{what}: frames must be (B,h,w,C) or (B,C,h,w), got {tuple(frames.shape)}")
    B, a, b, c = frames.shape
    return (B, c, a, b) if hwc else (B, a, b, c)                # B, C, h, w


def _u8_frames(B: int, Cc: int, h: int, w: int, hwc: bool, device, out: Optional[Tensor], what: str) -> Tensor:
    shape = (B, h, w, Cc) if hwc else (B, Cc, h, w)
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != device:
        raise UformerHipError(f"{what}: out must be a contiguous uint8 tensor of shape {shape} on {device}")
    return out


def frames_to_canvas(frames: Tensor, Xh: int, Xw: int, hwc: bool = True, swap_rb: bool = False, with_mask: bool = False):
    """uint8 frames (B,h,w,C) (``hwc``) or (B,C,h,w) -> f32 canvas (B,C,Xh,Xw) = u / 255 at ((Xh-h)//2, (Xw-w)//2), zero elsewhere, + the
    (B,1,Xh,Xw) mask (or None): ``expand_canvas`` of the float frames bit for bit, one launch.  ``swap_rb``: BGR(A) frames to RGB(A) planes."""
    _dev(frames)
    if frames.dtype != torch.uint8:
        raise UformerHipError("frames_to_canvas: frames must be uint8")
    B, Cc, h, w = _frame_dims(frames, hwc, "frames_to_canvas")
    canvas = torch.empty((B, Cc, Xh, Xw), dtype=torch.float32, device=frames.device)
    mask = torch.empty((B, 1, Xh, Xw), dtype=torch.float32, device=frames.device) if with_mask else None
    _launch("uf_frames_to_canvas", frames.device, _c(frames), int(hwc), int(swap_rb), canvas, mask, B, Cc, h, w, Xh, Xw)
    return canvas, mask


def canvas_to_frames(canvas: Tensor, h: int, w: int, hwc: bool = True, swap_rb: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """Inverse of frames_to_canvas: crop + clamp to [0,1] + quantise, ``img_as_ubyte(clamp(x, 0, 1))`` for float32 (rint of the f32 product
    with 255, ties to even; NaN gives 0), as uint8 (B,h,w,C) or (B,C,h,w); ``out`` receives the frames when given."""
    _dev(canvas)
    B, Cc, Xh, Xw = canvas.shape
    frames = _u8_frames(B, Cc, h, w, hwc, canvas.device, out, "canvas_to_frames")
    _launch("uf_canvas_to_frames", canvas.device, _c(canvas, torch.float32), frames, int(hwc), int(swap_rb), B, Cc, h, w, Xh, Xw)
    return frames


def tiles_gather(frames: Tensor, origins: Tensor, tile: int, hwc: bool = False, swap_rb: bool = False) -> Tensor:
    """The tile batch of ``infer.restore_tiled``: frames uint8 (divided by 255) or f32, (B,h,w,C) (``hwc``) or (B,C,h,w); origins int32 (T,2) =
    (y, x) on the device -> f32 (T*B, C, tile, tile), entry k*B + b = frame b from origin k, zero beyond the frame."""
    _dev(frames, origins)
    if frames.dtype not in (torch.uint8, torch.float32):
        raise UformerHipError("tiles_gather: frames must be uint8 or float32")
    B, Cc, h, w = _frame_dims(frames, hwc, "tiles_gather")
    if origins.dim() != 2 or origins.shape[1] != 2:
        raise UformerHipError(f"tiles_gather: origins must be (T,2), got {tuple(origins.shape)}")
    T = origins.shape[0]
    tiles = torch.empty((T * B, Cc, tile, tile), dtype=torch.float32, device=frames.device)
    _launch("uf_tiles_gather", frames.device, _c(frames), int(frames.dtype == torch.uint8), int(hwc), int(swap_rb), tiles, _c(origins, torch.int32),
            T, B, Cc, h, w, tile)
    return tiles


def tiles_blend(tiles_out: Tensor, ys, xs, h: int, w: int, u8: bool = False, hwc: bool = True, swap_rb: bool = False, clamp: bool = True,
                out: Optional[Tensor] = None) -> Tensor:
    """Cross-fade of restored tiles (len(ys)*len(xs)*B, C, tile, tile), job order [(y,x) for y in ys for x in xs], into frames of (h, w):
    sum of ramp weight x tile over the sum of the weights (``infer.restore_tiled``'s blend, one launch, no accumulator).  f32 planes
    (B,C,h,w), clamped to [0,1] with ``clamp``; ``u8``: uint8 frames (B,h,w,C) (``hwc``) or (B,C,h,w) through canvas_to_frames' quantiser."""
    _dev(tiles_out)
    ys, xs = [int(v) for v in ys], [int(v) for v in xs]
    n, Cc, tile, tile2 = tiles_out.shape
    if tile != tile2 or not ys or not xs or n % (len(ys) * len(xs)):
        raise UformerHipError(f"tiles_blend: {tuple(tiles_out.shape)} is no batch of square tiles for {len(ys)} x {len(xs)} origins")
    B = n // (len(ys) * len(xs))
    if u8:
        res = _u8_frames(B, Cc, h, w, hwc, tiles_out.device, out, "tiles_blend")
    elif out is None:
        res = torch.empty((B, Cc, h, w), dtype=torch.float32, device=tiles_out.device)
    else:
        if out.dtype != torch.float32 or tuple(out.shape) != (B, Cc, h, w) or not out.is_contiguous() or out.device != tiles_out.device:
            raise UformerHipError(f"tiles_blend: out must be a contiguous float32 tensor of shape {(B, Cc, h, w)} on {tiles_out.device}")
        res = out
    _launch("uf_tiles_blend", tiles_out.device, _c(tiles_out, torch.float32), (ctypes.c_int * len(ys))(*ys), len(ys), (ctypes.c_int * len(xs))(*xs), len(xs),
            res, int(u8), int(hwc), int(swap_rb), int(clamp), B, Cc, h, w, tile)
    return res


def tta_gather(src: Tensor, ks, Xh: int, Xw: int, hwc: bool = False, swap_rb: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """The member batch of ``infer.restore_ensemble``: frames uint8 (divided by 255) or f32, (B,h,w,C) (``hwc``) or (B,C,h,w) -> f32
    (len(ks)*B, C, Xh, Xw), entry m*B + b = frame b under ``T_ks[m]`` (``Augment_RGB_torch.transform<k>``), centred on the canvas, zero elsewhere.
    ``ks``: distinct, ascending, all even or all odd (odd members are (w, h)); ``out`` receives the batch when given (a slice of a larger one)."""
    _dev(src, out)
    if src.dtype not in (torch.uint8, torch.float32):
        raise UformerHipError("tta_gather: frames must be uint8 or float32")
    B, Cc, h, w = _frame_dims(src, hwc, "tta_gather")
    ks = [int(k) for k in ks]
    shape = (len(ks) * B, Cc, Xh, Xw)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != src.device:
        raise UformerHipError(f"tta_gather: out must be a contiguous float32 tensor of shape {shape} on {src.device}")
    _launch("uf_tta_gather", src.device, _c(src), int(src.dtype == torch.uint8), int(hwc), int(swap_rb), out, (ctypes.c_int * len(ks))(*ks), len(ks),
            B, Cc, h, w, Xh, Xw)
    return out


def tta_merge(even: Optional[Tensor], ks_even, odd: Optional[Tensor], ks_odd, h: int, w: int, u8: bool = False, hwc: bool = True, swap_rb: bool = False,
              clamp: bool = True, out: Optional[Tensor] = None) -> Tensor:
    """The mean of the restored members, each turned back: ``even`` (len(ks_even)*B, C, Xh, Xw) holds the even-k outputs, ``odd``
    (len(ks_odd)*B, C, Xoh, Xow) the odd-k ones (either may be None with an empty list); the balanced pairwise sum in ascending k times 1/n, f32,
    one launch.  f32 planes (B,C,h,w), clamped to [0,1] with ``clamp``; ``u8``: uint8 frames (B,h,w,C) (``hwc``) or (B,C,h,w) through
    canvas_to_frames' quantiser."""
    _dev(even, odd, out)
    ks_even, ks_odd = [int(k) for k in ks_even], [int(k) for k in ks_odd]
    ref = even if even is not None else odd
    if ref is None or (even is None) != (not ks_even) or (odd is None) != (not ks_odd):
        raise UformerHipError("tta_merge: a member buffer goes with a non-empty list of its transforms, and one of the two is needed")
    n, Cc = ref.shape[0], ref.shape[1]
    nk = len(ks_even) if even is not None else len(ks_odd)
    B = n // nk
    for t, ks in ((even, ks_even), (odd, ks_odd)):
        if t is not None and (t.dim() != 4 or tuple(t.shape[:2]) != (len(ks) * B, Cc)):
            raise UformerHipError(f"tta_merge: {tuple(t.shape)} is no batch of {len(ks)} members of {B} images with {Cc} channels")
    if u8:
        res = _u8_frames(B, Cc, h, w, hwc, ref.device, out, "tta_merge")
    elif out is None:
        res = torch.empty((B, Cc, h, w), dtype=torch.float32, device=ref.device)
    else:
        if out.dtype != torch.float32 or tuple(out.shape) != (B, Cc, h, w) or not out.is_contiguous() or out.device != ref.device:
            raise UformerHipError(f"tta_merge: out must be a contiguous float32 tensor of shape {(B, Cc, h, w)} on {ref.device}")
        res = out
    Xh, Xw = (even.shape[2], even.shape[3]) if even is not None else (0, 0)
    Xoh, Xow = (odd.shape[2], odd.shape[3]) if odd is not None else (0, 0)
    _launch("uf_tta_merge", ref.device, None if even is None else _c(even, torch.float32), (ctypes.c_int * max(1, len(ks_even)))(*ks_even), len(ks_even), Xh, Xw,
            None if odd is None else _c(odd, torch.float32), (ctypes.c_int * max(1, len(ks_odd)))(*ks_odd), len(ks_odd), Xoh, Xow,
            res, int(u8), int(hwc), int(swap_rb), int(clamp), B, Cc, h, w)
    return res


def mixup(x: Tensor, lam: Tensor, perm: Tensor) -> Tensor:
    """lam[b] x[b] + (1 - lam[b]) x[perm[b]] (utils/dataset_utils.py:44-53)."""
    _dev(x, lam, perm)
    x = _c(x, torch.float32)
    B = x.shape[0]
    out = torch.empty_like(x)
    _launch("uf_mixup", x.device, x, out, _f32(lam.reshape(-1)), _c(perm, torch.int32), B, x.numel() // B)
    return out


# ---------------------------------------------------------------------------------------
# a15: reductions / patch gathers of the backward, fused training forward of a block
# ---------------------------------------------------------------------------------------
def rows_sum(x: Tensor) -> Tensor:
    """f32 (N,) = sum over the rows of x (M, N) (bf16 / f32), fixed order (modulator gradient: x = d(xn) as (n_windows, 64*C))."""
    _dev(x)
    dt = uf_dtype(x.dtype)
    x = _c(x)
    M, N = x.shape
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    _launch("uf_rows_sum", x.device, x, N, out, M, N, dt, *_workspace("uf_rows_sum_workspace_bytes", x.device, M, N))
    return out


def lewin_block_bwd_workspace_bytes(B: int, H: int, W: int, C: int, heads: int, dtype) -> int:
    return int(_lib.load().uf_lewin_block_bwd_workspace_bytes(B, H, W, C, heads, uf_dtype(dtype)))


def _block_grads(C: int, heads: int, modulator: bool, device):
    """One flat f32 buffer holding all parameter gradients of a block, its uf_block_grads view and {field: tensor view}."""
    shapes = [("norm1_w", (C,)), ("norm1_b", (C,)), ("norm2_w", (C,)), ("norm2_b", (C,)), ("modulator", (64, C) if modulator else None),
              ("rpb_table", (225, heads)), ("wqkv", (3 * C, C)), ("bqkv", (3 * C,)), ("wproj", (C, C)), ("bproj", (C,)), ("w1", (4 * C, C)), ("b1", (4 * C,)),
              ("wdw", (4 * C, 1, 3, 3)), ("bdw", (4 * C,)), ("w2", (C, 4 * C)), ("b2", (C,))]
    total = 0
    offs = {}
    for name, shp in shapes:
        if shp is None:
            continue
        n = 1
        for d in shp:
            n *= d
        offs[name] = (total, n, shp)
        total += (n + 63) // 64 * 64                          # 256-byte aligned pieces
    flat = torch.empty(total, dtype=torch.float32, device=device)
    views = {name: flat[o:o + n].view(shp) for name, (o, n, shp) in offs.items()}
    g = _lib.BlockGrads()
    for name, _ in shapes:
        setattr(g, name, views[name].data_ptr() if name in views else None)
    return flat, g, views


def lewin_block_bwd(tp, x: Tensor, dy: Tensor, drop_attn: Optional[Tensor], drop_leff: Optional[Tensor], B: int, H: int, W: int, heads: int, dtype,
                    ws: Optional[Tensor] = None, half: str = "block"):
    """Recomputation + backward of one LeWin block through uf_lewin_block_bwd (``half``: "block", or "leff" / "attn" for the two
    halves: x is then x1 resp. the block input and dy the gradient of that half's output).  tp: _lib.BlockTrainParams.
    Returns (dx f32 (B*H*W, C), {uf_block_grads field: f32 gradient tensor})."""
    _dev(x, dy)
    x, dy = _c(x, torch.float32), _c(dy, torch.float32)
    C = x.shape[-1]
    dt = uf_dtype(dtype)
    nbytes = _lib.load().uf_lewin_block_bwd_workspace_bytes(B, H, W, C, heads, dt)
    if ws is None or ws.numel() < nbytes:
        ws = _ws(nbytes, x.device)
    _flat, g, views = _block_grads(C, heads, bool(tp.modulator), x.device)
    dx = torch.empty_like(x)
    da, dl = _f32(drop_attn), _f32(drop_leff)
    if half == "block":
        name, drops = "uf_lewin_block_bwd", (da, dl)
    elif half == "leff":
        name, drops = "uf_leff_bwd", (dl,)
    else:
        name, drops = "uf_lewin_attn_bwd", (da,)
    _launch(name, x.device, ctypes.byref(tp), x, dy, dx, *drops, ctypes.byref(g), B, H, W, C, dt, ws, ws.numel())
    if half != "block":       # a half writes only its own parameters' gradients: never hand out the other half's uninitialised views
        mine = {"leff": ("norm2_w", "norm2_b", "w1", "b1", "wdw", "bdw", "w2", "b2"),
                "attn": ("norm1_w", "norm1_b", "modulator", "rpb_table", "wqkv", "bqkv", "wproj", "bproj")}[half]
        views = {k: v for k, v in views.items() if k in mine}
    return dx, views


def downsample_bwd(x: Tensor, dy: Tensor, w_pk_t: Tensor, B: int, H: int, W: int, add_to: Optional[Tensor] = None):
    """Backward of Downsample (Conv2d k4 s2 p1): x f32 rows (B*H*W, Cin) (row stride may exceed Cin), dy f32 (B*H/2*W/2, Cout),
    w_pk_t T (16 Cin, Cout).  Returns (dx -- ``add_to`` accumulated in place when given --, dW_pk f32 (Cout, 16 Cin) packed order, db)."""
    _dev(x, dy, w_pk_t)
    dy = _c(dy, torch.float32)
    Cin, Cout = x.shape[1], dy.shape[1]
    if x.stride(1) != 1:
        x = x.contiguous()
    dt = uf_dtype(w_pk_t.dtype)
    dx = add_to if add_to is not None else torch.empty(B * H * W, Cin, dtype=torch.float32, device=x.device)
    dW = torch.empty(Cout, 16 * Cin, dtype=torch.float32, device=x.device)
    db = torch.empty(Cout, dtype=torch.float32, device=x.device)
    _launch("uf_downsample_bwd", x.device, x, x.stride(0), dy, _c(w_pk_t), dx, dx.stride(0), int(add_to is not None), dW, db, B, H, W, Cin, Cout, dt,
            *_workspace("uf_downsample_bwd_workspace_bytes", x.device, B, H, W, Cin, Cout, dt))
    return dx, dW, db


def upsample_cat_bwd(d: Tensor, x: Tensor, w_pk_t: Tensor, B: int, H: int, W: int):
    """Backward of Upsample (ConvTranspose2d k2 s2) from the gradient ``d`` (B*2H*2W, ld) of the concat buffer whose first Cout columns
    it wrote; x f32 (B*H*W, Cin); w_pk_t T (Cin, 4 Cout).  Returns (dx f32 (B*H*W, Cin), dW_pk f32 (4 Cout, Cin) packed order, db)."""
    _dev(d, x, w_pk_t)
    x = _c(x, torch.float32)
    if d.stride(1) != 1 or d.dtype != torch.float32:
        d = d.float().contiguous()
    Cin, Cout = x.shape[1], w_pk_t.shape[1] // 4
    dt = uf_dtype(w_pk_t.dtype)
    dx = torch.empty(B * H * W, Cin, dtype=torch.float32, device=x.device)
    dW = torch.empty(4 * Cout, Cin, dtype=torch.float32, device=x.device)
    db = torch.empty(Cout, dtype=torch.float32, device=x.device)
    _launch("uf_upsample_cat_bwd", x.device, d, d.stride(0), x, Cin, _c(w_pk_t), dx, dW, db, B, H, W, Cin, Cout, dt,
            *_workspace("uf_upsample_cat_bwd_workspace_bytes", x.device, B, H, W, Cin, Cout, dt))
    return dx, dW, db


def conv3x3_bwd(x: Tensor, dy_rows: Tensor, w: Tensor, B: int, H: int, W: int, nchw: bool = False, act_out: Optional[Tensor] = None, slope: float = 0.01,
                need_dx: bool = True) -> Tuple[Optional[Tensor], Tensor, Tensor]:
    """(dx, dW, db) of a 3x3 stride-1 pad-1 Conv2d with few channels on one side (OutputProj: Cout <= 4; InputProj: Cin <= 8; Cin * Cout * 9 <= 2304):
    x = f32 token rows (B*H*W, Cin) or the NCHW image when ``nchw``; dy_rows f32 (B*H*W, Cout); ``act_out``: the stored LeakyReLU output rows (InputProj)."""
    _dev(x, dy_rows, w)
    x, dy_rows, w = _c(x, torch.float32), _c(dy_rows, torch.float32), _c(w, torch.float32)
    Cout, Cin = w.shape[0], w.shape[1]
    dx = torch.empty_like(x) if need_dx else None
    dW, db = torch.empty_like(w), torch.empty(Cout, dtype=torch.float32, device=x.device)
    _launch("uf_conv3x3_bwd", x.device, x, int(nchw), dy_rows, _f32(act_out), slope, w, dx, dW, db, B, H, W, Cin, Cout,
            *_workspace("uf_conv3x3_bwd_workspace_bytes", x.device, B, H, W, Cin, Cout))
    return dx, dW, db


def residual_combine(a: Optional[Tensor], b: Tensor, scale: Optional[Tensor], B: int, H: int, W: int, windowed: bool = False, shift: int = 0) -> Tensor:
    """f32 (B*H*W, C) = (a or 0) + scale[image] * b; b (bf16/f32 rows) is in WINDOW order when ``windowed`` (window_reverse + roll
    back folded in), ``scale`` = f32 (B,) DropPath scales or None."""
    _dev(b)
    b = _c(b)
    C = b.shape[-1]
    out = torch.empty(B * H * W, C, dtype=torch.float32, device=b.device)
    _launch("uf_residual_combine", b.device, _f32(a), b, int(b.dtype == torch.float32), out, _f32(scale), B, H, W, C, int(windowed), shift, uf_dtype(b.dtype))
    return out


def grad_fork(g1: Tensor, g2: Optional[Tensor], scale: Optional[Tensor], B: int, H: int, W: int, dtype, windowed: bool = False, shift: int = 0,
              want_sum: bool = False) -> Tuple[Optional[Tensor], Tensor]:
    """t = g1 (+ g2) (f32 raster rows); returns (t if ``want_sum`` else None, (t * scale[image]) cast to ``dtype``, in window order
    when ``windowed``)."""
    _dev(g1)
    g1 = _c(g1, torch.float32)
    C = g1.shape[-1]
    tot = torch.empty_like(g1) if want_sum else None
    out = torch.empty(B * H * W, C, dtype=dtype, device=g1.device)
    _launch("uf_grad_fork", g1.device, g1, _f32(g2), tot, out, _f32(scale), B, H, W, C, int(windowed), shift, uf_dtype(dtype))
    return tot, out


def qkv_grad_merge(dq: Tensor, dk: Tensor, dvt: Tensor, heads: int) -> Tensor:
    """(n_windows*64, 3C) gradient of the fused q|k|v projection output from uf_window_attention_bwd's per-head tensors."""
    _dev(dq)
    dq, dk, dvt = _c(dq), _c(dk), _c(dvt)
    hd = dq.shape[-1]
    nW = dq.numel() // (heads * 64 * hd)
    out = torch.empty(nW * 64, 3 * heads * hd, dtype=dq.dtype, device=dq.device)
    _launch("uf_qkv_grad_merge", dq.device, dq, dk, dvt, out, nW, heads, hd, uf_dtype(dq.dtype))
    return out


def rpb_table_grad(dbias: Tensor) -> Tensor:
    """(heads,64,64) dense bias gradient -> (225, heads) relative_position_bias_table gradient (model.py:500-502 transposed)."""
    _dev(dbias)
    dbias = _c(dbias, torch.float32)
    heads = dbias.shape[0]
    out = torch.empty(225, heads, dtype=torch.float32, device=dbias.device)
    _launch("uf_rpb_table_grad", dbias.device, dbias, out, heads)
    return out


def im2col(x: Tensor, B: int, H: int, W: int, Cin: int, k: int, stride: int, pad: int, dtype, nchw: bool = False) -> Tensor:
    """Patch matrix (B*Ho*Wo, ldc) of a conv input: f32 token rows (B*H*W, Cin) or an NCHW image; column (ky*k+kx)*Cin + c,
    ldc = k*k*Cin rounded up to 8 (zero columns)."""
    _dev(x)
    x = _c(x, torch.float32)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ldc = (k * k * Cin + 7) // 8 * 8
    dt = uf_dtype(dtype)
    cols = torch.empty((B * Ho * Wo, ldc), dtype=torch_dtype(dt), device=x.device)
    _launch("uf_im2col", x.device, x, Cin, cols, ldc, B, H, W, Cin, k, stride, pad, int(nchw), dt)
    return cols


def col2im(dcols: Tensor, B: int, H: int, W: int, Cin: int, k: int, stride: int, pad: int, nchw: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """Transpose of im2col: f32 (B*H*W, Cin) rows (or NCHW) = gathered sum of the matching dcols entries; ``out`` given: added to it."""
    _dev(dcols, out)
    dt = uf_dtype(dcols.dtype)
    dcols = _c(dcols)
    acc = out is not None
    if out is None:
        out = torch.empty((B, Cin, H, W) if nchw else (B * H * W, Cin), dtype=torch.float32, device=dcols.device)
    elif not out.is_contiguous() or out.dtype != torch.float32:
        raise UformerHipError("col2im: out must be contiguous float32")
    _launch("uf_col2im", dcols.device, dcols, dcols.shape[1], out, Cin, B, H, W, Cin, k, stride, pad, int(nchw), int(acc), dt)
    return out


def lewin_block_train_fwd(bp, x: Tensor, B: int, H: int, W: int, dtype, drop_attn: Optional[Tensor] = None, drop_leff: Optional[Tensor] = None) -> Tensor:
    """Training forward of one LeWin block on the two fused inference kernels with DropPath scales (f32 (B,) per branch or None):
    returns the new stream; ``x`` (f32 (B*H*W, C)) is left untouched -- it is what the backward keeps."""
    _dev(x, drop_attn, drop_leff)
    dt = uf_dtype(dtype)
    y = _c(x, torch.float32).clone()
    Cc = y.shape[-1]
    _launch("uf_lewin_block_train_fwd", y.device, bp, y, Cc, B, H, W, Cc, _f32(drop_attn), _f32(drop_leff), dt,
            *_workspace("uf_block_workspace_bytes", y.device, B * H * W, Cc, dt))
    return y
