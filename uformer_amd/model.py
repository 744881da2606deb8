"""Drop-in ``Uformer(nn.Module)`` whose hot path runs in ``libuformer_hip.so`` (gfx950).

Boundary kept identical to the reference:
  * constructor kwargs of ``Uformer``                         model.py:1070-1077
  * ``forward(x, mask=None)`` on (B, dd_in, H, W) float       model.py:1269-1305
  * ``state_dict()`` key names / shapes / dtypes / order      SURVEY.md Appendix C
so reference checkpoints (with or without the ``module.`` prefix) load with ``strict=True``.

The sub-modules below carry the reference's names and parameter layout; their ``forward``
methods call the C ABI through ``uformer_amd.ops``.  ``torch.nn`` containers are used only to
HOLD parameters (so init, ``state_dict`` and optimizers behave as in the reference): no ATen
math runs on the hot path, and there is no CPU / eager fallback -- CPU inputs raise.

``compute_dtype`` selects the GEMM operand type: ``torch.bfloat16`` (MFMA bf16, f32 accumulate; BASELINE's headline type),
``torch.float16`` (IEEE half operands, the reference's own AMP type, train/train_denoise.py:180-184: the same MFMA rate and
within the 1e-3 output tolerance; train it under a loss scale as the reference does) or ``torch.float32`` (exact-f32 MFMA).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops, packing
from ._lib import UformerHipError
from .spec import MAX_IN_CHANS, STAGES, UformerConfig, check_image_chans, relative_position_index
from .train import block_hw

Tensor = torch.Tensor
HW = Optional[Tuple[int, int]]    # (H, W) of a token map; the module forwards take it as the keyword ``hw`` (None: the square side of L)


def window_partition(x: Tensor, win_size: int, dilation_rate: int = 1) -> Tensor:
    """model.py:704-715 (dilated branch is dead code in the reference and not provided)."""
    if dilation_rate != 1:
        raise NotImplementedError("dilation_rate != 1 is never exercised by the reference (SURVEY.md section 2 row 1)")
    return ops.window_partition(x, win_size, 0)


def window_reverse(windows: Tensor, win_size: int, H: int, W: int, dilation_rate: int = 1) -> Tensor:
    """model.py:717-726."""
    if dilation_rate != 1:
        raise NotImplementedError("dilation_rate != 1 is never exercised by the reference")
    return ops.window_reverse(windows, win_size, H, W, 0)


def _to_compute(t: Tensor, dtype: torch.dtype) -> Tensor:
    return t.detach().to(dtype).contiguous()


class LinearProjection(nn.Module):
    """model.py:421-447.  Parameters ``to_q`` (C,C) and ``to_kv`` (2C,C)."""

    def __init__(self, dim, heads=8, dim_head=64, dropout=0., bias=True):
        super().__init__()
        inner_dim = dim_head * heads
        self.heads = heads
        self.to_q = nn.Linear(dim, inner_dim, bias=bias)
        self.to_kv = nn.Linear(dim, inner_dim * 2, bias=bias)
        self.dim = dim
        self.inner_dim = inner_dim

    def packed(self, dtype):
        w = torch.cat([self.to_q.weight.detach(), self.to_kv.weight.detach()], 0).to(dtype).contiguous()
        b = torch.cat([self.to_q.bias.detach(), self.to_kv.bias.detach()], 0).float().contiguous()
        return w, b

    def flops(self, q_L, kv_L=None):
        kv_L = kv_L or q_L
        return q_L * self.dim * self.inner_dim + kv_L * self.dim * self.inner_dim * 2


CONV_PROJECTION_WIDTHS = (16, 32, 64, 128, 256, 512)     # uf_ln_convqkv_fwd


class SepConv2d(nn.Module):
    """model.py:344-378: depthwise conv -> ReLU -> pointwise 1x1 conv.  Holds the parameters; inside a block the three of a ConvProjection
    run in one ``uf_ln_convqkv_fwd`` launch."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, act_layer=nn.ReLU):
        super().__init__()
        if kernel_size != 3 or stride != 1 or padding != 1 or dilation != 1 or act_layer is not nn.ReLU:
            raise NotImplementedError("SepConv2d: only the configuration ConvProjection builds (3x3, stride 1, padding 1, ReLU; model.py:389-392)")
        self.depthwise = nn.Conv2d(in_channels, in_channels, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation,
                                   groups=in_channels)
        self.pointwise = nn.Conv2d(in_channels, out_channels, kernel_size=1)
        self.act_layer = act_layer()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        self.stride = stride

    def flops(self, HW):
        return HW * self.in_channels * self.kernel_size ** 2 / self.stride ** 2 + HW * self.in_channels * self.out_channels


class ConvProjection(nn.Module):
    """model.py:381-418 (``token_projection='conv'``): ``to_q``, ``to_k``, ``to_v``, each a SepConv2d over the 8x8 image of one window."""

    def __init__(self, dim, heads=8, dim_head=64, kernel_size=3, q_stride=1, k_stride=1, v_stride=1, dropout=0., last_stage=False, bias=True):
        super().__init__()
        if kernel_size != 3 or (q_stride, k_stride, v_stride) != (1, 1, 1) or not bias:
            raise NotImplementedError("ConvProjection: 3x3 kernels, stride 1 and biases only (WindowAttention's configuration, model.py:481)")
        inner_dim = dim_head * heads
        if inner_dim != dim:
            raise NotImplementedError("ConvProjection: heads * dim_head must equal dim (model.py:481)")
        self.heads = heads
        pad = (kernel_size - q_stride) // 2
        self.to_q = SepConv2d(dim, inner_dim, kernel_size, q_stride, pad)
        self.to_k = SepConv2d(dim, inner_dim, kernel_size, k_stride, pad)
        self.to_v = SepConv2d(dim, inner_dim, kernel_size, v_stride, pad)
        self.dim = dim
        self.inner_dim = inner_dim

    def flops(self, q_L, kv_L=None):
        kv_L = kv_L or q_L
        return self.to_q.flops(q_L) + self.to_k.flops(kv_L) + self.to_v.flops(kv_L)


class WindowAttention(nn.Module):
    """model.py:452-546; ``token_projection`` 'linear' (every get_arch architecture) or 'conv' (ConvProjection; 8x8 windows, inference inside a
    LeWinTransformerBlock, where it runs fused behind norm1: uf_ln_convqkv_fwd)."""

    def __init__(self, dim, win_size, num_heads, token_projection='linear', qkv_bias=True, qk_scale=None,
                 attn_drop=0., proj_drop=0.):
        super().__init__()
        if token_projection not in ('linear', 'conv'):
            raise NotImplementedError(f"token_projection={token_projection!r}: 'linear' and 'conv' are built (model.py:480-485)")
        if token_projection == 'conv' and (tuple(win_size) != (8, 8) or dim not in CONV_PROJECTION_WIDTHS or dim % num_heads
                                           or dim // num_heads not in (16, 32, 64)):
            raise NotImplementedError(f"token_projection='conv' is built for 8x8-window blocks of width 16 ... 512 with head_dim 16, 32 or 64 "
                                      f"(uf_ln_convqkv_fwd); this block has width {dim}, {num_heads} heads and window {tuple(win_size)} (img_size 64 "
                                      f"and embed_dim 64 take token_projection='linear' only)")
        if qk_scale is not None or attn_drop or proj_drop:
            raise NotImplementedError("qk_scale / attention dropout are never set by the reference archs")
        self.dim = dim
        self.win_size = tuple(win_size)
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim ** -0.5
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((2 * self.win_size[0] - 1) * (2 * self.win_size[1] - 1), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(self.win_size[0]))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        if token_projection == 'conv':
            self.qkv = ConvProjection(dim, num_heads, dim // num_heads, bias=qkv_bias)
        else:
            self.qkv = LinearProjection(dim, num_heads, dim // num_heads, bias=qkv_bias)
        self.token_projection = token_projection
        self.proj = nn.Linear(dim, dim)

    def forward(self, x: Tensor, attn_kv=None, mask: Optional[Tensor] = None, *, H: Optional[int] = None,
                W: Optional[int] = None, shift: int = 0, compute_dtype=torch.float32) -> Tensor:
        """x: (B_, 64, C) window tokens (B_, 16, C at win_size 4).  ``mask`` (nW,64,64) additive, as in model.py:508-512."""
        if attn_kv is not None:
            raise NotImplementedError("attn_kv (cross-modulator) is out of scope: never enabled by get_arch")
        if self.token_projection == 'conv':
            raise NotImplementedError("token_projection='conv': the ConvProjection runs fused behind norm1 (uf_ln_convqkv_fwd); call the "
                                      "LeWinTransformerBlock, there is no stand-alone WindowAttention forward for it")
        B_, N, Cc = x.shape
        if self.win_size == (4, 4):
            if mask is not None or shift:
                raise NotImplementedError("4x4-window attention takes no mask and no shift (the reference clamps the shift to 0, model.py:863-866)")
            if N != 16:
                raise UformerHipError("4x4-window attention needs 16 tokens per window")
            a = _to_compute(x.reshape(B_ * N, Cc), compute_dtype)
            wqkv, bqkv = self.qkv.packed(compute_dtype)
            qkv = ops.linear(a, wqkv, bqkv)
            # every window is a 4x4 "image" of its own: window-row order = raster order
            o = ops.window4_attention(qkv, packing.pack_rpb_table4(self.relative_position_bias_table, self.relative_position_index), B_, 4, 4,
                                      self.num_heads)
            y = ops.linear(o, _to_compute(self.proj.weight, compute_dtype), self.proj.bias.detach().float(), 0)
            return y.reshape(B_, N, Cc).to(x.dtype)
        if N != 64:
            raise UformerHipError("window attention needs 8x8 = 64 tokens per window")
        if H is None or W is None:  # any geometry with the right window count serves a dense mask
            H, W = 8, 8 * B_
            if shift:
                raise UformerHipError("analytic shift mask needs H and W")
        a = _to_compute(x.reshape(B_ * N, Cc), compute_dtype)
        wqkv, bqkv = self.qkv.packed(compute_dtype)
        q, k, vt = ops.qkv(a, wqkv, bqkv, self.num_heads)
        bias = packing.rpb_dense(self.relative_position_bias_table, self.relative_position_index)
        o = ops.window_attention_core(q, k, vt, bias, H=H, W=W, shift=shift, mask=mask)
        y = ops.linear(o, _to_compute(self.proj.weight, compute_dtype), self.proj.bias.detach().float(), 0)
        return y.reshape(B_, N, Cc).to(x.dtype)

    def extra_repr(self) -> str:
        return f'dim={self.dim}, win_size={self.win_size}, num_heads={self.num_heads}'

    def flops(self, H, W):
        N = self.win_size[0] * self.win_size[1]
        nW = H * W / N
        flops = self.qkv.flops(H * W, H * W)     # ConvProjection: + 27 depthwise taps per token and channel (model.py:373-377, :412-418)
        flops += nW * self.num_heads * N * (self.dim // self.num_heads) * N * 2
        flops += nW * N * self.dim * self.dim
        return flops


CROSS_MODULATOR_WIDTHS = (16, 32, 64, 128, 256, 512)      # uf_cross_attn_fwd


class Attention(nn.Module):
    """model.py:549-621: the ``cross_attn`` of a block built with ``cross_modulator=True``.  Holds the parameters (a LinearProjection whatever
    ``token_projection`` says, model.py:558, and ``proj``; no relative-position table); inside a LeWinTransformerBlock it runs as one
    ``uf_cross_attn_fwd`` launch against the block's 64 ``cross_modulator`` tokens."""

    def __init__(self, dim, num_heads, token_projection='linear', qkv_bias=True, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        if qk_scale is not None or attn_drop or proj_drop:
            raise NotImplementedError("qk_scale / attention dropout are never set by the reference archs")
        if dim not in CROSS_MODULATOR_WIDTHS or dim % num_heads or dim // num_heads not in (16, 32):
            raise NotImplementedError(f"cross_modulator is built for blocks of width 16 ... 512 with head_dim 16 or 32 (uf_cross_attn_fwd); this block "
                                      f"has width {dim} and {num_heads} heads (embed_dim 64 gives head_dim 64)")
        self.dim = dim
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = LinearProjection(dim, num_heads, dim // num_heads, bias=qkv_bias)
        self.token_projection = token_projection
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, attn_kv=None, mask=None):
        raise NotImplementedError("cross_modulator: the cross attention runs fused inside its block (uf_cross_attn_fwd); call the "
                                  "LeWinTransformerBlock, there is no stand-alone Attention forward")

    def extra_repr(self) -> str:
        return f'dim={self.dim}, num_heads={self.num_heads}'

    def flops(self, q_num, kv_num):
        """model.py:600-618 (without its print)."""
        return self.qkv.flops(q_num, kv_num) + 2 * self.num_heads * q_num * (self.dim // self.num_heads) * kv_num + q_num * self.dim * self.dim


class LeFF(nn.Module):
    """model.py:654-699."""

    def __init__(self, dim=32, hidden_dim=128, act_layer=nn.GELU, drop=0., use_eca=False):
        super().__init__()
        if use_eca or act_layer is not nn.GELU:
            raise NotImplementedError("LeFF is built with GELU and without ECA by every reference arch")
        self.linear1 = nn.Sequential(nn.Linear(dim, hidden_dim), act_layer())
        self.dwconv = nn.Sequential(nn.Conv2d(hidden_dim, hidden_dim, groups=hidden_dim, kernel_size=3, stride=1, padding=1),
                                    act_layer())
        self.linear2 = nn.Sequential(nn.Linear(hidden_dim, dim))
        self.dim = dim
        self.hidden_dim = hidden_dim

    def forward(self, x: Tensor, compute_dtype=torch.float32, *, hw: HW = None) -> Tensor:
        bs, L, c = x.shape
        H, W = block_hw(L, hw, "LeFF")
        a = _to_compute(x.reshape(bs * L, c), compute_dtype)
        h1 = ops.linear(a, _to_compute(self.linear1[0].weight, compute_dtype), self.linear1[0].bias.detach().float(), 1)
        h2 = ops.dwconv3x3_gelu(h1.reshape(bs, H, W, self.hidden_dim), packing.pack_dwconv(self.dwconv[0].weight),
                                self.dwconv[0].bias.detach().float())
        y = ops.linear(h2.reshape(bs * L, self.hidden_dim), _to_compute(self.linear2[0].weight, compute_dtype),
                       self.linear2[0].bias.detach().float(), 0)
        return y.reshape(bs, L, c).to(x.dtype)

    def flops(self, H, W):
        return H * W * self.dim * self.hidden_dim + H * W * self.hidden_dim * 9 + H * W * self.hidden_dim * self.dim


class Mlp(nn.Module):
    """model.py:623-651: fc1 -> GELU -> fc2, the block's feed-forward half under ``token_mlp='ffn'`` / ``'mlp'``.  Inside a block the
    whole half (norm2, both Linears, the residual) is one ``uf_ffn_fwd`` launch; this stand-alone forward runs the two GEMMs."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        if act_layer is not nn.GELU or drop:
            raise NotImplementedError("Mlp is built with GELU and drop=0 (every reference arch)")
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)
        self.in_features = in_features
        self.hidden_features = hidden_features
        self.out_features = out_features

    def forward(self, x: Tensor, compute_dtype=torch.float32, *, hw: HW = None) -> Tensor:
        bs, L, c = x.shape
        a = _to_compute(x.reshape(bs * L, c), compute_dtype)
        h = ops.linear(a, _to_compute(self.fc1.weight, compute_dtype), self.fc1.bias.detach().float(), 1)
        y = ops.linear(h, _to_compute(self.fc2.weight, compute_dtype), self.fc2.bias.detach().float(), 0)
        return y.reshape(bs, L, self.out_features).to(x.dtype)

    def flops(self, H, W):
        return H * W * self.in_features * self.hidden_features + H * W * self.hidden_features * self.out_features


class Downsample(nn.Module):
    """model.py:730-753."""

    def __init__(self, in_channel, out_channel):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_channel, out_channel, kernel_size=4, stride=2, padding=1))
        self.in_channel = in_channel
        self.out_channel = out_channel

    def forward(self, x: Tensor, compute_dtype=torch.float32, *, hw: HW = None) -> Tensor:
        B, L, Cc = x.shape
        H, W = block_hw(L, hw, "Downsample")
        y = ops.downsample(x.reshape(B * L, Cc), packing.pack_downsample(self.conv[0].weight, compute_dtype),
                           self.conv[0].bias.detach().float(), B, H, W)
        return y.reshape(B, L // 4, self.out_channel)

    def flops(self, H, W):
        return H / 2 * W / 2 * self.in_channel * self.out_channel * 4 * 4


class Upsample(nn.Module):
    """model.py:756-778."""

    def __init__(self, in_channel, out_channel):
        super().__init__()
        self.deconv = nn.Sequential(nn.ConvTranspose2d(in_channel, out_channel, kernel_size=2, stride=2))
        self.in_channel = in_channel
        self.out_channel = out_channel

    def forward(self, x: Tensor, compute_dtype=torch.float32, *, hw: HW = None) -> Tensor:
        B, L, Cc = x.shape
        H, W = block_hw(L, hw, "Upsample")
        y = ops.upsample(x.reshape(B * L, Cc), packing.pack_upsample(self.deconv[0].weight, compute_dtype),
                         self.deconv[0].bias.detach().float(), B, H, W)
        return y.reshape(B, 4 * L, self.out_channel)

    def flops(self, H, W):
        return H * W * self.in_channel * self.out_channel   # exact (the reference over-counts 4x, model.py:776)


class InputProj(nn.Module):
    """model.py:781-811."""

    def __init__(self, in_channel=3, out_channel=64, kernel_size=3, stride=1, norm_layer=None, act_layer=nn.LeakyReLU):
        super().__init__()
        if norm_layer is not None or kernel_size != 3 or stride != 1 or act_layer is not nn.LeakyReLU:
            raise NotImplementedError("InputProj: only the configuration Uformer builds (model.py:1100)")
        if in_channel < 1:
            raise NotImplementedError(f"InputProj: in_channel={in_channel}")
        self.proj = nn.Sequential(nn.Conv2d(in_channel, out_channel, kernel_size=3, stride=stride, padding=kernel_size // 2),
                                  act_layer(inplace=True))
        self.in_channel = in_channel
        self.out_channel = out_channel

    def forward(self, x: Tensor) -> Tensor:
        B, Cc, H, W = x.shape
        y = ops.input_proj(x, packing.pack_input_proj(self.proj[0].weight), self.proj[0].bias.detach().float())
        return y.reshape(B, H * W, self.out_channel)

    def flops(self, H, W):
        return H * W * self.in_channel * self.out_channel * 9


class OutputProj(nn.Module):
    """model.py:814-846."""

    def __init__(self, in_channel=64, out_channel=3, kernel_size=3, stride=1, norm_layer=None, act_layer=None):
        super().__init__()
        if norm_layer is not None or act_layer is not None or kernel_size != 3 or stride != 1 or not 1 <= out_channel <= MAX_IN_CHANS:
            raise NotImplementedError(f"OutputProj: only the configuration Uformer builds (model.py:1101), out_channel 1..{MAX_IN_CHANS}")
        self.proj = nn.Sequential(nn.Conv2d(in_channel, out_channel, kernel_size=3, stride=stride, padding=kernel_size // 2))
        self.in_channel = in_channel
        self.out_channel = out_channel

    def forward(self, x: Tensor, img: Optional[Tensor] = None, *, hw: HW = None) -> Tensor:
        B, L, Cc = x.shape
        H, W = block_hw(L, hw if hw is not None or img is None else tuple(img.shape[-2:]), "OutputProj")
        return ops.output_proj(x.reshape(B * L, Cc), packing.pack_output_proj(self.proj[0].weight),
                               self.proj[0].bias.detach().float(), B, H, W, img)

    def flops(self, H, W):
        return H * W * self.in_channel * self.out_channel * 9


class LeWinTransformerBlock(nn.Module):
    """model.py:850-1008 (``token_mlp`` 'leff', or 'ffn' / 'mlp' for the reference's Mlp; ``token_projection`` 'linear', or 'conv' for the
    reference's ConvProjection, inference only; ``cross_modulator=True`` adds the
    reference's ``cross_modulator`` / ``cross_attn`` / ``norm_cross``, inference only)."""

    def __init__(self, dim, input_resolution, num_heads, win_size=8, shift_size=0, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop=0., attn_drop=0., drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm,
                 token_projection='linear', token_mlp='leff', modulator=False, cross_modulator=False):
        super().__init__()
        if token_mlp not in ('leff', 'ffn', 'mlp'):
            raise NotImplementedError(f"token_mlp={token_mlp!r}: 'leff' and 'ffn' / 'mlp' are built ('fastleff' needs a third-party CUDA package, "
                                      "model.py:895-896)")
        if norm_layer is not nn.LayerNorm or drop:
            raise NotImplementedError("LayerNorm / drop=0 only")
        self.dim = dim
        self.input_resolution = tuple(input_resolution)
        self.num_heads = num_heads
        self.win_size = win_size
        self.shift_size = shift_size
        self.mlp_ratio = mlp_ratio
        self.token_mlp = token_mlp
        self.token_projection = token_projection
        if min(self.input_resolution) <= self.win_size:   # model.py:863-866
            self.shift_size = 0
            self.win_size = min(self.input_resolution)
        assert 0 <= self.shift_size < self.win_size, "shift_size must in 0-win_size"
        # built: window 8, and window 4 clamped from 8 (the bottleneck of a model built for 64x64 patches)
        if win_size != 8 or self.win_size not in (4, 8):
            raise NotImplementedError(f"the HIP path is built for win_size 8 and for a window clamped to 4; this block would need window "
                                      f"{self.win_size} (input_resolution {tuple(self.input_resolution)}, win_size {win_size})")
        if self.win_size == 4 and modulator:
            raise NotImplementedError("a 4x4-window block with a modulator: the reference's (64, C) embedding (model.py:868-869) does not broadcast "
                                      "onto 16-token windows (model.py:967-969)")
        self.modulator = nn.Embedding(win_size * win_size, dim) if modulator else None
        if cross_modulator:                     # model.py:873-877, registered between modulator and norm1
            if self.win_size != 8:
                raise NotImplementedError("cross_modulator is built for 8x8-window blocks (img_size 64 clamps the bottleneck's window to 4)")
            self.cross_modulator = nn.Embedding(win_size * win_size, dim)
            self.cross_attn = Attention(dim, num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop,
                                        token_projection=token_projection)
            self.norm_cross = norm_layer(dim)   # in the state_dict, never read: the reference overwrites its output (model.py:947-948)
        else:
            self.cross_modulator = None
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, win_size=(self.win_size, self.win_size), num_heads=num_heads, qkv_bias=qkv_bias,
                                    qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop, token_projection=token_projection)
        self.drop_path_rate = float(drop_path)
        self.norm2 = norm_layer(dim)
        if token_mlp == 'leff':
            self.mlp = LeFF(dim, int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        else:                                   # model.py:890-891
            if self.win_size == 4 or dim > 512 or dim not in (16, 32, 64, 128, 256, 512):
                raise NotImplementedError(f"token_mlp={token_mlp!r} is built for 8x8-window blocks of width 16 ... 512 (uf_ffn_fwd); this block has "
                                          f"width {dim} and window {self.win_size} (img_size 64 and embed_dim 64 take token_mlp='leff' only)")
            self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self._packed = None
        self._packed_cross = None

    def extra_repr(self) -> str:
        return (f"dim={self.dim}, input_resolution={self.input_resolution}, num_heads={self.num_heads}, "
                f"win_size={self.win_size}, shift_size={self.shift_size}, mlp_ratio={self.mlp_ratio}")

    def _pack(self, dtype):
        sd = {k: v for k, v in self.state_dict(keep_vars=True).items()}
        key = (dtype, tuple((v.data_ptr(), v._version) for v in sd.values()))
        if self._packed is None or self._packed[0] != key:
            if self.win_size == 4:
                bp, keep = packing.pack_block4(sd, "", self.num_heads, dtype)
            else:
                bp, keep = packing.pack_block(sd, "", self.num_heads, self.shift_size, dtype)
            self._packed = (key, bp, keep)
        return self._packed[1]

    def _pack_cross(self, dtype):
        """The ``uf_cross_params`` of this block's cross-modulator, cached by (data_ptr, _version) of the parameters it is made of."""
        sd = {k: v for k, v in self.state_dict(keep_vars=True).items() if k.startswith(("cross_modulator.", "cross_attn."))}
        key = (dtype, tuple((v.data_ptr(), v._version) for v in sd.values()))
        if self._packed_cross is None or self._packed_cross[0] != key:
            cp, keep = packing.pack_cross(sd, "", self.num_heads, dtype)
            self._packed_cross = (key, cp, keep)
        return self._packed_cross[1]

    def user_attn_mask(self, mask: Tensor, H: int, W: int) -> Tensor:
        """Dense additive mask (B*nW,64,64) from the user ``mask`` argument, model.py:914-921
        (index glue on the GPU: nearest interpolate, partition, outer product, +-100 fill)."""
        m = torch.nn.functional.interpolate(mask.float(), size=(H, W)).permute(0, 2, 3, 1).contiguous()
        mw = ops.window_partition(m, 8, 0).reshape(-1, 64)
        am = mw.unsqueeze(2) * mw.unsqueeze(1)
        return torch.where(am != 0, torch.full_like(am, -100.0), torch.zeros_like(am)).contiguous()

    def forward(self, x: Tensor, mask: Optional[Tensor] = None, compute_dtype=torch.float32, *, hw: HW = None) -> Tensor:
        """(B, L, C) -> (B, L, C); ``hw`` = (H, W) of the map (None: the square side of L).  With grad mode on and something to
        differentiate (train() mode, an input or a parameter that requires grad) the block is an autograd node like the reference's
        (model.py:908-989): op-by-op forward that keeps its intermediates + the op-level backward (uformer_amd.train.LeWinBlockFunction), timm's DropPath per sample in train() mode.
        Otherwise: the fused inference kernels (DropPath is the identity)."""
        if torch.is_grad_enabled() and mask is None and (self.training or x.requires_grad or any(p.requires_grad for p in self.parameters())):
            from . import train
            if self.token_projection == 'conv':
                raise NotImplementedError(train.TOKEN_PROJECTION_TRAINING)
            if self.cross_modulator is not None:
                raise NotImplementedError(train.CROSS_MODULATOR_TRAINING)
            if not x.is_cuda:
                raise UformerHipError("LeWinTransformerBlock runs on the GPU only; there is no CPU path")
            named = [(n, t) for n, t in self.state_dict(keep_vars=True).items()]
            drop = None
            if self.training and self.drop_path_rate > 0.0:
                drop = getattr(self, "_drop_scales_override", None)
                if drop is None:
                    drop = train.sample_drop_scales([self.drop_path_rate], x.shape[0], x.device)
            hw = block_hw(x.shape[1], hw, "LeWinTransformerBlock")
            return train.LeWinBlockFunction.apply(x, [n for n, _ in named], self.num_heads, self.shift_size, compute_dtype, drop, hw,
                                                  *[t for _, t in named])
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError("the mask argument is not supported by the block's autograd path (no reference script passes it)")
        B, L, Cc = x.shape
        H, W = block_hw(L, hw, "LeWinTransformerBlock")
        if not x.is_cuda:
            raise UformerHipError("LeWinTransformerBlock runs on the GPU only; there is no CPU path")
        dt = ops.uf_dtype(compute_dtype)
        y = x.detach().float().contiguous().clone()
        if self.win_size == 4:
            if mask is not None:
                raise NotImplementedError("the mask argument is not supported by 4x4-window blocks (no reference script passes it)")
            with torch.cuda.device(x.device):
                lib = _lib.load()
                nbytes = lib.uf_block_workspace_bytes(B * L, Cc, dt)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
                bp = self._pack(compute_dtype)
                ops._launch("uf_lewin_block4_fwd", x.device, bp, y, Cc, B, H, W, Cc, None, None, dt, ws, nbytes)
            return y.to(x.dtype)
        um = self.user_attn_mask(mask, H, W) if mask is not None else None
        with torch.cuda.device(x.device):
            lib = _lib.load()
            nbytes = lib.uf_block_workspace_bytes(B * L, Cc, dt)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            bp = self._pack(compute_dtype)
            if self.cross_modulator is not None:    # model.py:945-949, on the un-normalised stream, before the attention half
                ops._launch("uf_cross_attn_fwd", x.device, self._pack_cross(compute_dtype), y, Cc, B * L, Cc, dt)
            ops._launch("uf_lewin_block_fwd", x.device, bp, y, Cc, B, H, W, Cc, um, 0 if um is None else um.shape[0], dt, ws, nbytes)
        return y.to(x.dtype)


class BasicUformerLayer(nn.Module):
    """model.py:1013-1066."""

    def __init__(self, dim, output_dim, input_resolution, depth, num_heads, win_size, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop=0., attn_drop=0., drop_path=0., norm_layer=nn.LayerNorm, use_checkpoint=False,
                 token_projection='linear', token_mlp='ffn', shift_flag=True, modulator=False, cross_modulator=False):
        super().__init__()
        if use_checkpoint and token_projection == 'conv':
            from .train import TOKEN_PROJECTION_TRAINING
            raise NotImplementedError("use_checkpoint: " + TOKEN_PROJECTION_TRAINING)
        if use_checkpoint and cross_modulator:
            from .train import CROSS_MODULATOR_TRAINING
            raise NotImplementedError("use_checkpoint: " + CROSS_MODULATOR_TRAINING)
        self.dim = dim
        self.input_resolution = input_resolution
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            LeWinTransformerBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads, win_size=win_size,
                                  shift_size=0 if (i % 2 == 0 or not shift_flag) else win_size // 2,
                                  mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                  drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                                  norm_layer=norm_layer, token_projection=token_projection, token_mlp=token_mlp,
                                  modulator=modulator, cross_modulator=cross_modulator)
            for i in range(depth)])

    def forward(self, x, mask=None, compute_dtype=torch.float32, *, hw: HW = None):
        for blk in self.blocks:
            x = blk(x, None if self.use_checkpoint else mask, compute_dtype, hw=hw)  # checkpoint drops mask, model.py:1057
        return x


class Uformer(nn.Module):
    """model.py:1069-1328.  Same kwargs; extra keyword ``compute_dtype`` (default bf16)."""

    def __init__(self, img_size=256, in_chans=3, dd_in=3, embed_dim=32, depths=[2, 2, 2, 2, 2, 2, 2, 2, 2],
                 num_heads=[1, 2, 4, 8, 16, 16, 8, 4, 2], win_size=8, mlp_ratio=4., qkv_bias=True, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm, patch_norm=True,
                 use_checkpoint=False, token_projection='linear', token_mlp='leff', dowsample=Downsample, upsample=Upsample,
                 shift_flag=True, modulator=False, cross_modulator=False, compute_dtype=torch.bfloat16, **kwargs):
        super().__init__()
        if drop_rate or attn_drop_rate:
            raise NotImplementedError("drop_rate / attn_drop_rate are 0 in every reference arch")
        if dowsample is not Downsample or upsample is not Upsample:
            raise NotImplementedError("custom sampler classes are not supported")
        check_image_chans(dd_in, in_chans)
        self.num_enc_layers = len(depths) // 2
        self.num_dec_layers = len(depths) // 2
        self.embed_dim = embed_dim
        self.patch_norm = patch_norm
        self.mlp_ratio = mlp_ratio
        self.token_projection = token_projection
        self.mlp = token_mlp
        self.win_size = win_size
        self.reso = img_size
        self.dd_in = dd_in
        self.in_chans = in_chans
        self.use_checkpoint = use_checkpoint
        self.compute_dtype = compute_dtype
        self.cfg = UformerConfig(img_size=img_size, in_chans=in_chans, dd_in=dd_in, embed_dim=embed_dim,
                                 depths=tuple(depths), num_heads=tuple(num_heads), win_size=win_size, mlp_ratio=mlp_ratio,
                                 modulator=modulator, shift_flag=shift_flag, token_mlp=token_mlp, token_projection=token_projection,
                                 cross_modulator=bool(cross_modulator))
        bad = self.cfg.unsupported_clamp() if win_size == 8 else None
        if bad is not None:       # model.py:863-866 clamps a stage's window to its resolution; built: 8, and 4 for the bottleneck alone
            s_, res_, win_ = bad
            raise NotImplementedError(f"img_size={img_size}: stage {STAGES[s_]} has resolution {res_}, so the reference would run it on "
                                      f"{win_}x{win_} windows; the HIP path is built for 8x8 windows and, for the bottleneck (conv) alone, 4x4 "
                                      f"(img_size // 16 == 4, e.g. 64)")
        if win_size == 8 and self.cfg.stage_windows()[4] == 4 and (e16 := 16 * embed_dim) // num_heads[4] not in (16, 32):
            # found by tests/test_gpu_switch_matrix.py: the form built and its first forward failed inside uf_uformer_win4_fwd
            raise NotImplementedError(f"embed_dim={embed_dim} with img_size={img_size}: the bottleneck would run 4x4 windows at head_dim "
                                      f"{e16 // num_heads[4]}, and the 4x4-window kernels (uf_win4.hip) are built for head_dim 16 and 32 "
                                      f"(embed_dim 64 takes img_size 128 and up)")
        enc_dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths[:self.num_enc_layers]))]
        conv_dpr = [drop_path_rate] * depths[4]
        dec_dpr = enc_dpr[::-1]

        if cross_modulator and self.cfg.stage_windows()[4] != 8:
            raise NotImplementedError(f"cross_modulator is built for models whose every stage runs on 8x8 windows; img_size={img_size} gives the "
                                      f"bottleneck 4x4 windows (uf_uformer_win4_fwd does not run the cross attention)")
        if cross_modulator and use_checkpoint:
            from .train import CROSS_MODULATOR_TRAINING
            raise NotImplementedError("use_checkpoint: " + CROSS_MODULATOR_TRAINING)

        def layer(s, dim, res, dpr, mod):
            return BasicUformerLayer(dim=dim, output_dim=dim, input_resolution=(res, res), depth=depths[s],
                                     num_heads=num_heads[s], win_size=win_size, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                     qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr,
                                     norm_layer=norm_layer, use_checkpoint=use_checkpoint, token_projection=token_projection,
                                     token_mlp=token_mlp, shift_flag=shift_flag, modulator=mod,
                                     cross_modulator=self.cfg.stage_has_cross_modulator(s))   # decoder stages only, model.py:1196-1245

        e = embed_dim
        self.input_proj = InputProj(in_channel=dd_in, out_channel=e, kernel_size=3, stride=1, act_layer=nn.LeakyReLU)
        self.output_proj = OutputProj(in_channel=2 * e, out_channel=in_chans, kernel_size=3, stride=1)
        self.encoderlayer_0 = layer(0, e, img_size, enc_dpr[sum(depths[:0]):sum(depths[:1])], False)
        self.dowsample_0 = dowsample(e, e * 2)
        self.encoderlayer_1 = layer(1, e * 2, img_size // 2, enc_dpr[sum(depths[:1]):sum(depths[:2])], False)
        self.dowsample_1 = dowsample(e * 2, e * 4)
        self.encoderlayer_2 = layer(2, e * 4, img_size // 4, enc_dpr[sum(depths[:2]):sum(depths[:3])], False)
        self.dowsample_2 = dowsample(e * 4, e * 8)
        self.encoderlayer_3 = layer(3, e * 8, img_size // 8, enc_dpr[sum(depths[:3]):sum(depths[:4])], False)
        self.dowsample_3 = dowsample(e * 8, e * 16)
        self.conv = layer(4, e * 16, img_size // 16, conv_dpr, False)
        self.upsample_0 = upsample(e * 16, e * 8)
        self.decoderlayer_0 = layer(5, e * 16, img_size // 8, dec_dpr[:depths[5]], modulator)
        self.upsample_1 = upsample(e * 16, e * 4)
        self.decoderlayer_1 = layer(6, e * 8, img_size // 4, dec_dpr[sum(depths[5:6]):sum(depths[5:7])], modulator)
        self.upsample_2 = upsample(e * 8, e * 2)
        self.decoderlayer_2 = layer(7, e * 4, img_size // 2, dec_dpr[sum(depths[5:7]):sum(depths[5:8])], modulator)
        self.upsample_3 = upsample(e * 4, e)
        self.decoderlayer_3 = layer(8, e * 2, img_size, dec_dpr[sum(depths[5:8]):sum(depths[5:9])], modulator)
        self.apply(self._init_weights)
        self._packed = None
        self._packed_key = None
        self._ws = None

    def _init_weights(self, m):   # model.py:1249-1256
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'absolute_pos_embed'}

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {'relative_position_bias_table'}

    def extra_repr(self) -> str:
        return (f"embed_dim={self.embed_dim}, token_projection={self.token_projection}, token_mlp={self.mlp},"
                f"win_size={self.win_size}, compute_dtype={self.compute_dtype}")

    # ---- packed weights ------------------------------------------------------------------
    def _apply(self, fn, *a, **k):   # .to() / .cuda() / .half(): parameters are replaced -- packed weights, workspaces and the cached parameter list go
        self._packed = None
        self._ws = None
        self.__dict__.pop("_plist", None)
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts reference checkpoints, including ``{'state_dict': ...}`` payloads and the
        ``module.`` prefix left by nn.DataParallel (utils/model_utils.py:23-33)."""
        if "state_dict" in state_dict and not any(k.startswith("input_proj") for k in state_dict):
            state_dict = state_dict["state_dict"]
        if all(k.startswith("module.") for k in state_dict):
            state_dict = {k[7:]: v for k, v in state_dict.items()}
        self._packed = None
        self.__dict__.pop("_plist", None)
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def repack(self):
        self._packed = None
        self.__dict__.pop("_plist", None)

    def _get_packed(self, device):
        self._check_not_replica()
        # (storage, version) of every parameter: catches in-place updates (optimizer steps bump _version) AND writes through
        # ``p.data`` / ``p.data = ...`` that swap the storage without bumping it (EMA swaps, older optimizers)
        # The parameter LIST is cached (walking the module tree costs 1.1 ms per call for Uformer-B's 719 parameters, the key itself
        # 0.1 ms): Parameter objects survive .to() / load_state_dict() / optimizer steps; replacing one (m.w = nn.Parameter(..)) needs
        # repack(), which also drops this list -- as do _apply() and load_state_dict().
        plist = self.__dict__.get("_plist")
        if plist is None:
            plist = self.__dict__["_plist"] = list(self.parameters())
        key = (self.compute_dtype, str(device), tuple(map(torch.Tensor.data_ptr, plist)), tuple(p._version for p in plist))
        if self._packed is None or self._packed_key != key:
            sd = self.state_dict(keep_vars=True)
            self._packed = packing.PackedModel(self.cfg, sd, self.compute_dtype)
            self._packed_key = key
        return self._packed

    def _check_not_replica(self):
        """nn.DataParallel replicas carry no parameters of their own (``_parameters`` is emptied by ``replicate``) and would
        share the packed weights / workspace of device 0.  The reference wraps the model in nn.DataParallel
        (train/train_denoise.py:83); here multi-GPU is one process per GPU (uformer_amd.dist) -- say so instead of failing
        with a KeyError deep inside the packing code."""
        if getattr(self, "_is_replica", False):
            raise UformerHipError("uformer_amd.Uformer cannot run as an nn.DataParallel replica: launch one process per GPU "
                                  "(torch.distributed.run, uformer_amd.dist.shard_batch / GradientAllReduce) instead; "
                                  "nn.DataParallel over a single device is fine")

    def _workspace(self, need: int, device) -> Tensor:
        """One workspace per (device, caller stream): two host threads driving the same module on their own streams must
        not scribble over each other's activations."""
        if self._ws is None:
            from collections import OrderedDict
            self._ws = OrderedDict()
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
        self._ws.move_to_end(key)
        while len(self._ws) > self.MAX_WORKSPACES:       # least recently used first: a caller cycling through PyTorch's stream pool
            self._ws.popitem(last=False)                 # (32 per priority) must not pin a multi-GB workspace per stream; the block goes
                                                         # back to the caching allocator's pool of the stream it was allocated (and used) on
        return ws

    MAX_WORKSPACES = 8      # (round 6: infer.PipelinedForward drives the module from a ring of streams)

    # ---- forward -----------------------------------------------------------------------------
    def forward(self, x: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        if self.token_projection == 'conv' and torch.is_grad_enabled() and (self.training or x.requires_grad or any(p.requires_grad for p in self.parameters())):
            from .train import TOKEN_PROJECTION_TRAINING
            raise NotImplementedError(TOKEN_PROJECTION_TRAINING)
        if self.cfg.cross_modulator and torch.is_grad_enabled() and (self.training or x.requires_grad or any(p.requires_grad for p in self.parameters())):
            from .train import CROSS_MODULATOR_TRAINING
            raise NotImplementedError(CROSS_MODULATOR_TRAINING)
        if self.cfg.stage_windows()[4] == 4 and x.dim() == 4:     # built for 64x64 patches: 4 downsamplings x the bottleneck's window 4
            for name, n in (("H", x.shape[2]), ("W", x.shape[3])):
                if n % 64 or n <= 0:
                    raise UformerHipError(f"{name}={n} must be a positive multiple of 64 (a model built for img_size {self.reso}: "
                                          f"4 downsamplings x the bottleneck's 4x4 windows)")
            if mask is not None:
                raise NotImplementedError("the mask argument is not supported by a model whose bottleneck runs on 4x4 windows (img_size 64; "
                                          "no reference script passes it)")
        if not x.is_cuda:
            raise UformerHipError("uformer_amd.Uformer runs on an MI355X only; there is no CPU fallback "
                                  "(the CPU oracle lives in oracle/ and is test infrastructure)")
        if x.dim() != 4 or x.shape[1] != self.dd_in:
            raise UformerHipError(f"expected (B,{self.dd_in},H,W) input, got {tuple(x.shape)}")
        # autograd is wanted whenever grad mode is on and something upstream requires it -- in train() AND in eval() mode
        # (fine-tuning with frozen statistics, input gradients): the fused inference kernels keep no activations and would
        # return a tensor without grad_fn, i.e. silently drop the data term's gradients
        if torch.is_grad_enabled() and (self.training or x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if mask is None:
                return self._forward_train(x)
            # the autograd path does not take the mask argument (no reference script passes it).  Gradients explicitly asked for
            # (train() mode, or an input that requires grad): say so.  eval() with grad mode merely left on (``model.eval(); model(x,
            # mask)`` without torch.no_grad(), the reference's test scripts' habit): run the inference kernels, warn once.
            if self.training or x.requires_grad:
                raise NotImplementedError("the mask argument is not supported by the autograd path (no reference script passes it): "
                                          "wrap the call in torch.no_grad() for inference")
            if not getattr(self, "_warned_eval_mask", False):
                import warnings
                warnings.warn("uformer_amd.Uformer: eval() forward with a mask while grad mode is on runs the inference kernels; the result has no "
                              "grad_fn (wrap the call in torch.no_grad() to silence this)", stacklevel=2)
                self._warned_eval_mask = True
        if mask is not None:
            return self._forward_blockwise(x, mask)
        B, _, H, W = x.shape
        xin = x.detach().float().contiguous()
        dt = ops.uf_dtype(self.compute_dtype)
        with torch.cuda.device(x.device):
            lib = _lib.load()
            pk = self._get_packed(x.device)
            if pk.win4:      # built for 64x64 patches: the bottleneck runs on 4x4 windows (uf_uformer_win4_fwd)
                need = lib.uf_uformer_win4_workspace_bytes(pk.desc, B, H, W, dt)
                if need == 0:
                    raise UformerHipError("uf_uformer_win4_workspace_bytes: " + _lib.last_error())
                ws = self._workspace(need, x.device)
                out = torch.empty((B, self.in_chans, H, W), dtype=torch.float32, device=x.device)
                ops._launch("uf_uformer_win4_fwd", x.device, pk.desc, pk.bneck, xin, out, B, H, W, dt, ws, ws.numel())
                return out.to(x.dtype)
            need = lib.uf_uformer_workspace_bytes(pk.desc, B, H, W, dt)
            if need == 0:
                raise UformerHipError("uf_uformer_workspace_bytes: " + _lib.last_error())
            ws = self._workspace(need, x.device)
            out = torch.empty((B, self.in_chans, H, W), dtype=torch.float32, device=x.device)
            ops._launch("uf_uformer_fwd", x.device, pk.desc, xin, out, B, H, W, dt, ws, ws.numel())
        return out.to(x.dtype)

    def drop_path_rates(self):
        """Per-block stochastic-depth rates in execution order (model.py:1093-1095)."""
        from .spec import STAGES
        return [float(blk.drop_path_rate) for name in STAGES for blk in getattr(self, name).blocks]

    def _forward_train(self, x: Tensor) -> Tensor:
        """train() with grad enabled: the op-by-op tape of uformer_amd/train.py behind torch.autograd (the fused inference
        kernels keep no activations).  DropPath masks are drawn here, per block and branch, as timm's DropPath does
        (train/train_denoise.py:181-184 then calls backward on the loss)."""
        from . import train
        self._check_not_replica()
        sd = self.state_dict(keep_vars=True)
        names, params = list(sd.keys()), list(sd.values())
        sink = getattr(self, "grad_sink", None)
        # gradients go straight into the all-reduce buckets as the reverse sweep finishes each stage (sink); use_checkpoint=True
        # (model.py:1056-1057: torch.utils.checkpoint around every block) = the recompute form: a block keeps only its input
        names = train.NamesWithSink(names)
        names.sink = sink
        # (2-byte operand types only: compute_dtype=float32 always keeps its intermediates -- UformerTape's rule; the f32 fused forward + op-level
        #  recomputation pair is a combination no fixture covers)
        names.recompute = True if (self.use_checkpoint and self.compute_dtype in (torch.bfloat16, torch.float16)) else None
        rates = self.drop_path_rates() if self.training else []      # eval(): DropPath is the identity (timm)
        drop = getattr(self, "_drop_scales_override", None) if self.training else None
        if drop is None and any(r > 0 for r in rates):
            drop = train.sample_drop_scales(rates, x.shape[0], x.device)
        return train.UformerFunction.apply(x, self.cfg, self.compute_dtype, drop, names, *params)

    def _forward_blockwise(self, x: Tensor, mask: Optional[Tensor]) -> Tensor:
        """Module-by-module path (used when the rarely-used ``mask`` argument is given):
        the same wiring as model.py:1269-1305, every step through the C ABI."""
        cd = self.compute_dtype
        H, W = x.shape[-2:]
        r = [(H // d, W // d) for d in (1, 2, 4, 8, 16)]     # (height, width) of each resolution level
        y = self.input_proj(x.detach().float())
        conv0 = self.encoderlayer_0(y, mask, cd, hw=r[0])
        conv1 = self.encoderlayer_1(self.dowsample_0(conv0, cd, hw=r[0]), mask, cd, hw=r[1])
        conv2 = self.encoderlayer_2(self.dowsample_1(conv1, cd, hw=r[1]), mask, cd, hw=r[2])
        conv3 = self.encoderlayer_3(self.dowsample_2(conv2, cd, hw=r[2]), mask, cd, hw=r[3])
        conv4 = self.conv(self.dowsample_3(conv3, cd, hw=r[3]), mask, cd, hw=r[4])
        d0 = self.decoderlayer_0(torch.cat([self.upsample_0(conv4, cd, hw=r[4]), conv3], -1), mask, cd, hw=r[3])
        d1 = self.decoderlayer_1(torch.cat([self.upsample_1(d0, cd, hw=r[3]), conv2], -1), mask, cd, hw=r[2])
        d2 = self.decoderlayer_2(torch.cat([self.upsample_2(d1, cd, hw=r[2]), conv1], -1), mask, cd, hw=r[1])
        d3 = self.decoderlayer_3(torch.cat([self.upsample_3(d2, cd, hw=r[1]), conv0], -1), mask, cd, hw=r[0])
        out = self.output_proj(d3, x.detach().float() if self.dd_in == 3 else None, hw=r[0])
        return out.to(x.dtype)

    def flops(self):
        """Exact multiply-accumulates of one forward at the constructor resolution."""
        total = 0
        r = self.reso
        total += self.input_proj.flops(r, r) + self.output_proj.flops(r, r)
        dims = self.cfg.stage_dims()
        div = self.cfg.stage_res_div()
        wins = self.cfg.stage_windows()
        for s in range(9):
            L = (r // div[s]) ** 2
            # LeFF: the depthwise conv's 9 taps over 4C channels (36); Mlp has none (model.py:644-651)
            # ConvProjection: three depthwise 3x3 convolutions in front of the q | k | v GEMM (27 taps per channel, model.py:373-377)
            total += self.cfg.depths[s] * L * dims[s] * (12 * dims[s] + 2 * wins[s] ** 2 + (0 if self.cfg.mlp_is_ffn() else 36)
                                                         + (27 if self.cfg.token_projection == 'conv' else 0))
            if self.cfg.stage_has_cross_modulator(s):
                # cross attention (model.py:600-618): to_q and proj over the L tokens, to_kv over the 64 learned tokens, q k^T and attn v against 64 keys
                total += self.cfg.depths[s] * (2 * L * dims[s] * dims[s] + 2 * 64 * dims[s] * dims[s] + 2 * L * dims[s] * 64)
        for s in range(4):
            L = (r // div[s]) ** 2
            total += (L // 4) * dims[s] * 2 * dims[s] * 16
        for k, (cin, cout) in enumerate(self.cfg.upsample_io()):
            L = (r // div[4 + k]) ** 2
            total += 4 * L * cin * cout
        return total


class ConvBlock(nn.Module):
    """model.py:83-106.  Holds the parameters (``block.0``, ``block.2``, ``conv11``); UNet.forward runs them through the C ABI."""

    def __init__(self, in_channel, out_channel, strides=1):
        super().__init__()
        if strides != 1:
            raise NotImplementedError(f"ConvBlock(strides={strides}): the HIP UNet runs stride-1 blocks only (the reference's UNet uses no other)")
        self.strides = strides
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.block = nn.Sequential(
            nn.Conv2d(in_channel, out_channel, kernel_size=3, stride=strides, padding=1),
            nn.LeakyReLU(inplace=True),
            nn.Conv2d(out_channel, out_channel, kernel_size=3, stride=strides, padding=1),
            nn.LeakyReLU(inplace=True),
        )
        self.conv11 = nn.Conv2d(in_channel, out_channel, kernel_size=1, stride=strides, padding=0)

    def flops(self, H, W):
        return H * W * self.in_channel * self.out_channel * (3 * 3 + 1) + H * W * self.out_channel * self.out_channel * 3 * 3


class UNet(nn.Module):
    """Drop-in for the reference's conv baseline ``UNet`` (model.py:128-174): the same constructor, submodule names and
    ``state_dict`` layout; ``forward`` is one ``uf_unet_fwd`` call (implicit-GEMM convolutions on MFMA, include/uformer_hip.h).
    Inputs (B, 3, H, W) with H and W positive multiples of 16 (four stride-2 convolutions); H != W is allowed."""

    def __init__(self, block=ConvBlock, dim=32, compute_dtype=torch.bfloat16):
        super().__init__()
        if compute_dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"compute_dtype must be float32, bfloat16 or float16, got {compute_dtype}")
        if dim not in (16, 32, 64, 128):
            raise ValueError(f"UNet(dim={dim}): dim must be 16, 32, 64 or 128 (conv10 runs on the OutputProj kernel, which takes those widths)")
        self.dim = dim
        self.compute_dtype = compute_dtype
        self.ConvBlock1 = ConvBlock(3, dim, strides=1)
        self.pool1 = nn.Conv2d(dim, dim, kernel_size=4, stride=2, padding=1)
        self.ConvBlock2 = block(dim, dim * 2, strides=1)
        self.pool2 = nn.Conv2d(dim * 2, dim * 2, kernel_size=4, stride=2, padding=1)
        self.ConvBlock3 = block(dim * 2, dim * 4, strides=1)
        self.pool3 = nn.Conv2d(dim * 4, dim * 4, kernel_size=4, stride=2, padding=1)
        self.ConvBlock4 = block(dim * 4, dim * 8, strides=1)
        self.pool4 = nn.Conv2d(dim * 8, dim * 8, kernel_size=4, stride=2, padding=1)
        self.ConvBlock5 = block(dim * 8, dim * 16, strides=1)
        self.upv6 = nn.ConvTranspose2d(dim * 16, dim * 8, 2, stride=2)
        self.ConvBlock6 = block(dim * 16, dim * 8, strides=1)
        self.upv7 = nn.ConvTranspose2d(dim * 8, dim * 4, 2, stride=2)
        self.ConvBlock7 = block(dim * 8, dim * 4, strides=1)
        self.upv8 = nn.ConvTranspose2d(dim * 4, dim * 2, 2, stride=2)
        self.ConvBlock8 = block(dim * 4, dim * 2, strides=1)
        self.upv9 = nn.ConvTranspose2d(dim * 2, dim, 2, stride=2)
        self.ConvBlock9 = block(dim * 2, dim, strides=1)
        self.conv10 = nn.Conv2d(dim, 3, kernel_size=3, stride=1, padding=1)
        self._packed = None
        self._ws = None

    MAX_WORKSPACES = Uformer.MAX_WORKSPACES
    _workspace = Uformer._workspace

    def _apply(self, fn, *a, **k):
        self._packed = None
        self._ws = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts reference checkpoints, including ``{'state_dict': ...}`` payloads and the ``module.`` prefix
        (utils/model_utils.py:23-33)."""
        if "state_dict" in state_dict and not any(k.startswith("ConvBlock1") for k in state_dict):
            state_dict = state_dict["state_dict"]
        if all(k.startswith("module.") for k in state_dict):
            state_dict = {k[7:]: v for k, v in state_dict.items()}
        self._packed = None
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def repack(self):
        self._packed = None

    def _get_packed(self, device):
        plist = list(self.parameters())
        key = (self.compute_dtype, str(device), tuple(map(torch.Tensor.data_ptr, plist)), tuple(p._version for p in plist))
        if self._packed is None or self._packed_key != key:
            self._packed = packing.PackedUNet(self.state_dict(keep_vars=True), self.dim, self.compute_dtype)
            self._packed_key = key
        return self._packed

    def forward(self, x: Tensor) -> Tensor:
        if x.dim() != 4 or x.shape[1] != 3:
            raise UformerHipError(f"expected (B,3,H,W) input, got {tuple(x.shape)}")
        B, _, H, W = x.shape
        if H <= 0 or W <= 0 or H % 16 or W % 16:
            raise UformerHipError(f"UNet: H={H} and W={W} must be positive multiples of 16 (four stride-2 convolutions)")
        if not x.is_cuda:
            raise UformerHipError("uformer_amd.UNet runs on an MI355X only; there is no CPU fallback")
        if torch.is_grad_enabled() and (self.training or x.requires_grad):
            raise NotImplementedError("uformer_amd.UNet has no autograd path yet: run it in eval() under torch.no_grad(), and train "
                                      "the reference's UNet (INTEGRATION.md section A)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()) and not getattr(self, "_warned_grad", False):
            import warnings
            warnings.warn("uformer_amd.UNet: eval() forward with grad mode on runs the inference kernels; the result has no grad_fn "
                          "(wrap the call in torch.no_grad() to silence this)", stacklevel=2)
            self._warned_grad = True
        xin = x.detach().float().contiguous()
        dt = ops.uf_dtype(self.compute_dtype)
        with torch.cuda.device(x.device):
            lib = _lib.load()
            pk = self._get_packed(x.device)
            need = lib.uf_unet_workspace_bytes(pk.desc, B, H, W, dt)
            if need == 0:
                raise UformerHipError("uf_unet_workspace_bytes: " + _lib.last_error())
            ws = self._workspace(need, x.device)
            out = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
            ops._launch("uf_unet_fwd", x.device, pk.desc, xin, out, B, H, W, dt, ws, ws.numel())
        return out.to(x.dtype)

    def flops(self, H, W):
        """model.py:176-200, the reference's count (multiply-accumulates)."""
        d = self.dim
        flops = 0
        flops += self.ConvBlock1.flops(H, W)
        flops += H / 2 * W / 2 * d * d * 4 * 4
        flops += self.ConvBlock2.flops(H / 2, W / 2)
        flops += H / 4 * W / 4 * d * 2 * d * 2 * 4 * 4
        flops += self.ConvBlock3.flops(H / 4, W / 4)
        flops += H / 8 * W / 8 * d * 4 * d * 4 * 4 * 4
        flops += self.ConvBlock4.flops(H / 8, W / 8)
        flops += H / 16 * W / 16 * d * 8 * d * 8 * 4 * 4
        flops += self.ConvBlock5.flops(H / 16, W / 16)
        flops += H / 8 * W / 8 * d * 16 * d * 8 * 2 * 2
        flops += self.ConvBlock6.flops(H / 8, W / 8)
        flops += H / 4 * W / 4 * d * 8 * d * 4 * 2 * 2
        flops += self.ConvBlock7.flops(H / 4, W / 4)
        flops += H / 2 * W / 2 * d * 4 * d * 2 * 2 * 2
        flops += self.ConvBlock8.flops(H / 2, W / 2)
        flops += H * W * d * 2 * d * 2 * 2
        flops += self.ConvBlock9.flops(H, W)
        flops += H * W * d * 3 * 3 * 3
        return flops


def get_arch(arch: str, train_ps: int = 128, dd_in: int = 3, embed_dim: int = 32, compute_dtype=torch.bfloat16,
             token_projection: str = 'linear', cross_modulator: bool = False, in_chans: int = 3) -> nn.Module:
    """utils/model_utils.py:56-81 ``get_arch(opt)`` with the option fields as arguments (``token_projection``: its hard-coded 'linear', or
    'conv' for the paper's ablation row; ``cross_modulator``: its hard-coded False, or True for the cross-modulator variant, inference only).
    ``dd_in`` is forwarded exactly where the reference forwards it (Uformer_B alone); ``in_chans`` (not an option of the reference's: its
    constructor default 3) goes to every Uformer arch."""
    common = dict(win_size=8, token_projection=token_projection, token_mlp='leff', modulator=True, compute_dtype=compute_dtype,
                  cross_modulator=cross_modulator, in_chans=in_chans)
    if arch == 'Uformer':
        return Uformer(img_size=train_ps, embed_dim=embed_dim, **common)
    if arch == 'Uformer_T':
        return Uformer(img_size=train_ps, embed_dim=16, **common)
    if arch == 'Uformer_S':
        return Uformer(img_size=train_ps, embed_dim=32, **common)
    if arch == 'Uformer_S_noshift':
        return Uformer(img_size=train_ps, embed_dim=32, shift_flag=False, **common)
    if arch == 'Uformer_B':
        return Uformer(img_size=train_ps, embed_dim=32, depths=[1, 2, 8, 8, 2, 8, 8, 2, 1], dd_in=dd_in, **common)
    if arch == 'UNet':
        return UNet(dim=embed_dim, compute_dtype=compute_dtype)
    raise Exception("Arch error!")
