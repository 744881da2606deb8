"""A rectangle-general CPU composition of the Uformer forward, built from the oracle's own primitives (window attention, LayerNorm,
shift mask, user-mask expansion, GELU) plus torch convolutions for LeFF's depthwise conv, the samplers, the stem and the head.

The oracle (oracle/uformer_oracle.py) restates the reference square-only (it takes H = W = sqrt(L), as model.py:910-911 does); this
module carries (H, W) explicitly instead.  tests/test_rect.py pins it to ``O.uformer_forward`` at H == W and checks it for transpose
equivariance; the GPU tests compare the library's rectangular forward / backward against it.  Differentiable (plain torch ops), so
torch autograd through it is the reference for the rectangular training path.  TEST INFRASTRUCTURE ONLY."""
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import uformer_oracle as O

Tensor = torch.Tensor
WIN = O.WIN


def leff(x: Tensor, p: Dict[str, Tensor], prefix: str, H: int, W: int) -> Tensor:
    B, L, C = x.shape
    h = O.gelu_erf(x @ p[prefix + "linear1.0.weight"].t() + p[prefix + "linear1.0.bias"])
    hid = h.shape[-1]
    h = h.reshape(B, H, W, hid).permute(0, 3, 1, 2)
    h = O.gelu_erf(F.conv2d(h, p[prefix + "dwconv.0.weight"], p[prefix + "dwconv.0.bias"], stride=1, padding=1, groups=hid))
    h = h.permute(0, 2, 3, 1).reshape(B, L, hid)
    return h @ p[prefix + "linear2.0.weight"].t() + p[prefix + "linear2.0.bias"]


def lewin_block(x: Tensor, p: Dict[str, Tensor], prefix: str, heads: int, shift: int, H: int, W: int,
                mask: Optional[Tensor] = None) -> Tensor:
    """O.lewin_block (eval mode) on an H x W map."""
    B, L, C = x.shape
    attn_mask = O.input_attn_mask(mask, H, W, WIN) if mask is not None else None
    if shift > 0:
        sm = O.shift_attn_mask(H, W, WIN, shift)
        attn_mask = attn_mask + sm if attn_mask is not None else sm
    shortcut = x
    y = O.layer_norm(x, p[prefix + "norm1.weight"], p[prefix + "norm1.bias"]).reshape(B, H, W, C)
    if shift > 0:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    yw = O.window_partition(y, WIN).reshape(-1, WIN * WIN, C)
    if (prefix + "modulator.weight") in p:
        yw = yw + p[prefix + "modulator.weight"]
    aw = O.window_attention(yw, p, prefix + "attn.", heads, attn_mask)
    y = O.window_reverse(aw.reshape(-1, WIN, WIN, C), WIN, H, W)
    if shift > 0:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    x = shortcut + y.reshape(B, L, C)
    z = O.layer_norm(x, p[prefix + "norm2.weight"], p[prefix + "norm2.bias"])
    return x + leff(z, p, prefix + "mlp.", H, W)


def _tokens_to_nchw(x: Tensor, H: int, W: int) -> Tensor:
    B, L, C = x.shape
    return x.transpose(1, 2).reshape(B, C, H, W)


def _nchw_to_tokens(y: Tensor) -> Tensor:
    return y.flatten(2).transpose(1, 2).contiguous()


def downsample(x: Tensor, p: Dict[str, Tensor], prefix: str, H: int, W: int) -> Tensor:
    return _nchw_to_tokens(F.conv2d(_tokens_to_nchw(x, H, W), p[prefix + "conv.0.weight"], p[prefix + "conv.0.bias"], stride=2, padding=1))


def upsample(x: Tensor, p: Dict[str, Tensor], prefix: str, H: int, W: int) -> Tensor:
    return _nchw_to_tokens(F.conv_transpose2d(_tokens_to_nchw(x, H, W), p[prefix + "deconv.0.weight"], p[prefix + "deconv.0.bias"], stride=2))


def uformer_forward(x: Tensor, p: Dict[str, Tensor], *, img_size: int, embed_dim: int, depths: Sequence[int], num_heads: Sequence[int],
                    dd_in: int = 3, mask: Optional[Tensor] = None) -> Tensor:
    """O.uformer_forward (eval mode) for a (B, dd_in, H, W) input with H, W multiples of 128, H != W allowed.  Shifts are decided by
    the CONSTRUCTOR size, as in the reference (model.py:863-866, 1030)."""
    H, W = x.shape[-2:]
    shifts = O.block_shifts(img_size, depths, WIN)
    hw = [(H // d, W // d) for d in (1, 2, 4, 8, 16, 8, 4, 2, 1)]

    def stage(y: Tensor, s: int) -> Tensor:
        for i in range(depths[s]):
            y = lewin_block(y, p, f"{O.STAGES[s]}.blocks.{i}.", num_heads[s], shifts[s][i], *hw[s], mask=mask)
        return y

    y = O.input_proj(x, p)
    skips = []
    for s in range(4):
        y = stage(y, s)
        skips.append(y)
        y = downsample(y, p, f"dowsample_{s}.", *hw[s])
    y = stage(y, 4)
    for k in range(4):
        y = stage(torch.cat([upsample(y, p, f"upsample_{k}.", *hw[4 + k]), skips[3 - k]], -1), 5 + k)
    y = F.conv2d(_tokens_to_nchw(y, H, W), p["output_proj.proj.0.weight"], p["output_proj.proj.0.bias"], stride=1, padding=1)
    return x + y if dd_in == 3 else y


def transpose_state_dict(sd: Dict[str, Tensor], win: int = WIN) -> Dict[str, Tensor]:
    """The weights of the transposed network: every spatial kernel transposed (conv, deconv, depthwise), the (2w-1) x (2w-1) layout of
    each relative-position table and the w x w layout of each modulator.  uformer(x^T; sd^T) = uformer(x; sd)^T in exact arithmetic."""
    out = {}
    n = 2 * win - 1
    for k, v in sd.items():
        if k.endswith("relative_position_bias_table"):
            v = v.reshape(n, n, -1).transpose(0, 1).reshape(n * n, -1)
        elif k.endswith("modulator.weight"):
            v = v.reshape(win, win, -1).transpose(0, 1).reshape(win * win, -1)
        elif v.dim() == 4:
            v = v.transpose(-1, -2)
        out[k] = v.contiguous()
    return out
