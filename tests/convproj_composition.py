"""fp32 CPU restatement of the Uformer forward with ``token_projection='conv'`` (the reference's ConvProjection, model.py:381-410, in place of
LinearProjection): the rectangle-general composition of tests/rect_composition.py with q, k and v of every 8x8 window made by three SepConv2d
(depthwise 3x3 with zero padding at the WINDOW border -> ReLU -> pointwise 1x1, model.py:344-371).  The feed-forward half is LeFF or, where
the parameters are ``mlp.fc1`` / ``mlp.fc2``, the Mlp of tests/ffn_composition.py: the two halves are independent.

tests/test_convproj.py pins it to the reference's own outputs (tests/golden/convproj_*.npz, written by tests/golden/make_golden_convproj.py);
the GPU tests use it where the reference cannot go (rectangular inputs, the mask argument, 'conv' with 'ffn').  Plain torch.  TEST INFRASTRUCTURE ONLY."""
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

import ffn_composition as FC
import rect_composition as RC
from oracle import uformer_oracle as O

Tensor = torch.Tensor
WIN = O.WIN


def sep_conv(img: Tensor, p: Dict[str, Tensor], prefix: str) -> Tensor:
    """SepConv2d.forward (model.py:367-371) on (B_, C, 8, 8) window images; ``prefix`` ends in 'to_q.' / 'to_k.' / 'to_v.'."""
    h = F.conv2d(img, p[prefix + "depthwise.weight"], p[prefix + "depthwise.bias"], stride=1, padding=1, groups=img.shape[1])
    return F.conv2d(F.relu(h), p[prefix + "pointwise.weight"], p[prefix + "pointwise.bias"])


def conv_projection(x: Tensor, p: Dict[str, Tensor], prefix: str, heads: int):
    """ConvProjection.forward (model.py:394-410) for self-attention: x (B_, 64, C) -> q, k, v (B_, heads, 64, hd); ``prefix`` ends in 'qkv.'."""
    B_, N, C = x.shape
    img = x.transpose(1, 2).reshape(B_, C, WIN, WIN)                               # 'b (l w) c -> b c l w'
    return tuple(sep_conv(img, p, prefix + f"to_{j}.").reshape(B_, heads, C // heads, N).transpose(2, 3) for j in "qkv")   # 'b (h d) l w -> b h (l w) d'


def window_attention(x: Tensor, p: Dict[str, Tensor], prefix: str, heads: int, mask: Optional[Tensor] = None) -> Tensor:
    """WindowAttention.forward (model.py:494-522) with the ConvProjection; ``prefix`` ends in 'attn.'."""
    B_, N, C = x.shape
    q, k, v = conv_projection(x, p, prefix + "qkv.", heads)
    attn = (q * (C // heads) ** -0.5) @ k.transpose(-2, -1)
    attn = attn + O.relative_position_bias(p[prefix + "relative_position_bias_table"], p[prefix + "relative_position_index"]).unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.reshape(B_ // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).reshape(-1, heads, N, N)
    out = (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(B_, N, C)
    return out @ p[prefix + "proj.weight"].t() + p[prefix + "proj.bias"]


def lewin_block(x: Tensor, p: Dict[str, Tensor], prefix: str, heads: int, shift: int, H: int, W: int, mask: Optional[Tensor] = None) -> Tensor:
    """LeWinTransformerBlock.forward (model.py:908-989, eval mode) with a ConvProjection, on an H x W map."""
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
    aw = window_attention(yw, p, prefix + "attn.", heads, attn_mask)
    y = O.window_reverse(aw.reshape(-1, WIN, WIN, C), WIN, H, W)
    if shift > 0:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    x = shortcut + y.reshape(B, L, C)
    z = O.layer_norm(x, p[prefix + "norm2.weight"], p[prefix + "norm2.bias"])
    if (prefix + "mlp.fc1.weight") in p:
        return x + FC.mlp(z, p, prefix + "mlp.")
    return x + RC.leff(z, p, prefix + "mlp.", H, W)


def uformer_forward(x: Tensor, p: Dict[str, Tensor], *, img_size: int, embed_dim: int, depths: Sequence[int], num_heads: Sequence[int],
                    dd_in: int = 3, mask: Optional[Tensor] = None) -> Tensor:
    """Uformer.forward (model.py:1269-1305, eval mode) with token_projection='conv' for a (B, dd_in, H, W) input, H and W multiples of 128."""
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
        y = RC.downsample(y, p, f"dowsample_{s}.", *hw[s])
    y = stage(y, 4)
    for k in range(4):
        y = stage(torch.cat([RC.upsample(y, p, f"upsample_{k}.", *hw[4 + k]), skips[3 - k]], -1), 5 + k)
    y = F.conv2d(RC._tokens_to_nchw(y, H, W), p["output_proj.proj.0.weight"], p["output_proj.proj.0.bias"], stride=1, padding=1)
    return x + y if dd_in == 3 else y
