"""fp32 CPU restatement of the Uformer forward with ``cross_modulator=True`` (model.py:873-877, :945-949): in front of every decoder block the
UN-normalised stream attends to the 64 learned rows of ``cross_modulator.weight`` through ``cross_attn`` (the reference's Attention, model.py:549-595:
a LinearProjection whatever ``token_projection`` says, no relative-position bias, no mask) and the result is added to the stream.  ``norm_cross`` is
in the state_dict and never read: the reference overwrites its output on the next line.  The rest of a block is the rectangle-general composition
of tests/rect_composition.py, or tests/ffn_composition.py / tests/convproj_composition.py where the block's parameters are an Mlp's / a ConvProjection's.

tests/test_crossmod.py pins it to the reference's own outputs (tests/golden/crossmod_*.npz, written by tests/golden/make_golden_crossmod.py); the GPU
tests use it where the reference cannot go (rectangular inputs, the mask argument).  Plain torch.  TEST INFRASTRUCTURE ONLY."""
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

import convproj_composition as CC
import ffn_composition as FC
import rect_composition as RC
from oracle import uformer_oracle as O

Tensor = torch.Tensor
WIN = O.WIN


def cross_attention(x: Tensor, p: Dict[str, Tensor], prefix: str, heads: int) -> Tensor:
    """``cross_attn(x, cross_modulator.weight)`` (Attention.forward model.py:567-595 over LinearProjection.forward with attn_kv, :431-442) for
    x (..., C): every row on its own against the 64 shared keys / values.  ``prefix`` is the block's."""
    C = x.shape[-1]
    hd = C // heads
    rows = x.reshape(-1, C)
    q = rows @ p[prefix + "cross_attn.qkv.to_q.weight"].t() + p[prefix + "cross_attn.qkv.to_q.bias"]
    kv = p[prefix + "cross_modulator.weight"] @ p[prefix + "cross_attn.qkv.to_kv.weight"].t() + p[prefix + "cross_attn.qkv.to_kv.bias"]
    q = q.reshape(-1, heads, hd).transpose(0, 1) * hd ** -0.5                     # (heads, M, hd)
    k = kv[:, :C].reshape(-1, heads, hd).transpose(0, 1)                          # (heads, 64, hd)
    v = kv[:, C:].reshape(-1, heads, hd).transpose(0, 1)
    o = (torch.softmax(q @ k.transpose(-2, -1), dim=-1) @ v).transpose(0, 1).reshape(-1, C)
    return (o @ p[prefix + "cross_attn.proj.weight"].t() + p[prefix + "cross_attn.proj.bias"]).reshape(x.shape)


def lewin_block(x: Tensor, p: Dict[str, Tensor], prefix: str, heads: int, shift: int, H: int, W: int, mask: Optional[Tensor] = None) -> Tensor:
    """LeWinTransformerBlock.forward (model.py:908-989, eval mode) on an H x W map, with or without a cross-modulator."""
    if (prefix + "cross_modulator.weight") in p:
        x = x + cross_attention(x, p, prefix, heads)                               # model.py:945-949: no norm_cross, no DropPath
    if (prefix + "attn.qkv.to_q.depthwise.weight") in p:
        return CC.lewin_block(x, p, prefix, heads, shift, H, W, mask)
    if (prefix + "mlp.fc1.weight") in p:
        return FC.lewin_block(x, p, prefix, heads, shift, H, W, mask)
    return RC.lewin_block(x, p, prefix, heads, shift, H, W, mask)


def uformer_forward(x: Tensor, p: Dict[str, Tensor], *, img_size: int, embed_dim: int, depths: Sequence[int], num_heads: Sequence[int],
                    dd_in: int = 3, mask: Optional[Tensor] = None) -> Tensor:
    """Uformer.forward (model.py:1269-1305, eval mode) for a (B, dd_in, H, W) input, H and W multiples of 128; the cross-modulator runs in
    whichever blocks carry its parameters (the decoder stages of a model built with cross_modulator=True)."""
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
