"""fp32 CPU restatement of the Uformer forward with ``token_mlp='ffn'`` (the reference's Mlp, model.py:623-642, in place of LeFF): the
rectangle-general composition of tests/rect_composition.py with the block's feed-forward half replaced by fc1 -> GELU -> fc2.

tests/test_ffn.py pins it to the reference's own outputs (tests/golden/ffn_*.npz, written by tests/golden/make_golden_ffn.py); the GPU
tests use it where the reference cannot go (rectangular inputs, the mask argument).  Differentiable plain torch.  TEST INFRASTRUCTURE ONLY."""
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

import rect_composition as RC
from oracle import uformer_oracle as O

Tensor = torch.Tensor
WIN = O.WIN


def mlp(x: Tensor, p: Dict[str, Tensor], prefix: str) -> Tensor:
    """Mlp.forward with drop = 0 (model.py:636-642); ``prefix`` ends in 'mlp.'."""
    return O.gelu_erf(x @ p[prefix + "fc1.weight"].t() + p[prefix + "fc1.bias"]) @ p[prefix + "fc2.weight"].t() + p[prefix + "fc2.bias"]


def lewin_block(x: Tensor, p: Dict[str, Tensor], prefix: str, heads: int, shift: int, H: int, W: int, mask: Optional[Tensor] = None,
                drop: Optional[Tensor] = None) -> Tensor:
    """LeWinTransformerBlock.forward (model.py:908-989) with an Mlp, on an H x W map.  ``drop``: None or (2, B) DropPath scales."""
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
    y = y.reshape(B, L, C)
    s1 = 1.0 if drop is None else drop[0].reshape(B, 1, 1)
    s2 = 1.0 if drop is None else drop[1].reshape(B, 1, 1)
    x = shortcut + s1 * y
    return x + s2 * mlp(O.layer_norm(x, p[prefix + "norm2.weight"], p[prefix + "norm2.bias"]), p, prefix + "mlp.")


def uformer_forward(x: Tensor, p: Dict[str, Tensor], *, img_size: int, embed_dim: int, depths: Sequence[int], num_heads: Sequence[int],
                    dd_in: int = 3, mask: Optional[Tensor] = None, drop_scales: Optional[Tensor] = None) -> Tensor:
    """Uformer.forward (model.py:1269-1305) with token_mlp='ffn' for a (B, dd_in, H, W) input, H and W multiples of 128.
    ``drop_scales``: None (eval) or (2 * n_blocks, B) DropPath scales in execution order."""
    H, W = x.shape[-2:]
    shifts = O.block_shifts(img_size, depths, WIN)
    hw = [(H // d, W // d) for d in (1, 2, 4, 8, 16, 8, 4, 2, 1)]
    first = [sum(depths[:s]) for s in range(9)]

    def stage(y: Tensor, s: int) -> Tensor:
        for i in range(depths[s]):
            bi = first[s] + i
            dr = drop_scales[2 * bi:2 * bi + 2] if drop_scales is not None else None
            y = lewin_block(y, p, f"{O.STAGES[s]}.blocks.{i}.", num_heads[s], shifts[s][i], *hw[s], mask=mask, drop=dr)
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
