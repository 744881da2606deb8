"""Weight re-layout from the reference ``state_dict`` to what the kernels read.

Pure tensor reshapes (no arithmetic except the dtype cast of GEMM weights to the operand
type); runs on whatever device the parameters live on.  Layouts are documented in
``include/uformer_hip.h``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

import torch

from . import _lib

Tensor = torch.Tensor


def rpb_dense(table: Tensor, index: Tensor) -> Tensor:
    """(225,heads) table + (64,64) int64 index -> (heads,64,64) f32.  model.py:500-502."""
    n = index.shape[0]
    return table.detach()[index.reshape(-1)].reshape(n, n, -1).permute(2, 0, 1).contiguous().float()


def pack_frag(w: Tensor, dtype: torch.dtype) -> Tensor:
    """nn.Linear weight (N,K) -> fragment-major (N/16, ceil(K/32), 4, 16, 8) of ``dtype``: one wave-level
    MFMA-operand load then reads 1 KiB contiguous (layout formula in include/uformer_hip.h)."""
    N, K = w.shape
    KP = (K + 31) // 32 * 32
    w = w.detach().to(dtype)
    if KP != K:
        w = torch.nn.functional.pad(w, (0, KP - K))
    return w.reshape(N // 16, 16, KP // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def pack_rpb_table(dense: Tensor):
    """(heads,64,64) bias -> compact (heads,15,15) table T[h][dy+7][7-dx] with dy = yq-yk, dx = xq-xk, if the bias is
    Toeplitz in (dy,dx) (true for the reference's relative_position_index, model.py:467-477); else None."""
    h = dense.shape[0]
    c = torch.arange(8, device=dense.device)
    ys, xs = torch.meshgrid(c, c, indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    row = (ys[:, None] - ys[None, :] + 7)          # (64,64) dy+7
    pos = (7 - (xs[:, None] - xs[None, :]))        # (64,64) 7-dx
    tab = torch.zeros(h, 15, 15, dtype=torch.float32, device=dense.device)
    tab[:, row, pos] = dense.float()
    if not torch.equal(tab[:, row, pos], dense.float()):
        return None
    return tab.contiguous()


def pack_rpb_table4(table: Tensor, index: Tensor) -> Tensor:
    """4x4-window bias: (49, heads) table + (16, 16) index -> (heads, 49) f32 T4[h][(dy+3)*7 + dx+3], dy = yq-yk, dx = xq-xk,
    the layout the 4x4-window kernels read (bias(q, k) = T4[h][Toeplitz entry of (q, k)], model.py:467-477 at win 4).  Raises
    unless the bias IS Toeplitz in (dy, dx) -- always true for the reference's relative_position_index."""
    dense = rpb_dense(table, index)                                  # (heads, 16, 16)
    if dense.shape[1:] != (16, 16):
        raise ValueError(f"pack_rpb_table4: expected a (16, 16) relative_position_index, got {tuple(index.shape)}")
    c = torch.arange(4, device=dense.device)
    ys, xs = torch.meshgrid(c, c, indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    ent = (ys[:, None] - ys[None, :] + 3) * 7 + (xs[:, None] - xs[None, :] + 3)     # (16, 16) entry of each (q, k) pair
    tab = torch.zeros(dense.shape[0], 49, dtype=torch.float32, device=dense.device)
    tab[:, ent] = dense
    if not torch.equal(tab[:, ent], dense):
        raise ValueError("pack_rpb_table4: the relative-position bias is not Toeplitz in (dy, dx); the 4x4-window kernels need the "
                         "reference's relative_position_index")
    return tab.contiguous()


def pack_dwconv(w: Tensor) -> Tensor:
    """(C,1,3,3) -> (9,C) tap-major f32."""
    return w.detach().reshape(w.shape[0], 9).t().contiguous().float()


def conv_projection_keys(sd: Dict[str, Tensor], prefix: str) -> bool:
    """True where the block under ``prefix`` carries a ConvProjection (``token_projection='conv'``, model.py:381-392)."""
    return (prefix + "attn.qkv.to_q.depthwise.weight") in sd


def pack_conv_projection(sd: Dict[str, Tensor], prefix: str):
    """The operands of ``uf_ln_convqkv_fwd`` from ``attn.qkv.to_{q,k,v}.{depthwise,pointwise}``: the three pointwise weights (C,C,1,1) as one
    row-major (3C, C) matrix q | k | v (not yet cast or fragment-packed), their biases f32 (3C,), the depthwise taps f32 (3, 9, C) tap-major
    as ``pack_dwconv`` lays them out (tap = ky * 3 + kx), and the depthwise biases f32 (3, C)."""
    g = lambda j, k: sd[prefix + f"attn.qkv.to_{j}.{k}"].detach()  # noqa: E731
    wpw = torch.cat([g(j, "pointwise.weight").reshape(g(j, "pointwise.weight").shape[0], -1) for j in "qkv"], 0)
    bpw = torch.cat([g(j, "pointwise.bias") for j in "qkv"], 0).contiguous().float()
    dw9 = torch.stack([pack_dwconv(g(j, "depthwise.weight")) for j in "qkv"], 0).contiguous()
    bdw = torch.stack([g(j, "depthwise.bias").float() for j in "qkv"], 0).contiguous()
    return wpw, bpw, dw9, bdw


def pack_downsample(w: Tensor, dtype: torch.dtype) -> Tensor:
    """Conv2d weight (2C,C,4,4) -> (2C, 16C) with k = (ky*4+kx)*C + c."""
    return w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous().to(dtype)


def pack_upsample(w: Tensor, dtype: torch.dtype) -> Tensor:
    """ConvTranspose2d weight (Cin,Cout,2,2) -> (4*Cout, Cin) with n = (dy*2+dx)*Cout + co."""
    return w.detach().permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous().to(dtype)


def pack_input_proj(w: Tensor) -> Tensor:
    """Conv2d weight (E,Cin,3,3) -> (Cin*9, E) f32."""
    return w.detach().permute(1, 2, 3, 0).reshape(-1, w.shape[0]).contiguous().float()


def pack_output_proj(w: Tensor) -> Tensor:
    """Conv2d weight (CO,C2,3,3) -> (CO, 9, C2) f32, CO = in_chans (1..4)."""
    return w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).contiguous().float()


def pack_block(sd: Dict[str, Tensor], prefix: str, heads: int, shift: int, dtype: torch.dtype):
    """Returns (BlockParams, keepalive list).  ``sd`` maps reference keys to tensors on the GPU."""
    # small f32 tensors are COPIED, never aliased: the packed block must stay valid when a parameter's storage is replaced
    # (p.data = ..., EMA swaps) until the owner notices the new (data_ptr, _version) key and repacks
    f = lambda k: sd[prefix + k].detach().float().clone().contiguous()  # noqa: E731
    t = lambda k: sd[prefix + k].detach().to(dtype, copy=True).contiguous()  # noqa: E731
    conv = conv_projection_keys(sd, prefix)
    if conv:      # ConvProjection (token_projection 'conv'): the three pointwise convolutions in the q | k | v slots, the depthwise taps beside them
        wqkv, bqkv, dw9, bdw = pack_conv_projection(sd, prefix)
    else:
        wqkv = torch.cat([sd[prefix + "attn.qkv.to_q.weight"].detach(), sd[prefix + "attn.qkv.to_kv.weight"].detach()], 0)
        bqkv = torch.cat([sd[prefix + "attn.qkv.to_q.bias"].detach(), sd[prefix + "attn.qkv.to_kv.bias"].detach()], 0).contiguous().float()
    dense = rpb_dense(sd[prefix + "attn.relative_position_bias_table"], sd[prefix + "attn.relative_position_index"])
    keep: Dict[str, Tensor] = {
        "norm1_w": f("norm1.weight"), "norm1_b": f("norm1.bias"),
        "rpb_dense": dense,
        "wqkv_fm": pack_frag(wqkv, dtype),
        "bqkv": bqkv,
        "wproj": t("attn.proj.weight"), "wproj_fm": pack_frag(sd[prefix + "attn.proj.weight"], dtype), "bproj": f("attn.proj.bias"),
        "norm2_w": f("norm2.weight"), "norm2_b": f("norm2.bias"),
    }
    if (prefix + "mlp.fc1.weight") in sd:      # Mlp (token_mlp 'ffn' / 'mlp'): fc1 / fc2 in the linear1 / linear2 slots, wdw9 = bdw = NULL (uf_ffn_fwd)
        keep.update({"w1_fm": pack_frag(sd[prefix + "mlp.fc1.weight"], dtype), "b1": f("mlp.fc1.bias"),
                     "w2_fm": pack_frag(sd[prefix + "mlp.fc2.weight"], dtype), "b2": f("mlp.fc2.bias")})
    else:
        keep.update({"w1_fm": pack_frag(sd[prefix + "mlp.linear1.0.weight"], dtype), "b1": f("mlp.linear1.0.bias"),
                     "wdw9": pack_dwconv(sd[prefix + "mlp.dwconv.0.weight"]), "bdw": f("mlp.dwconv.0.bias"),
                     "w2_fm": pack_frag(sd[prefix + "mlp.linear2.0.weight"], dtype), "b2": f("mlp.linear2.0.bias")})
    if conv:
        keep.update({"qkv_dw9": dw9, "qkv_bdw": bdw})
    if (prefix + "modulator.weight") in sd:
        keep["modulator"] = f("modulator.weight")
    tab = pack_rpb_table(dense)
    if tab is not None:
        keep["rpb_tab"] = tab
    bp = _lib.BlockParams()
    for name, _ in _lib.BlockParams._fields_:
        if name in ("shift", "heads"):
            continue
        setattr(bp, name, keep[name].data_ptr() if name in keep else None)
    bp.shift = int(shift)
    bp.heads = int(heads)
    return bp, keep


def cross_modulator_keys(sd: Dict[str, Tensor], prefix: str) -> bool:
    """True where the block under ``prefix`` carries a cross-modulator (``cross_modulator=True``, model.py:873-877)."""
    return (prefix + "cross_modulator.weight") in sd


def pack_cross(sd: Dict[str, Tensor], prefix: str, heads: int, dtype: torch.dtype):
    """``uf_cross_params`` of the block under ``prefix``: returns (CrossParams, keepalive dict); a block without a cross-modulator gives the
    all-NULL entry ``uf_uformer_fwd`` skips.  k and v^T are ``to_kv(cross_modulator.weight)`` (model.py:436-441 with attn_kv) evaluated in f32 and
    then rounded to ``dtype``: 64 rows that depend on parameters only, so they are projected here, once per pack, and not per forward.  k is NOT
    scaled (the kernel scales q); ``norm_cross`` is never read (model.py:947-948)."""
    cp = _lib.CrossParams()
    if not cross_modulator_keys(sd, prefix):
        return cp, {}
    g = lambda k: sd[prefix + k].detach()  # noqa: E731
    emb = g("cross_modulator.weight").float()
    n, C = emb.shape
    if n != 64 or C % heads or C // heads not in (16, 32):
        raise NotImplementedError(f"cross_modulator: built for 64 learned tokens and head_dim 16 or 32 (uf_cross_attn_fwd); this block has {n} tokens, "
                                  f"width {C} and {heads} heads")
    hd = C // heads
    kv = torch.nn.functional.linear(emb, g("cross_attn.qkv.to_kv.weight").float(), g("cross_attn.qkv.to_kv.bias").float())      # (64, 2C) = k | v
    keep: Dict[str, Tensor] = {
        "wq_fm": pack_frag(g("cross_attn.qkv.to_q.weight"), dtype),
        "bq": g("cross_attn.qkv.to_q.bias").float().clone().contiguous(),
        "k": kv[:, :C].reshape(64, heads, hd).permute(1, 0, 2).to(dtype).contiguous(),          # [heads][64][hd]
        "vt": kv[:, C:].reshape(64, heads, hd).permute(1, 2, 0).to(dtype).contiguous(),         # [heads][hd][64]
        "wp_fm": pack_frag(g("cross_attn.proj.weight"), dtype),
        "bp": g("cross_attn.proj.bias").float().clone().contiguous(),
    }
    for name, tns in keep.items():
        setattr(cp, name, tns.data_ptr())
    cp.heads = int(heads)
    return cp, keep


def pack_block4(sd: Dict[str, Tensor], prefix: str, heads: int, dtype: torch.dtype):
    if cross_modulator_keys(sd, prefix):
        raise NotImplementedError("cross_modulator is not built for 4x4-window blocks (the bottleneck of an img_size-64 model)")
    """``uf_block4_params`` of a 4x4-window block (row-major T weights, the (heads, 49) bias table): returns (Block4Params, keepalive)."""
    if conv_projection_keys(sd, prefix):
        raise NotImplementedError("token_projection='conv' is not built for 4x4-window blocks (the bottleneck of an img_size-64 model)")
    if (prefix + "mlp.fc1.weight") in sd:
        raise NotImplementedError("token_mlp='ffn' is not built for 4x4-window blocks (the bottleneck of an img_size-64 model)")
    if (prefix + "modulator.weight") in sd:
        raise NotImplementedError("a 4x4-window block with a modulator: the reference adds a (64, C) embedding to 16-token windows, "
                                  "which does not broadcast (model.py:868-869, :967-969)")
    f = lambda k: sd[prefix + k].detach().float().clone().contiguous()  # noqa: E731
    t = lambda k: sd[prefix + k].detach().to(dtype, copy=True).contiguous()  # noqa: E731
    keep: Dict[str, Tensor] = {
        "norm1_w": f("norm1.weight"), "norm1_b": f("norm1.bias"), "norm2_w": f("norm2.weight"), "norm2_b": f("norm2.bias"),
        "rpb4": pack_rpb_table4(sd[prefix + "attn.relative_position_bias_table"], sd[prefix + "attn.relative_position_index"]),
        "wqkv": torch.cat([sd[prefix + "attn.qkv.to_q.weight"].detach(), sd[prefix + "attn.qkv.to_kv.weight"].detach()], 0).to(dtype).contiguous(),
        "bqkv": torch.cat([sd[prefix + "attn.qkv.to_q.bias"].detach(), sd[prefix + "attn.qkv.to_kv.bias"].detach()], 0).float().contiguous(),
        "wproj": t("attn.proj.weight"), "bproj": f("attn.proj.bias"),
        "w1": t("mlp.linear1.0.weight"), "b1": f("mlp.linear1.0.bias"),
        "wdw9": pack_dwconv(sd[prefix + "mlp.dwconv.0.weight"]), "bdw": f("mlp.dwconv.0.bias"),
        "w2": t("mlp.linear2.0.weight"), "b2": f("mlp.linear2.0.bias"),
    }
    bp = _lib.Block4Params()
    for name, _ in _lib.Block4Params._fields_:
        if name != "heads":
            setattr(bp, name, keep[name].data_ptr())
    bp.heads = int(heads)
    return bp, keep


class PackedModel:
    """All packed weights of one ``Uformer`` + the ``uf_model_desc`` that points at them."""

    def __init__(self, cfg, sd: Dict[str, Tensor], dtype: torch.dtype):
        from .spec import STAGES
        self.dtype = dtype
        self.keep: List[object] = []
        shifts = cfg.block_shifts()
        wins = cfg.stage_windows()
        n_blocks = sum(cfg.depths)
        self.blocks = (_lib.BlockParams * n_blocks)()
        # 4x4-window bottleneck (img_size 64): its blocks go to uf_uformer_win4_fwd as uf_block4_params; their uf_block_params
        # slots stay zeroed (the whole-model entry skips them)
        self.win4 = wins[4] == 4
        self.bneck = (_lib.Block4Params * max(1, cfg.depths[4]))() if self.win4 else None
        # cross-modulator (decoder stages of a model built with cross_modulator=True): one uf_cross_params per block, aligned with `blocks`;
        # without the flag the descriptor's pointer stays NULL and the forward is the same launches as before
        self.cross = (_lib.CrossParams * n_blocks)() if getattr(cfg, "cross_modulator", False) else None
        i = 0
        for s in range(9):
            for b in range(cfg.depths[s]):
                if wins[s] == 4:
                    bp4, keep = pack_block4(sd, f"{STAGES[s]}.blocks.{b}.", cfg.num_heads[s], dtype)
                    self.bneck[b] = bp4
                else:
                    bp, keep = pack_block(sd, f"{STAGES[s]}.blocks.{b}.", cfg.num_heads[s], shifts[s][b], dtype)
                    self.blocks[i] = bp
                    if self.cross is not None:
                        cp, ckeep = pack_cross(sd, f"{STAGES[s]}.blocks.{b}.", cfg.num_heads[s], dtype)
                        self.cross[i] = cp
                        self.keep.append(ckeep)
                self.keep.append(keep)
                i += 1
        d = _lib.ModelDesc()
        d.embed_dim, d.dd_in, d.in_chans = cfg.embed_dim, cfg.dd_in, cfg.in_chans
        for s in range(9):
            d.depths[s] = cfg.depths[s]
        d.blocks = C.cast(self.blocks, C.POINTER(_lib.BlockParams))
        if self.cross is not None:
            d.cross = C.cast(self.cross, C.POINTER(_lib.CrossParams))
        g = {
            "in_w27": pack_input_proj(sd["input_proj.proj.0.weight"]),
            "in_b": sd["input_proj.proj.0.bias"].detach().float().clone().contiguous(),
            "out_w": pack_output_proj(sd["output_proj.proj.0.weight"]),
            "out_b": sd["output_proj.proj.0.bias"].detach().float().clone().contiguous(),
        }
        for name, tns in g.items():
            setattr(d, name, tns.data_ptr())
        self.keep.append(g)
        for k in range(4):
            dw = pack_downsample(sd[f"dowsample_{k}.conv.0.weight"], dtype)
            db = sd[f"dowsample_{k}.conv.0.bias"].detach().float().clone().contiguous()
            uw = pack_upsample(sd[f"upsample_{k}.deconv.0.weight"], dtype)
            ub = sd[f"upsample_{k}.deconv.0.bias"].detach().float().clone().contiguous()
            d.down_w[k], d.down_b[k], d.up_w[k], d.up_b[k] = dw.data_ptr(), db.data_ptr(), uw.data_ptr(), ub.data_ptr()
            # round 6: the Downsample weight also in the fragment-major layout its second form streams (2-byte operand types; N = 2C a multiple of 16)
            dwf = None
            if dtype in (torch.bfloat16, torch.float16) and dw.is_cuda and dw.shape[0] % 16 == 0 and dw.shape[1] % 32 == 0:
                from . import ops
                dwf = ops.pack_weight_fm(dw)
            d.down_w_fm[k] = dwf.data_ptr() if dwf is not None else None
            self.keep.append((dw, db, uw, ub, dwf))
        self.desc = d


def pack_conv(w: Tensor, dtype: torch.dtype) -> Tensor:
    """Conv2d weight (Cout,Cin,k,k) -> T[Cout_p][k*k*Cin_p] with [n][(ky*k + kx)*Cin_p + c] = w[n][c][ky][kx], Cout_p = Cout rounded up
    to 64, Cin_p = Cin rounded up to 32, zero padded (uf_conv_packed_elems, include/uformer_hip.h)."""
    cout, cin, k, _ = w.shape
    cp, np_ = (cin + 31) // 32 * 32, (cout + 63) // 64 * 64
    t = torch.zeros(np_, k, k, cp, dtype=dtype, device=w.device)
    t[:cout, :, :, :cin] = w.detach().permute(0, 2, 3, 1).to(dtype)
    return t.reshape(np_, -1).contiguous()


def pack_conv_dgrad(w: Tensor, dtype: torch.dtype) -> Tensor:
    """The input gradient of a 3x3 stride-1 pad-1 conv is the same conv with the flipped, transposed weight w'[c][n][2-ky][2-kx]:
    its pack_conv form, for uf_conv3x3_fwd's epilogue 3."""
    return pack_conv(w.detach().transpose(0, 1).flip(2, 3), dtype)


class PackedUNet:
    """All packed weights of one ``UNet`` + the ``uf_unet_desc`` that points at them."""

    def __init__(self, sd: Dict[str, Tensor], dim: int, dtype: torch.dtype):
        f = lambda k: sd[k].detach().float().clone().contiguous()  # noqa: E731
        d = _lib.UnetDesc()
        d.dim = dim
        keep: Dict[str, Tensor] = {
            "in_w27": pack_input_proj(sd["ConvBlock1.block.0.weight"]), "in_b": f("ConvBlock1.block.0.bias"),
            "c11_w1": sd["ConvBlock1.conv11.weight"].detach().float().reshape(dim, -1).clone().contiguous(),
            "c11_b1": f("ConvBlock1.conv11.bias"),
            "out_w": pack_output_proj(sd["conv10.weight"]), "out_b": f("conv10.bias"),
        }
        for name, tns in keep.items():
            setattr(d, name, tns.data_ptr())
        for i in range(9):
            p = f"ConvBlock{i + 1}."
            for slot, key in (("w2", "block.2"),) + ((("w0", "block.0"), ("w11", "conv11")) if i > 0 else ()):
                w = keep[f"{slot}.{i}"] = pack_conv(sd[p + key + ".weight"], dtype)
                b = keep[f"b{slot[1:]}.{i}"] = f(p + key + ".bias")
                getattr(d, slot)[i] = w.data_ptr()
                getattr(d, "b" + slot[1:])[i] = b.data_ptr()
        for k in range(4):
            w = keep[f"pool_w.{k}"] = pack_conv(sd[f"pool{k + 1}.weight"], dtype)
            b = keep[f"pool_b.{k}"] = f(f"pool{k + 1}.bias")
            d.pool_w[k], d.pool_b[k] = w.data_ptr(), b.data_ptr()
            w = keep[f"up_w.{k}"] = pack_upsample(sd[f"upv{k + 6}.weight"], dtype)
            b = keep[f"up_b.{k}"] = f(f"upv{k + 6}.bias")
            d.up_w[k], d.up_b[k] = w.data_ptr(), b.data_ptr()
        self.keep = keep
        self.desc = d
