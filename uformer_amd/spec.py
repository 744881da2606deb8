"""Host-side description of the reference's ``Uformer`` boundary: constructor kwargs,
the ``state_dict`` key layout and the per-stage geometry.

Pure Python / torch-CPU, no HIP.  References:
  * constructor kwargs            /root/reference model.py:1070-1077
  * arch factory (T/S/B kwargs)   utils/model_utils.py:56-81
  * shift / window clamp          model.py:863-866, :1030
  * state_dict layout             SURVEY.md Appendix C (probed from model.py)
"""
from __future__ import annotations

import dataclasses
import hashlib
import math
from typing import Dict, Iterator, List, Sequence, Tuple

import torch

STAGES = ("encoderlayer_0", "encoderlayer_1", "encoderlayer_2", "encoderlayer_3", "conv",
          "decoderlayer_0", "decoderlayer_1", "decoderlayer_2", "decoderlayer_3")


@dataclasses.dataclass(frozen=True)
class UformerConfig:
    img_size: int = 256
    in_chans: int = 3
    dd_in: int = 3
    embed_dim: int = 32
    depths: Tuple[int, ...] = (2, 2, 2, 2, 2, 2, 2, 2, 2)
    num_heads: Tuple[int, ...] = (1, 2, 4, 8, 16, 16, 8, 4, 2)
    win_size: int = 8
    mlp_ratio: float = 4.0
    modulator: bool = False
    shift_flag: bool = True
    token_mlp: str = "leff"      # 'leff' (LeFF) or 'ffn' / 'mlp' (Mlp: fc1 -> GELU -> fc2, model.py:890-893)
    token_projection: str = "linear"   # 'linear' (LinearProjection) or 'conv' (ConvProjection: three SepConv2d per window, model.py:381-410)
    cross_modulator: bool = False      # decoder blocks attend to 64 learned tokens in front of their window attention (model.py:873-877, :945-949)

    def mlp_is_ffn(self) -> bool:
        return self.token_mlp in ("ffn", "mlp")

    # ---- geometry -------------------------------------------------------------------
    def stage_dims(self) -> List[int]:
        """Channel width of the LeWin blocks of each of the 9 stages (model.py:1104-1245)."""
        e = self.embed_dim
        return [e, 2 * e, 4 * e, 8 * e, 16 * e, 16 * e, 8 * e, 4 * e, 2 * e]

    def stage_res_div(self) -> List[int]:
        """Resolution divisor of each stage relative to the input image."""
        return [1, 2, 4, 8, 16, 8, 4, 2, 1]

    def stage_has_modulator(self, s: int) -> bool:
        """Only decoder stages receive ``modulator`` (model.py:1197,1213,1229,1245)."""
        return self.modulator and s >= 5

    def stage_has_cross_modulator(self, s: int) -> bool:
        """Only decoder stages receive ``cross_modulator`` (model.py:1197,1213,1229,1245)."""
        return self.cross_modulator and s >= 5

    def stage_windows(self) -> List[int]:
        """Constructor-time window of each stage: ``win_size``, clamped to the stage's resolution where that is not larger
        (model.py:863-866).  At img_size 64 the bottleneck (resolution 4) gets 4x4 windows."""
        out = []
        for s in range(9):
            res = self.img_size // self.stage_res_div()[s]
            out.append(res if res <= self.win_size else self.win_size)
        return out

    def block_shifts(self) -> List[List[int]]:
        """Constructor-time shift of every block (model.py:1030 then the clamp :863-866)."""
        out = []
        for s, d in enumerate(self.depths):
            res = self.img_size // self.stage_res_div()[s]
            row = []
            for i in range(d):
                sh = 0 if (i % 2 == 0 or not self.shift_flag) else self.win_size // 2
                if res <= self.win_size:
                    sh = 0
                row.append(sh)
            out.append(row)
        return out

    def unsupported_clamp(self):
        """None if every stage runs on a window this project builds (8, or 4 for the bottleneck alone), else (stage index,
        resolution, window the reference would use) of the first stage that does not."""
        for s, win in enumerate(self.stage_windows()):
            if win == self.win_size == 8 or (s == 4 and win == 4):
                continue
            return s, self.img_size // self.stage_res_div()[s], win
        return None

    def input_multiple(self) -> int:
        """H and W of a forward input must be multiples of this: 2^s x window at every stage (128, or 64 with a 4x4 bottleneck)."""
        return max((1 << min(s, 8 - s)) * w for s, w in enumerate(self.stage_windows()))

    def upsample_io(self) -> List[Tuple[int, int]]:
        """(Cin, Cout) of upsample_0..3 (model.py:1182,1198,1214,1230)."""
        e = self.embed_dim
        return [(16 * e, 8 * e), (16 * e, 4 * e), (8 * e, 2 * e), (4 * e, e)]


MAX_DD_IN = 8        # input planes the stem kernels and their backward take
MAX_IN_CHANS = 4     # output planes the head kernels and their backward take


def check_image_chans(dd_in: int, in_chans: int) -> None:
    """The image channel counts this project runs.  The reference adds the input to the output exactly when ``dd_in == 3`` (model.py:1305), which
    needs an output of 3 planes: with ``in_chans`` 2 or 4 its forward raises, with 1 it broadcasts the single plane onto the three by accident."""
    if dd_in == 3 and in_chans != 3:
        raise ValueError(f"dd_in={dd_in} adds the input image to the output (global residual, model.py:1305), so in_chans={in_chans} must be 3 as well; "
                         f"a model without the residual takes any other dd_in")
    if not (isinstance(dd_in, int) and 1 <= dd_in <= MAX_DD_IN):
        raise NotImplementedError(f"dd_in={dd_in}: the HIP stem is built for 1..{MAX_DD_IN} input planes")
    if not (isinstance(in_chans, int) and 1 <= in_chans <= MAX_IN_CHANS):
        raise NotImplementedError(f"in_chans={in_chans}: the HIP head is built for 1..{MAX_IN_CHANS} output planes")


def arch_config(name: str, img_size: int = 256, dd_in: int = 3) -> UformerConfig:
    """kwargs of ``utils.get_arch`` (utils/model_utils.py:65-78); 'tiny' is BASELINE config 0."""
    if name == "Uformer_T":
        return UformerConfig(img_size=img_size, embed_dim=16, modulator=True)
    if name == "Uformer_S":
        return UformerConfig(img_size=img_size, embed_dim=32, modulator=True)
    if name == "Uformer_B":
        return UformerConfig(img_size=img_size, embed_dim=32, depths=(1, 2, 8, 8, 2, 8, 8, 2, 1),
                             modulator=True, dd_in=dd_in)
    if name == "tiny":   # BASELINE.json configs[0]: embed_dim=16, depths [1]*9
        return UformerConfig(img_size=img_size, embed_dim=16, depths=(1,) * 9, modulator=True)
    if name == "tiny32":  # smallest head_dim-32 model, used by the GPU parity tests
        return UformerConfig(img_size=img_size, embed_dim=32, depths=(1, 2, 2, 2, 2, 2, 2, 2, 1), modulator=True)
    if name == "tiny64":  # tiny32's shape at twice the width: head_dim 64 at every stage, C = 1024 at the bottleneck and dec0
        return UformerConfig(img_size=img_size, embed_dim=64, depths=(1, 2, 2, 2, 2, 2, 2, 2, 1), modulator=True)
    raise ValueError(f"unknown arch {name!r}")


# ---- state_dict layout ------------------------------------------------------------------
def block_spec(prefix: str, C: int, heads: int, win: int, modulator: bool,
               mlp_ratio: float = 4.0, mod_win: int = None, token_mlp: str = "leff",
               token_projection: str = "linear", cross_modulator: bool = False) -> Iterator[Tuple[str, Tuple[int, ...], str]]:
    """(key, shape, kind) of one LeWinTransformerBlock, in registration order.  ``win``: the block's (clamped) window;
    ``mod_win`` (default ``win``): the unclamped window the modulator embedding is sized by (model.py:868-869);
    ``token_mlp``: 'leff', or 'ffn' / 'mlp' for the reference's Mlp (``mlp.fc1`` / ``mlp.fc2``, model.py:623-631);
    ``token_projection``: 'linear', or 'conv' for the reference's ConvProjection (``attn.qkv.to_{q,k,v}.{depthwise,pointwise}``, model.py:344-392);
    ``cross_modulator``: the block carries ``cross_modulator`` / ``cross_attn`` / ``norm_cross`` (model.py:873-877; ``cross_attn`` is an Attention, whose
    projection is a LinearProjection whatever ``token_projection`` says, :558; ``norm_cross`` is registered and never read, :947-948)."""
    hid = int(C * mlp_ratio)
    mw = win if mod_win is None else mod_win
    if modulator:
        yield prefix + "modulator.weight", (mw * mw, C), "embedding"
    if cross_modulator:
        yield prefix + "cross_modulator.weight", (mw * mw, C), "embedding"
        yield prefix + "cross_attn.qkv.to_q.weight", (C, C), "linear_w"
        yield prefix + "cross_attn.qkv.to_q.bias", (C,), "linear_b"
        yield prefix + "cross_attn.qkv.to_kv.weight", (2 * C, C), "linear_w"
        yield prefix + "cross_attn.qkv.to_kv.bias", (2 * C,), "linear_b"
        yield prefix + "cross_attn.proj.weight", (C, C), "linear_w"
        yield prefix + "cross_attn.proj.bias", (C,), "linear_b"
        yield prefix + "norm_cross.weight", (C,), "ln_w"
        yield prefix + "norm_cross.bias", (C,), "ln_b"
    yield prefix + "norm1.weight", (C,), "ln_w"
    yield prefix + "norm1.bias", (C,), "ln_b"
    yield prefix + "attn.relative_position_bias_table", ((2 * win - 1) ** 2, heads), "rpb"
    yield prefix + "attn.relative_position_index", (win * win, win * win), "rpi"
    if token_projection == "conv":
        for j in "qkv":
            yield prefix + f"attn.qkv.to_{j}.depthwise.weight", (C, 1, 3, 3), "conv_w"
            yield prefix + f"attn.qkv.to_{j}.depthwise.bias", (C,), "conv_b"
            yield prefix + f"attn.qkv.to_{j}.pointwise.weight", (C, C, 1, 1), "conv_w"
            yield prefix + f"attn.qkv.to_{j}.pointwise.bias", (C,), "conv_b"
    else:
        yield prefix + "attn.qkv.to_q.weight", (C, C), "linear_w"
        yield prefix + "attn.qkv.to_q.bias", (C,), "linear_b"
        yield prefix + "attn.qkv.to_kv.weight", (2 * C, C), "linear_w"
        yield prefix + "attn.qkv.to_kv.bias", (2 * C,), "linear_b"
    yield prefix + "attn.proj.weight", (C, C), "linear_w"
    yield prefix + "attn.proj.bias", (C,), "linear_b"
    yield prefix + "norm2.weight", (C,), "ln_w"
    yield prefix + "norm2.bias", (C,), "ln_b"
    if token_mlp in ("ffn", "mlp"):
        yield prefix + "mlp.fc1.weight", (hid, C), "linear_w"
        yield prefix + "mlp.fc1.bias", (hid,), "linear_b"
        yield prefix + "mlp.fc2.weight", (C, hid), "linear_w"
        yield prefix + "mlp.fc2.bias", (C,), "linear_b"
        return
    yield prefix + "mlp.linear1.0.weight", (hid, C), "linear_w"
    yield prefix + "mlp.linear1.0.bias", (hid,), "linear_b"
    yield prefix + "mlp.dwconv.0.weight", (hid, 1, 3, 3), "conv_w"
    yield prefix + "mlp.dwconv.0.bias", (hid,), "conv_b"
    yield prefix + "mlp.linear2.0.weight", (C, hid), "linear_w"
    yield prefix + "mlp.linear2.0.bias", (C,), "linear_b"


def state_dict_spec(cfg: UformerConfig) -> List[Tuple[str, Tuple[int, ...], str]]:
    """Every key of the reference ``Uformer.state_dict()`` with shape, in reference order."""
    e = cfg.embed_dim
    dims = cfg.stage_dims()
    wins = cfg.stage_windows()
    spec: List[Tuple[str, Tuple[int, ...], str]] = []
    spec.append(("input_proj.proj.0.weight", (e, cfg.dd_in, 3, 3), "conv_w"))
    spec.append(("input_proj.proj.0.bias", (e,), "conv_b"))
    spec.append(("output_proj.proj.0.weight", (cfg.in_chans, 2 * e, 3, 3), "conv_w"))
    spec.append(("output_proj.proj.0.bias", (cfg.in_chans,), "conv_b"))

    def stage(s: int):
        for i in range(cfg.depths[s]):
            spec.extend(block_spec(f"{STAGES[s]}.blocks.{i}.", dims[s], cfg.num_heads[s],
                                   wins[s], cfg.stage_has_modulator(s), cfg.mlp_ratio, mod_win=cfg.win_size, token_mlp=cfg.token_mlp,
                                   token_projection=cfg.token_projection, cross_modulator=cfg.stage_has_cross_modulator(s)))

    for s in range(4):
        stage(s)
        spec.append((f"dowsample_{s}.conv.0.weight", (2 * dims[s], dims[s], 4, 4), "conv_w"))
        spec.append((f"dowsample_{s}.conv.0.bias", (2 * dims[s],), "conv_b"))
    stage(4)
    for k, (cin, cout) in enumerate(cfg.upsample_io()):
        spec.append((f"upsample_{k}.deconv.0.weight", (cin, cout, 2, 2), "deconv_w"))
        spec.append((f"upsample_{k}.deconv.0.bias", (cout,), "conv_b"))
        stage(5 + k)
    return spec


def relative_position_index(win: int) -> torch.Tensor:
    """(win², win²) int64 buffer, model.py:467-477: (yi-yj+win-1)*(2win-1) + (xi-xj+win-1)."""
    c = torch.arange(win)
    ys, xs = torch.meshgrid(c, c, indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    return ((ys[:, None] - ys[None, :] + win - 1) * (2 * win - 1)
            + (xs[:, None] - xs[None, :] + win - 1)).to(torch.int64)


def synth_state_dict(cfg: UformerConfig, seed: int = 1234) -> Dict[str, torch.Tensor]:
    """Deterministic "trained-like" weights in the reference layout (set W1).

    Every tensor is drawn from its own CPU generator seeded by (seed, key), so the result
    does not depend on key order.  Biases, LN affine params and the relative-position
    tables are non-trivial so those code paths are exercised by the parity tests.
    """
    return _synth(state_dict_spec(cfg), seed)


def unet_state_dict_spec(dim: int = 32) -> List[Tuple[str, Tuple[int, ...], str]]:
    """(key, shape, kind) of the reference's ``UNet(dim=dim)`` state_dict in its order (model.py:128-152)."""
    spec: List[Tuple[str, Tuple[int, ...], str]] = []

    def block(name, cin, cout):
        spec.extend([(f"{name}.block.0.weight", (cout, cin, 3, 3), "conv_w"), (f"{name}.block.0.bias", (cout,), "conv_b"),
                     (f"{name}.block.2.weight", (cout, cout, 3, 3), "conv_w"), (f"{name}.block.2.bias", (cout,), "conv_b"),
                     (f"{name}.conv11.weight", (cout, cin, 1, 1), "conv_w"), (f"{name}.conv11.bias", (cout,), "conv_b")])

    block("ConvBlock1", 3, dim)
    for k in range(1, 5):
        c = dim * 2 ** (k - 1)
        spec.extend([(f"pool{k}.weight", (c, c, 4, 4), "conv_w"), (f"pool{k}.bias", (c,), "conv_b")])
        block(f"ConvBlock{k + 1}", c, 2 * c)
    for k in range(6, 10):
        cout = dim * 2 ** (9 - k)
        spec.extend([(f"upv{k}.weight", (2 * cout, cout, 2, 2), "deconv_w"), (f"upv{k}.bias", (cout,), "conv_b")])
        block(f"ConvBlock{k}", 2 * cout, cout)
    spec.extend([("conv10.weight", (3, dim, 3, 3), "conv_w"), ("conv10.bias", (3,), "conv_b")])
    return spec


def synth_unet_state_dict(dim: int = 32, seed: int = 1234) -> Dict[str, torch.Tensor]:
    """Deterministic weights of ``UNet(dim)`` in the reference layout, drawn as ``synth_state_dict`` draws them (per-key seeding,
    the conv_w / conv_b / deconv_w kinds)."""
    return _synth(unet_state_dict_spec(dim), seed)


def _synth(spec, seed: int) -> Dict[str, torch.Tensor]:
    out: Dict[str, torch.Tensor] = {}
    for key, shape, kind in spec:
        h = int.from_bytes(hashlib.sha256(f"{seed}:{key}".encode()).digest()[:6], "little")
        g = torch.Generator().manual_seed(h)
        if kind == "rpi":
            out[key] = relative_position_index(math.isqrt(shape[0]))
            continue
        n = torch.randn(shape, generator=g, dtype=torch.float32)
        if kind == "linear_w":
            t = 0.02 * n.clamp_(-2, 2) * 2.5          # a bit hotter than init so branches matter
        elif kind == "linear_b":
            t = 0.05 * n
        elif kind == "ln_w":
            t = 1.0 + 0.05 * n
        elif kind == "ln_b":
            t = 0.05 * n
        elif kind == "rpb":
            t = 0.2 * n
        elif kind == "embedding":
            t = 0.5 * n
        elif kind in ("conv_w", "deconv_w"):
            fan_in = shape[1] * shape[2] * shape[3] if kind == "conv_w" else shape[0] * shape[2] * shape[3]
            t = n.clamp_(-2, 2) * (0.6 / math.sqrt(fan_in))
        elif kind == "conv_b":
            t = 0.05 * n
        else:
            raise AssertionError(kind)
        out[key] = t.contiguous()
    return out


def synth_input(B: int, H: int, W: int, seed: int = 1234, channels: int = 3) -> torch.Tensor:
    """U[0,1) images of ``channels`` planes, the range ``load_img`` produces (utils/image_utils.py:31-35)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, channels, H, W, generator=g, dtype=torch.float32)
