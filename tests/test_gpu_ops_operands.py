"""Every ops wrapper that converts an operand gives the same bits whether it had to convert or not.

A wrapper converts (``_c`` / ``_f32`` / ``_pack_frag``) what is not contiguous or not of the dtype the entry point reads.  The converted
tensors are temporaries; ``ops._launch`` holds them until the entry point has returned ("Launch wrappers").  A temporary freed
too early hands its block to the next one, and the kernel reads one operand twice -- nothing faults, the result is wrong.  So per wrapper:

  (a) contiguous operands of the expected dtype;
  (b) "views":  the same values, every convertible operand a non-contiguous view;
  (c) "dtypes": the same values, every f32 operand given in bf16 and every 2-byte operand the wrapper casts to its leader's dtype in f32
      (``perm`` of mixup: int64);

and (b), (c) must ``torch.equal`` (a) on every output, with no input modified.  Values: k/8, |k| <= 64 (exact in bf16, so every
conversion is lossless), each operand drawn on its own, so operands of equal size differ and aliasing shows.  Shapes: the smallest the
kernels take (B = 1, 8x8, C = 32, one head of 32, 64 rows; two windows for attention)."""
import pytest
import torch

from uformer_amd import ops

pytestmark = pytest.mark.gpu

C, HEADS, HD, B, H, W, M = 32, 1, 32, 1, 8, 8, 64
HID = 4 * C
NW, WA, MA = 2, 16, 128                      # the attention wrappers: one 8x16 image = two windows
BF16, F32 = torch.bfloat16, torch.float32
_seed = [0]


def grid(*shape):
    """f32 (shape) of k/8, |k| <= 64, a fresh seed per call."""
    _seed[0] += 1
    g = torch.Generator().manual_seed(1000 + _seed[0])
    return torch.randint(-64, 65, shape, generator=g).float() / 8


class Op:
    """One operand: its canonical tensor and how the variants may present it.
    kind "conv": the wrapper converts dtype and layout; "lead": layout only (its dtype selects the kernel); "fixed": taken as it is."""

    def __init__(self, t, kind):
        self.t, self.kind = t.cuda(), kind

    def variant(self, which):
        t = self.t
        if self.kind == "fixed" or which == "plain":
            return t
        if which == "views":
            junk = torch.roll(t.flatten(), 1).view_as(t)
            return torch.stack([t, junk], -1)[..., 0]
        if self.kind == "lead":
            return t
        if t.dtype == torch.int32:
            return t.long()
        return t.to(BF16 if t.dtype == F32 else F32)


def f(*shape):
    return Op(grid(*shape), "conv")


def cast(T, *shape):
    return Op(grid(*shape).to(T), "conv")


def lead(T, *shape):
    return Op(grid(*shape).to(T), "lead")


def fixed(*shape):
    return Op(grid(*shape), "fixed")


# ---- the cases: name -> (takes an operand type, builder(T) -> (operands, call(tensors) -> outputs)) ------------------------------------
def c_layernorm(T):
    o = dict(x=f(M, C), gamma=f(C), beta=f(C), mod=f(64, C))
    return o, lambda t: ops.layernorm(t["x"], t["gamma"], t["beta"], B=B, H=H, W=W, dtype=T, windowed=True, modulator=t["mod"])


def c_linear(T):
    o = dict(a=lead(T, M, C), w=cast(T, 2 * C, C), b=f(2 * C))
    return o, lambda t: ops.linear(t["a"], t["w"], t["b"])


def c_linear_residual(T):
    o = dict(a=lead(T, M, C), w=cast(T, C, C), b=f(C), resid=f(M, C), scale=f(B))
    return o, lambda t: ops.linear_residual(t["a"], t["w"], t["b"], t["resid"], t["scale"], B, H, W)


def c_qkv(T):
    o = dict(a=lead(T, M, C), w=cast(T, 3 * C, C), b=f(3 * C))
    return o, lambda t: ops.qkv(t["a"], t["w"], t["b"], HEADS)


def c_ln_qkv(T):
    o = dict(x=f(M, C), gamma=f(C), beta=f(C), w=lead(T, 3 * C, C), b=f(3 * C), mod=f(64, C))
    return o, lambda t: ops.ln_qkv(t["x"], t["gamma"], t["beta"], t["w"], t["b"], HEADS, B=B, H=H, W=W, modulator=t["mod"])


def c_ln_linear_gelu(T):
    o = dict(x=f(M, C), gamma=f(C), beta=f(C), w=lead(T, HID, C), b=f(HID))
    return o, lambda t: ops.ln_linear_gelu(t["x"], t["gamma"], t["beta"], t["w"], t["b"])


def c_window_attention_core(T):
    o = dict(q=lead(T, NW, HEADS, 64, HD), k=lead(T, NW, HEADS, 64, HD), vt=lead(T, NW, HEADS, HD, 64), bias=f(HEADS, 64, 64), mask=f(NW, 64, 64))
    return o, lambda t: ops.window_attention_core(t["q"], t["k"], t["vt"], t["bias"], H=H, W=WA, mask=t["mask"])


def c_dwconv3x3_gelu(T):
    o = dict(x=lead(T, B, H, W, HID), w9=f(9, HID), b=f(HID))
    return o, lambda t: ops.dwconv3x3_gelu(t["x"], t["w9"], t["b"])


def c_dwconv3x3(T):
    o = dict(x=lead(T, B, H, W, HID), w9=f(9, HID), b=f(HID))
    return o, lambda t: ops.dwconv3x3(t["x"], t["w9"], t["b"])


def c_dwconv3x3_pre_gelu(gelu_in):
    def build(T):
        o = dict(x=lead(T, B, H, W, HID), w9=f(9, HID), b=f(HID))
        return o, lambda t: ops.dwconv3x3_pre_gelu(t["x"], t["w9"], t["b"], gelu_in=gelu_in)
    return build


def c_dwconv3x3_mul_dgelu(T):
    o = dict(dy=lead(T, B, H, W, HID), w9=f(9, HID), pre=cast(T, B, H, W, HID))
    return o, lambda t: ops.dwconv3x3_mul_dgelu(t["dy"], t["w9"], t["pre"])


def c_linear_pre_gelu(T):
    o = dict(a=lead(T, M, C), w=cast(T, HID, C), b=f(HID))
    return o, lambda t: ops.linear_pre_gelu(t["a"], t["w"], t["b"])


def c_linear_mul_dgelu(T):
    o = dict(dy=lead(T, M, HID), w_t=cast(T, C, HID), zb=f(C), pre=cast(T, M, C))
    return o, lambda t: ops.linear_mul_dgelu(t["dy"], t["w_t"], t["zb"], t["pre"])


def c_layernorm_bwd(T):
    o = dict(x=f(M, C), gamma=f(C), dy=f(M, C))
    return o, lambda t: ops.layernorm_bwd(t["x"], t["gamma"], t["dy"])


def c_layernorm_bwd_fused(with_cast):
    def build(T):
        o = dict(x=f(M, C), gamma=f(C), dy=lead(T, M, C), add=f(M, C), scale=f(B))
        return o, lambda t: ops.layernorm_bwd_fused(t["x"], t["gamma"], t["dy"], B, H, W, add=t["add"], windowed=True,
                                                    cast=dict(scale=t["scale"], windowed=True, shift=0) if with_cast else None)
    return build


def c_window_attention_bwd(fn):
    def build(T):
        o = dict(q=lead(T, NW, HEADS, 64, HD), k=cast(T, NW, HEADS, 64, HD), vt=cast(T, NW, HEADS, HD, 64), bias=f(HEADS, 64, 64), do=cast(T, MA, C),
                 mask=f(NW, 64, 64))
        return o, lambda t: getattr(ops, fn)(t["q"], t["k"], t["vt"], t["bias"], t["do"], H, WA, mask=t["mask"])
    return build


def c_dwconv3x3_bwd(T):
    o = dict(dc=lead(T, B, H, W, HID), w9=f(9, HID), pre=cast(T, B, H, W, HID))
    return o, lambda t: ops.dwconv3x3_bwd(t["dc"], t["w9"], t["pre"])


def c_dwconv_linear2(T):
    o = dict(h1=lead(T, B, H, W, HID), w9=f(9, HID), bdw=f(HID), w2=cast(T, C, HID), b2=f(C), x=f(M, C))
    return o, lambda t: ops.dwconv_linear2(t["h1"], t["w9"], t["bdw"], t["w2"], t["b2"], t["x"])


def c_downsample(with_fm):
    def build(T):
        o = dict(x=f(M, C), w=lead(T, 2 * C, 16 * C), b=f(2 * C))
        if with_fm:
            o["w_fm"] = Op(ops.pack_weight_fm(o["w"].t), "lead")
        return o, lambda t: ops.downsample(t["x"], t["w"], t["b"], B, H, W, w_fm=t.get("w_fm"))
    return build


def c_upsample(T):
    o = dict(x=f(M, C), w=lead(T, 4 * (C // 2), C), b=f(C // 2))
    return o, lambda t: ops.upsample(t["x"], t["w"], t["b"], B, H, W)


def c_input_proj(T):
    o = dict(img=f(B, 3, H, W), w27=f(27, C), b=f(C))
    return o, lambda t: ops.input_proj(t["img"], t["w27"], t["b"])


def c_output_proj(T):
    o = dict(x=f(M, C), w=f(3, 9, C), b=f(3), img=f(B, 3, H, W))
    return o, lambda t: ops.output_proj(t["x"], t["w"], t["b"], B, H, W, img=t["img"])


def c_mixup(T):
    o = dict(x=f(2, 3, H, W), lam=f(2), perm=Op(torch.tensor([1, 0], dtype=torch.int32), "conv"))
    return o, lambda t: ops.mixup(t["x"], t["lam"], t["perm"])


def c_window4_attention(T):
    o = dict(qkv=lead(T, M, 3 * C), rpb4=f(HEADS, 49))
    return o, lambda t: ops.window4_attention(t["qkv"], t["rpb4"], B, H, W, HEADS)


def c_window4_attention_bwd(T):
    o = dict(qkv=lead(T, M, 3 * C), rpb4=f(HEADS, 49), do=cast(T, M, C))
    return o, lambda t: ops.window4_attention_bwd(t["qkv"], t["rpb4"], t["do"], B, H, W, HEADS)


def c_ffn(T):      # in place on x: every call gets its own copy, the copy is the output
    o = dict(x=fixed(M, C), gamma=f(C), beta=f(C), w1=lead(T, HID, C), b1=f(HID), w2=cast(T, C, HID), b2=f(C), scale=f(B))
    return o, lambda t: ops.ffn(t["x"].clone(), t["gamma"], t["beta"], t["w1"], t["b1"], t["w2"], t["b2"], t["scale"], B)


def c_cross_attn(T):
    o = dict(x=fixed(M, C), wq=lead(T, C, C), bq=f(C), k=cast(T, HEADS, 64, HD), vt=cast(T, HEADS, HD, 64), wp=cast(T, C, C), bp=f(C))
    return o, lambda t: ops.cross_attn(t["x"].clone(), t["wq"], t["bq"], t["k"], t["vt"], t["wp"], t["bp"])


def c_ln_conv_qkv(T):
    o = dict(x=f(M, C), gamma=f(C), beta=f(C), dw9=f(3, 9, C), bdw=f(3, C), wpw=lead(T, 3 * C, C), bpw=f(3 * C), mod=f(64, C))
    return o, lambda t: ops.ln_conv_qkv(t["x"], t["gamma"], t["beta"], t["dw9"], t["bdw"], t["wpw"], t["bpw"], HEADS, B=B, H=H, W=W, modulator=t["mod"])


CASES = {                               # name: (the entry point takes bf16 and f32 operands, builder)
    "layernorm": (True, c_layernorm), "linear": (True, c_linear), "linear_residual": (True, c_linear_residual), "qkv": (True, c_qkv),
    "ln_qkv": (True, c_ln_qkv), "ln_linear_gelu": (True, c_ln_linear_gelu), "window_attention_core": (True, c_window_attention_core),
    "dwconv3x3_gelu": (True, c_dwconv3x3_gelu), "dwconv3x3": (True, c_dwconv3x3), "dwconv3x3_pre_gelu": (True, c_dwconv3x3_pre_gelu(False)),
    "dwconv3x3_pre_gelu_gelu_in": (True, c_dwconv3x3_pre_gelu(True)), "dwconv3x3_mul_dgelu": (True, c_dwconv3x3_mul_dgelu),
    "linear_pre_gelu": (True, c_linear_pre_gelu), "linear_mul_dgelu": (True, c_linear_mul_dgelu), "layernorm_bwd": (False, c_layernorm_bwd),
    "layernorm_bwd_fused": (True, c_layernorm_bwd_fused(False)), "layernorm_bwd_fused_cast": (True, c_layernorm_bwd_fused(True)),
    "window_attention_bwd": (True, c_window_attention_bwd("window_attention_bwd")),
    "window_attention_bwd_qkv": (True, c_window_attention_bwd("window_attention_bwd_qkv")), "dwconv3x3_bwd": (True, c_dwconv3x3_bwd),
    "dwconv_linear2": (True, c_dwconv_linear2), "downsample": (True, c_downsample(False)), "downsample_fm": (True, c_downsample(True)),
    "upsample": (True, c_upsample), "input_proj": (False, c_input_proj), "output_proj": (False, c_output_proj), "mixup": (False, c_mixup),
    "window4_attention": (True, c_window4_attention), "window4_attention_bwd": (True, c_window4_attention_bwd), "ffn": (True, c_ffn),
    "cross_attn": (True, c_cross_attn), "ln_conv_qkv": (True, c_ln_conv_qkv),
}
PARAMS = [pytest.param(name, T, which, id=f"{name}-{'bf16' if T == BF16 else 'f32'}-{which}")
          for name, (typed, _) in CASES.items() for T in ((BF16, F32) if typed else (F32,)) for which in ("views", "dtypes")]


def run(call, operands, which):
    given = {k: op.variant(which) for k, op in operands.items()}
    before = {k: v.clone() for k, v in given.items()}
    out = call(given)
    out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
    torch.cuda.synchronize()
    for k, v in given.items():
        assert torch.equal(v, before[k]), f"input {k} was modified"
    return given, out


@pytest.mark.parametrize("name,T,which", PARAMS)
def test_converted_operands_give_the_same_bits(name, T, which):
    _seed[0] = 100 * list(CASES).index(name)            # the same draw whichever tests are selected
    operands, call = CASES[name][1](T)
    vals = list(operands.values())
    assert not any(a.t.shape == b.t.shape and torch.equal(a.t.float(), b.t.float()) for i, a in enumerate(vals) for b in vals[i + 1:])
    _, ref = run(call, operands, "plain")
    given, got = run(call, operands, which)
    # the variant does present what it claims, with the same values
    for k, op in operands.items():
        assert torch.equal(given[k].float(), op.t.float())
        if op.kind != "fixed" and which == "views" and op.t.numel() > 1:
            assert not given[k].is_contiguous()
        if op.kind == "conv" and which == "dtypes":
            assert given[k].dtype != op.t.dtype
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.isfinite(r.float()).all(), f"output {i} of the plain call is not finite"
        assert g.dtype == r.dtype and g.shape == r.shape and torch.equal(g, r), f"output {i} differs under '{which}'"
