"""GPU: the fused nonlinear kernels against their float64 reference TO THE BIT, on saturated-lattice inputs (tests/saturated_lattice.py has the
argument, the constructions, the conditions and the references; tests/test_saturated_reference.py checks them on the CPU).

Through the C ABI.  No tolerance appears in this file: on these inputs the LayerNorm, the softmax and the GELU of a kernel return exact values, the
rest is float32 accumulation of small integers, and a store to T rounds a T value.  Every element of every output is compared.  Operands that take
a leading dimension lie in the right half of a poisoned concat buffer (row stride 2C), dense outputs between poisoned guard rows; the NaN patterns
must come back intact.  Every kernel here is reduction-order free, runs twice and must reproduce its bits.  Per-entry-point figures go to
$UF_REPORT_DIR/parity_saturated.json.

f32 runs the LN-fused kernels with LayerNorm weight 0 (xn = bias + modulator): f32 keeps xn unrounded, so eps would show.  The row gather of
uf_ln_qkv_fwd is then NOT observed in f32; the 2-byte types observe it.
"""
import os

import pytest
import torch

import exact_lattice as X
import saturated_lattice as S
from edge_cases import PoisonedView
from exact_lattice import BF16, F16, F32, MODES, TAG, assert_exact

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ["uf_ln_linear_gelu_fwd", "uf_ffn_fwd", "uf_mlp_fwd", "uf_ln_qkv_fwd", "uf_ln_convqkv_fwd", "uf_dwconv_linear2_fwd", "uf_window_attention_fwd", "uf_window4_attention_fwd", "uf_lewin_attn_fwd", "uf_lewin_block_fwd",
                "uf_leff_fwd", "uf_lewin_attn_train_fwd", "uf_lewin_block_train_fwd"]
_RAN = set()


@pytest.fixture(autouse=True)
def _ran(request):
    yield
    _RAN.add(request.node.originalname)


@pytest.fixture(scope="module", autouse=True)
def _dump_report(request):
    yield
    X.dump_report("parity_saturated.json")
    rep = X.report()
    assert all(e["differing"] == 0 for e in rep.values()), {k: v for k, v in rep.items() if v["differing"]}
    mine = {n for n, f in request.module.__dict__.items() if n.startswith("test_") and callable(f)}
    if mine <= _RAN:
        missing = [n for n in ENTRY_POINTS if n not in rep]
        assert not missing, f"every test of this file ran, but these entry points were not compared: {missing}"


class variant:
    """UF_VARIANT for the calls inside the block (None: the key is absent, the shape picks); the selector is read on every call"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("UF_VARIANT")
        if self.value is None:
            os.environ.pop("UF_VARIANT", None)
        else:
            os.environ["UF_VARIANT"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("UF_VARIANT", None)
        else:
            os.environ["UF_VARIANT"] = self.old


def call(name, *args):
    from uformer_amd import _lib
    _lib.check(getattr(_lib.load(), name)(*args), name)
    torch.cuda.synchronize()


def st():
    return torch.cuda.current_stream().cuda_stream


def dt(dtype):
    from uformer_amd import ops
    return ops.uf_dtype(dtype)


def dev(t, dtype=F32):
    """a lattice tensor on the GPU as ``dtype``: the cast must be exact"""
    out = t.to(dtype)
    assert torch.equal(out.double(), t.double()), "lattice value is not representable in the operand type"
    return out.cuda().contiguous()


def fm(w, dtype):
    """(N, K) lattice weight -> the fragment-major pack the fused kernels stream"""
    from uformer_amd import ops
    return ops.pack_weight_fm(dev(w, dtype))


def stream_view(x64):
    """the f32 residual stream as encoder stages hold it: the right half of a 2C-wide poisoned concat buffer"""
    rows, C = x64.shape
    return PoisonedView(rows, C, F32, "cat", "cuda").fill(dev(x64))


def dense(rows, C, dtype, src=None):
    v = PoisonedView(rows, C, dtype, "guard", "cuda")
    return v if src is None else v.fill(dev(src.reshape(rows, C), dtype))


def twice(name, run, refs, dtypes):
    """``run`` -> {key: PoisonedView}, fresh buffers per call.  Both runs: guards intact; the first against the reference, the second against the first"""
    first = None
    for _ in range(2):
        outs, views = run()
        torch.cuda.synchronize()
        for v in list(outs.values()) + views:
            assert v.guard_intact(), f"{name}: wrote outside a view"
        bits = {k: v.live_bits().cpu() for k, v in outs.items()}
        if first is None:
            first = bits
            for k, v in outs.items():
                assert_exact(f"{name}/{k}", v.live().reshape(refs[k].shape), refs[k], dtypes[k])
        else:
            for k in bits:
                assert torch.equal(bits[k], first[k]), f"{name}: {k} differs between two runs on the same inputs"


# ---------------------------------------------------------------------------------------------------------------------------
# LN2 -> linear1 -> GELU, and the whole Mlp feed-forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("M,C", S.LNL1_CASES)
def test_ln_linear_gelu(dtype, M, C):
    c = S.lnl1_case(M, C, dtype)
    gm, bt, b1, w1 = dev(c["gamma"]), dev(c["beta"]), dev(c["b1"]), fm(c["w1"], dtype)

    def run():
        xi, out = stream_view(c["x"]), dense(M, 4 * C, dtype)
        call("uf_ln_linear_gelu_fwd", xi.ptr(), xi.ld, gm.data_ptr(), bt.data_ptr(), w1.data_ptr(), b1.data_ptr(), out.ptr(), M, 4 * C, C, dt(dtype), st())
        return {"h1": out}, [xi]
    twice(f"uf_ln_linear_gelu_fwd/{TAG[dtype]} M={M} C={C}", run, {"h1": c["h1"]}, {"h1": dtype})


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,M,C", S.FFN_CASES)
def test_ffn(dtype, B, M, C):
    c = S.ffn_case(B, M, C, dtype)
    gm, bt, b1, b2 = dev(c["gamma"]), dev(c["beta"]), dev(c["b1"]), dev(c["b2"])
    w1, w2 = fm(c["w1"], dtype), fm(c["w2"], dtype)
    for scale in S.FFN_SCALES:
        sc = None if scale is None else torch.tensor(scale, dtype=F32, device="cuda")

        def run():
            xi = stream_view(c["x"])
            call("uf_ffn_fwd", xi.ptr(), xi.ld, gm.data_ptr(), bt.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                 None if sc is None else sc.data_ptr(), B, M, C, dt(dtype), st())
            return {"x": xi}, []
        twice(f"uf_ffn_fwd/{TAG[dtype]} C={C} scale={scale}", run, {"x": S.ffn_out(c, B, scale)}, {"x": F32})


# ---------------------------------------------------------------------------------------------------------------------------
# LN1 -> roll -> window partition -> + modulator -> q | k | v^T
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C,heads,shift,use_mod", S.LNQKV_CASES)
def test_ln_qkv(dtype, B, H, W, C, heads, shift, use_mod):
    c = S.lnqkv_case(B, H, W, C, heads, shift, use_mod, dtype)
    M = B * H * W
    gm, bt, b, w = dev(c["gamma"]), dev(c["beta"]), dev(c["b"]), fm(c["w"], dtype)
    mod = dev(c["mod"]) if use_mod else None

    def run():
        xi = stream_view(c["x"])
        q, k, vt = (dense(M, C, dtype) for _ in range(3))
        call("uf_ln_qkv_fwd", xi.ptr(), xi.ld, gm.data_ptr(), bt.data_ptr(), None if mod is None else mod.data_ptr(), w.data_ptr(), b.data_ptr(),
             q.ptr(), k.ptr(), vt.ptr(), B, H, W, C, heads, shift, dt(dtype), st())
        return {"q": q, "k": k, "vt": vt}, [xi]
    twice(f"uf_ln_qkv_fwd/{TAG[dtype]} {B}x{H}x{W} C={C} heads={heads} shift={shift} mod={use_mod}", run,
          {"q": c["q"], "k": c["k"], "vt": c["vt"]}, {"q": dtype, "k": dtype, "vt": dtype})


@pytest.mark.parametrize("dtype", [BF16, F16], ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C,heads,shift", S.CONVQKV_CASES)
def test_ln_convqkv_live_layernorm(dtype, B, H, W, C, heads, shift):
    """the ConvProjection producer with a live LayerNorm, more than one head and the modulator (tests/test_gpu_convproj.py runs the lattice with LayerNorm weight 0)"""
    c = S.convqkv_case(B, H, W, C, heads, shift, dtype)
    M = B * H * W
    gm, bt, mod, dw9, bdw, bpw, wpw = dev(c["gamma"]), dev(c["beta"]), dev(c["mod"]), dev(c["dw9"]), dev(c["bdw"]), dev(c["bpw"]), fm(c["wpw"], dtype)

    def run():
        xi = stream_view(c["x"])
        q, k, vt = (dense(M, C, dtype) for _ in range(3))
        call("uf_ln_convqkv_fwd", xi.ptr(), xi.ld, gm.data_ptr(), bt.data_ptr(), mod.data_ptr(), dw9.data_ptr(), bdw.data_ptr(), wpw.data_ptr(), bpw.data_ptr(),
             q.ptr(), k.ptr(), vt.ptr(), B, H, W, C, heads, shift, dt(dtype), st())
        return {"q": q, "k": k, "vt": vt}, [xi]
    twice(f"uf_ln_convqkv_fwd/{TAG[dtype]} {B}x{H}x{W} C={C} heads={heads} shift={shift}", run, {"q": c["q"], "k": c["k"], "vt": c["vt"]}, {"q": dtype, "k": dtype, "vt": dtype})


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise 3x3 -> GELU -> linear2 -> residual
# ---------------------------------------------------------------------------------------------------------------------------
def run_leff2(dtype, B, H, W, C, variants):
    c = S.leff2_case(B, H, W, C, dtype)
    M = B * H * W
    w9, bdw, b2, w2 = dev(c["w9"]), dev(c["bdw"]), dev(c["b2"]), fm(c["w2"], dtype)
    for v in variants:
        if v is not None and dtype == F32 and v.startswith("leff2"):
            continue                                                     # the eight-producer-wave forms exist for the 2-byte types only

        def run():
            hi, xi = dense(M, 4 * C, dtype, c["h1"]), stream_view(c["x"])
            with variant(v):
                call("uf_dwconv_linear2_fwd", hi.ptr(), w9.data_ptr(), bdw.data_ptr(), w2.data_ptr(), b2.data_ptr(), xi.ptr(), xi.ld, B, H, W, C, dt(dtype), st())
            return {"x": xi}, [hi]
        twice(f"uf_dwconv_linear2_fwd/{TAG[dtype]} {B}x{H}x{W} C={C} {v}", run, {"x": c["out"]}, {"x": F32})


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C", S.LEFF2_CASES)
def test_dwconv_linear2(dtype, B, H, W, C):
    run_leff2(dtype, B, H, W, C, S.LEFF2_VARIANTS)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("case,variants", S.LEFF2_WALK_CASES, ids=["C32", "C64"])
def test_dwconv_linear2_persistent_walk(dtype, case, variants):
    """more tiles than resident workgroups: a workgroup walks several tiles (C = 32: the default launch; C = 64: "persist=1") or takes one"""
    run_leff2(dtype, *case, variants)


# ---------------------------------------------------------------------------------------------------------------------------
# window attention core
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,heads,hd,shift,kind", S.ATTN_CASES)
def test_window_attention(dtype, B, H, W, heads, hd, shift, kind):
    c = S.attn_case(B, H, W, heads, hd, shift, kind, dtype)
    n, C = c["n"], heads * hd
    bias = dev(c["bias"])

    def run():
        q, k, vt = (dense(n * 64, C, dtype, c[key]) for key in ("q", "k", "vt"))
        out = dense(n * 64, C, dtype)
        call("uf_window_attention_fwd", q.ptr(), k.ptr(), vt.ptr(), bias.data_ptr(), None, 0, out.ptr(), n, heads, hd, H, W, shift, dt(dtype), st())
        return {"o": out}, [q, k, vt]
    twice(f"uf_window_attention_fwd/{TAG[dtype]} {B}x{H}x{W} heads={heads} hd={hd} shift={shift} {kind}", run, {"o": c["o"]}, {"o": dtype})


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,heads,hd,kind", S.ATTN4_CASES)
def test_window4_attention(dtype, B, H, W, heads, hd, kind):
    """the 4 x 4-window core on raster q | k | v rows at row stride 3C + 16 inside a poisoned buffer; the output into the right half of a concat buffer"""
    c = S.attn4_case(B, H, W, heads, hd, kind, dtype)
    M, C = B * H * W, c["C"]
    tab = dev(c["tab"])

    def run():
        qkv = PoisonedView(M, 3 * C, dtype, "strided", "cuda").fill(dev(c["qkv"], dtype))
        out = PoisonedView(M, C, dtype, "cat", "cuda")
        call("uf_window4_attention_fwd", qkv.ptr(), qkv.ld, tab.data_ptr(), out.ptr(), out.ld, B, H, W, C, heads, dt(dtype), st())
        return {"o": out}, [qkv]
    twice(f"uf_window4_attention_fwd/{TAG[dtype]} {B}x{H}x{W} heads={heads} hd={hd} {kind}", run, {"o": c["o"]}, {"o": dtype})


# ---------------------------------------------------------------------------------------------------------------------------
# the fused window kernel and the block drivers
# ---------------------------------------------------------------------------------------------------------------------------
HALF = [BF16, F16]


def block_params(sd64, heads, shift, dtype):
    """uf_block_params of a block given by float64 lattice tensors under the reference's names (every cast must be exact)"""
    from uformer_amd import packing
    sd = {k: dev(v) for k, v in sd64.items()}
    for k, v in sd.items():
        if v.dim() == 2 and "table" not in k and "modulator" not in k:
            assert torch.equal(v.to(dtype).double().cpu(), sd64[k]), k
    sd["attn.relative_position_index"] = X.rpb_index(8).cuda()
    return packing.pack_block(sd, "", heads, shift, dtype)


class Workspace:
    """the block workspace filled with 0xFF bytes (NaN patterns in every type) and a guard behind it"""

    def __init__(self, M, C, dtype):
        from uformer_amd import _lib
        import edge_cases as E
        self.M, self.C, self.sz = M, C, torch.empty(0, dtype=dtype).element_size()
        self.nbytes = int(_lib.load().uf_block_workspace_bytes(M, C, dt(dtype)))
        self.buf, self.guard = E.poisoned_bytes(self.nbytes, 4096, 0xFF, "cuda")
        self.dtype = dtype

    def ptr(self):
        return self.buf.data_ptr()

    def h1(self):
        off = (self.M * self.C * self.sz + 255) // 256 * 256
        return self.buf[off:off + self.M * 4 * self.C * self.sz].view(self.dtype).reshape(self.M, 4 * self.C).clone()

    def intact(self):
        return bool((self.guard == 0xA5).all())


def drops_of(B):
    """per-image DropPath scales {0, 2} (and 1 where there is a third image)"""
    return [None, ((0.0, 2.0, 1.0) if B == 3 else (2.0, 0.0, 2.0, 0.0, 2.0)[:B])]


def block_ids(dtype):
    return [f"{B}x{H}x{W}-C{C}-s{shift}-{kind}-mod{int(m)}" for (B, H, W, C, shift, kind, m) in S.block_cases(dtype)]


def run_rows(name, fn, ref, M, C, dtype, x64, want_h1=None):
    """``fn(x view, workspace)`` updates the stream in place; twice; rows (and h1 from the workspace) against the reference, guards intact"""
    first = None
    for _ in range(2):
        xi, ws = stream_view(x64), Workspace(M, C, dtype)
        fn(xi, ws)
        torch.cuda.synchronize()
        assert xi.guard_intact() and ws.intact(), f"{name}: wrote outside the stream view or behind the workspace"
        bits = xi.live_bits().cpu()
        if first is None:
            first = bits
            assert_exact(f"{name}/rows", xi.live(), ref, F32)
            if want_h1 is not None:
                assert_exact(f"{name}/h1", ws.h1(), want_h1, dtype)
        else:
            assert torch.equal(bits, first), f"{name}: rows differ between two runs on the same inputs"
    return first


def block_test_cases():
    return [(dtype, case) for dtype in MODES for case in S.block_cases(dtype)]


def block_test_ids():
    return [f"{TAG[d]}-{i}" for d in MODES for i in block_ids(d)]


@pytest.mark.parametrize("dtype,case", block_test_cases(), ids=block_test_ids())
def test_lewin_attn_and_block(dtype, case):
    """uf_lewin_attn_fwd and uf_lewin_block_fwd (rows, and h1 read back from the workspace) in every form built for the shape.  f32: "uniform" and "table" only, LayerNorm weights 0."""
    B, H, W, C, shift, kind, use_mod = case
    c = S.block_case(B, H, W, C, shift, kind, use_mod, dtype)
    M = B * H * W
    bp, keep = block_params(S.block_state_dict(c, C), c["heads"], shift, dtype)
    rows = S.block_attn_out(c, B)
    z, a1, h1, out = S.block_ffn_half(c, rows, B, H, W, dtype)
    tag = f"{TAG[dtype]} {B}x{H}x{W} C={C} shift={shift} {kind} mod={use_mod}"
    seen = {}
    for v in S.block_variants(C, M // 64, dtype):
        def attn(xi, ws):
            with variant(v):
                call("uf_lewin_attn_fwd", bp, xi.ptr(), xi.ld, B, H, W, C, None, 0, dt(dtype), ws.ptr(), ws.nbytes, st())
        seen[v] = run_rows(f"uf_lewin_attn_fwd/{tag} {v}", attn, rows, M, C, dtype, c["x"])
    for v in S.block_variants(C, M // 64, dtype):
        def block(xi, ws):
            with variant(v):
                call("uf_lewin_block_fwd", bp, xi.ptr(), xi.ld, B, H, W, C, None, 0, dt(dtype), ws.ptr(), ws.nbytes, st())
        run_rows(f"uf_lewin_block_fwd/{tag} {v}", block, out, M, C, dtype, c["x"], want_h1=h1)

    def leff(xi, ws):
        call("uf_leff_fwd", bp, xi.ptr(), xi.ld, B, H, W, C, dt(dtype), ws.ptr(), ws.nbytes, st())
    run_rows(f"uf_leff_fwd/{tag}", leff, out, M, C, dtype, rows, want_h1=h1)


def train_cases():
    return [(dtype, case) for dtype in HALF for case in S.block_cases(dtype)]


@pytest.mark.parametrize("dtype,case", train_cases(), ids=[f"{TAG[d]}-{i}" for d in HALF for i in block_ids(d)])
def test_lewin_train_forms(dtype, case):
    """uf_lewin_attn_train_fwd: the new rows (out of place) and every side store -- xn, q with the plain scale, k, v^T, o in window-row order, z and the
    linear1 pre-activation a1 in token order -- are the lattice values, with and without DropPath scales; uf_lewin_block_train_fwd: the block's rows."""
    B, H, W, C, shift, kind, use_mod = case
    c = S.block_case(B, H, W, C, shift, kind, use_mod, dtype)
    M, heads = B * H * W, c["heads"]
    n = M // 64
    bp, keep = block_params(S.block_state_dict(c, C), heads, shift, dtype)
    tag = f"{TAG[dtype]} {B}x{H}x{W} C={C} shift={shift} {kind} mod={use_mod}"
    hv = lambda t: t.reshape(n, 64, heads, 32).permute(0, 2, 1, 3).contiguous()          # noqa: E731
    for drop in (drops_of(B) if B <= 3 else drops_of(B)[1:]):                              # the 320-window case (the 4-wave launch of C = 256): one setting
        rows = S.block_attn_out(c, B, drop)
        z, a1, h1, out = S.block_ffn_half(c, rows, B, H, W, dtype, drop=drop)
        refs = {"x1": rows, "xn": c["xn"], "q": hv(c["q_plain"].double()), "k": hv(c["P"][:, C:2 * C]), "vt": hv(c["P"][:, 2 * C:]).transpose(2, 3).contiguous(),
                "o": c["o"], "z": z, "a1": a1}
        types = {k: (F32 if k == "x1" else dtype) for k in refs}
        dv = None if drop is None else torch.tensor(drop, dtype=F32, device="cuda")

        def run():
            xi = stream_view(c["x"])
            o = {"x1": PoisonedView(M, C, F32, "cat", "cuda")}
            for k in ("xn", "q", "k", "vt", "o", "z"):
                o[k] = dense(M, C, dtype)
            o["a1"] = dense(M, 4 * C, dtype)
            call("uf_lewin_attn_train_fwd", bp, xi.ptr(), xi.ld, o["x1"].ptr(), o["x1"].ld, B, H, W, C, None if dv is None else dv.data_ptr(), dt(dtype),
                 *(o[k].ptr() for k in ("xn", "q", "k", "vt", "o", "z", "a1")), st())
            assert torch.equal(xi.live().cpu().double(), c["x"]), "the training form changed its input"
            return o, [xi]
        twice(f"uf_lewin_attn_train_fwd/{tag} drop={drop}", run, refs, types)

        def block(xi, ws):
            call("uf_lewin_block_train_fwd", bp, xi.ptr(), xi.ld, B, H, W, C, None if dv is None else dv.data_ptr(), None if dv is None else dv.data_ptr(),
                 dt(dtype), ws.ptr(), ws.nbytes, st())
        run_rows(f"uf_lewin_block_train_fwd/{tag} drop={drop}", block, out, M, C, dtype, c["x"], want_h1=h1)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,M,C", S.FFN_CASES)
def test_mlp_block_half(dtype, B, M, C):
    """uf_mlp_fwd: the FFN half of an Mlp block through its descriptor -- the fused kernel, and the unfused pair of launches ("ffn=1"; the default at C = 512)"""
    from uformer_amd import _lib
    c = S.ffn_case(B, M, C, dtype)
    keep = [dev(c["gamma"]), dev(c["beta"]), fm(c["w1"], dtype), dev(c["b1"]), fm(c["w2"], dtype), dev(c["b2"])]
    bp = _lib.BlockParams()
    bp.norm2_w, bp.norm2_b, bp.w1_fm, bp.b1, bp.w2_fm, bp.b2 = (t.data_ptr() for t in keep)
    bp.heads, bp.shift = max(1, C // 32), 0
    H, W = 8, M // B // 8
    for v in ((None, "ffn=1") if M >= C else (None,)):                                     # below M = C "ffn=1" falls back to the fused kernel
        def run(xi, ws):
            with variant(v):
                call("uf_mlp_fwd", bp, xi.ptr(), xi.ld, B, H, W, C, dt(dtype), ws.ptr(), ws.nbytes, st())
        run_rows(f"uf_mlp_fwd/{TAG[dtype]} M={M} C={C} {v}", run, S.ffn_out(c, B, None), M, C, dtype, c["x"])
