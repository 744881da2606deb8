"""GPU: every linear kernel against its float64 reference TO THE BIT, on integer-lattice inputs (tests/exact_lattice.py has the argument,
the two conditions, the case lists and the references; tests/test_exact_reference.py checks them on the CPU).

Through the C ABI, in f32 / bf16 / f16.  No tolerance appears in this file: a kernel with float32 accumulation returns the float64
result exactly, and where it stores type T, that result rounded once, round-to-nearest-even.  Strided sources and destinations carry a
sentinel in their pad columns and behind their last row that must come back intact.  An entry point that rejects a shape must return
its documented status.  Per-entry-point figures go to $UF_REPORT_DIR/parity_exact.json.

Inherent roundings (references mirror them with the same single IEEE operation, see exact_lattice):
  * LeakyReLU epilogues: one float32 multiply by float32(0.01) of the exact pre-activation;
  * the query third of uf_qkv_fwd / uf_qkv_grad_merge: one float32 multiply by float32(head_dim ** -0.5), then the store's rounding
    (exact for head widths 16 and 64);
  * uf_downsample_bwd / uf_upsample_cat_bwd store the input gradient as T before they widen it (tap by tap in the former): condition 2
    is asserted on those intermediates, so the rounding is the identity here.
"""
import pytest
import torch

import exact_lattice as X
from exact_lattice import BF16, F16, F32, MODES, PM1, PM2, SENTINEL, TAG, assert_exact

pytestmark = pytest.mark.gpu
HALF = [BF16, F16]


ENTRY_POINTS = ["uf_linear_fwd", "uf_qkv_fwd", "uf_linear_residual_fwd", "uf_downsample_fwd", "uf_downsample_fm_fwd", "uf_upsample_fwd", "uf_input_proj_fwd", "uf_output_proj_fwd",
                "uf_dwconv3x3_fwd", "uf_conv3x3_fwd", "uf_conv4s2_fwd", "uf_conv1x1_fwd", "uf_conv1x1_nchw_fwd", "uf_im2col", "uf_col2im", "uf_linear_wgrad", "uf_rows_sum",
                "uf_dwconv3x3_wgrad", "uf_conv3x3_bwd", "uf_downsample_bwd", "uf_upsample_cat_bwd", "uf_rpb_table_grad", "uf_rpb4_table_grad", "uf_residual_combine", "uf_grad_fork",
                "uf_qkv_grad_merge"]
_RAN = set()             # test functions of this file that have run in this process


@pytest.fixture(autouse=True)
def _ran(request):
    yield
    _RAN.add(request.node.originalname)


def check_report(request, exclude=None):
    """no element differs; and if every test function of this file was selected and has run (a run of the whole file, whatever -k / -m left of each function's
    cases), every entry point is in the report"""
    rep = X.report()
    assert all(e["differing"] == 0 for e in rep.values()), {k: v for k, v in rep.items() if v["differing"]}
    mine = {n for n, f in request.module.__dict__.items() if n.startswith("test_") and callable(f)} - {exclude}
    if mine <= _RAN:
        missing = [n for n in ENTRY_POINTS if n not in rep]
        assert not missing, f"every test of this file ran, but these entry points were not compared: {missing}"


@pytest.fixture(scope="module", autouse=True)
def _dump_report(request):
    yield
    X.dump_report()
    check_report(request)


def L():
    from uformer_amd import _lib
    return _lib.load()


def call(name, *args):
    from uformer_amd import _lib
    _lib.check(getattr(L(), name)(*args), name)
    torch.cuda.synchronize()


def status(name, *args):
    return getattr(L(), name)(*args)


def st():
    return torch.cuda.current_stream().cuda_stream


def dt(dtype):
    from uformer_amd import _lib
    return {F32: _lib.UF_F32, BF16: _lib.UF_BF16, F16: _lib.UF_F16}[dtype]


_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def keep(t):
    """a tensor whose data_ptr() goes into a call lives until the test ends: a temporary would be freed, and its block handed to the next allocation,
    before the kernel has read it"""
    _KEEP.append(t)
    return t


def dev(t, dtype=F32):
    """a lattice tensor on the GPU as ``dtype``: the cast must be exact"""
    out = t.to(dtype)
    assert torch.equal(out.double(), t), "lattice value is not representable in the operand type"
    return keep(out.cuda().contiguous())


class Strided:
    """(rows, C) live columns at column offset ``off`` of a (rows + 2, off + C + pad) allocation filled with the sentinel"""

    def __init__(self, rows, C, dtype=F32, pad=8, off=0, data=None):
        self.rows, self.C, self.off = rows, C, off
        self.buf = torch.full((rows + 2, off + C + pad), SENTINEL, dtype=dtype, device="cuda")
        self.ld = self.buf.shape[1]
        if data is not None:
            self.live()[:] = dev(data.reshape(rows, C), dtype)

    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def live(self):
        return self.buf[:self.rows, self.off:self.off + self.C]

    def intact(self):
        s = torch.full((), SENTINEL, dtype=self.buf.dtype, device="cuda")
        return bool((self.buf[self.rows:] == s).all() and (self.buf[:, :self.off] == s).all() and (self.buf[:, self.off + self.C:] == s).all())


def flat_guarded(n, dtype=F32, guard=64):
    """a dense output of n elements with a sentinel tail behind it"""
    return torch.full((n + guard,), SENTINEL, dtype=dtype, device="cuda")


def tail_intact(buf, n):
    return bool((buf[n:] == torch.full((), SENTINEL, dtype=buf.dtype, device="cuda")).all())


def staging_variants(dtype, K):
    """both staging paths of the dense GEMM where the LDS-DMA one exists (2-byte types, K a multiple of 64 and at least two K tiles)"""
    return ["gemm_dma=0", "gemm_dma=1"] if dtype in HALF and K % 64 == 0 and K >= 128 else [None]


def set_variant(monkeypatch, v):
    if v is None:
        monkeypatch.delenv("UF_VARIANT", raising=False)
    else:
        monkeypatch.setenv("UF_VARIANT", v)


def twice(run):
    """a reduction must be bit-identical when run twice"""
    a = [t.clone() for t in run()]
    b = run()
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32) if u.dtype == F32 else u.view(torch.int16), v.view(torch.int32) if v.dtype == F32 else v.view(torch.int16)), "two runs differ"
    return b


# ---------------------------------------------------------------------------------------------------------------------------
# dense GEMM family
# ---------------------------------------------------------------------------------------------------------------------------
def run_linear(c, dtype, M, N, K):
    A, W, b = dev(c["A"], dtype), dev(c["W"], dtype), dev(c["bias"])
    out = flat_guarded(M * N, dtype)
    call("uf_linear_fwd", A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, 0, dt(dtype), st())
    assert tail_intact(out, M * N)
    return out[:M * N].reshape(M, N)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("M,N,K", X.GEMM_CASES)
def test_dense_gemm(dtype, M, N, K, monkeypatch):
    """uf_linear_fwd (act = 0) and uf_linear_residual_fwd, plain and windowed with shift 0 and 4, per-image scales from {0, 0.5, 1, 2}"""
    c = X.gemm_case(M, N, K)
    X.check_representable(c["P"], dtype)
    A, W, b = dev(c["A"], dtype), dev(c["W"], dtype), dev(c["bias"])
    for v in staging_variants(dtype, K):
        set_variant(monkeypatch, v)
        tag = f"{TAG[dtype]}/M{M}N{N}K{K}/{v}"
        assert_exact(f"uf_linear_fwd/{tag}", run_linear(c, dtype, M, N, K), c["P"], dtype)
        for mode, (B, H, Wd), shifts in (("plain", X.RES_PLAIN[M], [None]), ("windowed", X.RES_WINDOWED[M], [0, 4])):
            Mr = B * H * Wd
            resid = X.lattice((Mr, N), PM2, 7 + M + N)
            scale = torch.tensor([X.SCALES[(i + 1) % 4] for i in range(B)], dtype=torch.float64)
            for shift in shifts:
                for sc in (None, scale):
                    out = flat_guarded(Mr * N)
                    out[:Mr * N] = dev(resid).reshape(-1)                                   # in place: resid aliases out
                    call("uf_linear_residual_fwd", A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), out.data_ptr(), None if sc is None else dev(sc).data_ptr(),
                         B, H, Wd, N, K, int(shift is not None), shift or 0, dt(dtype), st())
                    ref = X.ref_residual(c["P"], resid, sc, B, H, Wd, None if shift is None else X.window_tokens(B, H, Wd, shift))
                    assert tail_intact(out, Mr * N)
                    assert_exact(f"uf_linear_residual_fwd/{tag}/{mode}{shift}/{'scaled' if sc is not None else 'unscaled'}", out[:Mr * N].reshape(Mr, N), ref, F32)
    # a windowed call on a map that is not whole windows is a shape error
    if M == 130:
        B, H, Wd = X.RES_PLAIN[M]
        out = torch.zeros(M, N, device="cuda")
        assert status("uf_linear_residual_fwd", A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), out.data_ptr(), None, B, H, Wd, N, K, 1, 4, dt(dtype), st()) == X.UF_ERR_SHAPE


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_linear_fwd_wide_tile(dtype, monkeypatch):
    """the 128-column tile configuration, which uf_linear_fwd takes only from 512 tiles of 128 x 128 on (exact_lattice.GEMM_WIDE_TILE_CASE)"""
    M, N, K = X.GEMM_WIDE_TILE_CASE
    assert N > 64 and ((M + 127) // 128) * ((N + 127) // 128) >= 512
    c = X.gemm_case(M, N, K)
    X.check_representable(c["P"], dtype)
    for v in staging_variants(dtype, K):
        set_variant(monkeypatch, v)
        assert_exact(f"uf_linear_fwd/{TAG[dtype]}/M{M}N{N}K{K}/{v}", run_linear(c, dtype, M, N, K), c["P"], dtype, tile=(128, 128))


@pytest.mark.parametrize("dtype", HALF, ids=TAG.get)
def test_linear_fwd_rounding_mode(dtype):
    """results past 2^p on purpose: the store must round to nearest even (truncation and round-half-away give other bits)"""
    c = X.gemm_rounding_case(dtype)
    prof = X.rounding_profile(c["P"], dtype)
    assert prof["away"] > 0 and prof["ties"] > 0
    assert_exact(f"uf_linear_fwd/{TAG[dtype]}/rounding", run_linear(c, dtype, 64, 32, 64), c["P"], dtype)


def run_qkv(c, dtype, M, C, heads):
    A, W, b = dev(c["A"], dtype), dev(c["W"], dtype), dev(c["bias"])
    outs = [flat_guarded(M * C, dtype) for _ in range(3)]
    call("uf_qkv_fwd", A.data_ptr(), W.data_ptr(), b.data_ptr(), *[o.data_ptr() for o in outs], M, C, heads, dt(dtype), st())
    assert all(tail_intact(o, M * C) for o in outs)
    return [o[:M * C] for o in outs]


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("M,C,heads", X.QKV_CASES)
def test_qkv(dtype, M, C, heads, monkeypatch):
    c = X.gemm_case(M, 3 * C, C)
    X.check_representable(c["P"][:, C:], dtype)
    refs = X.ref_qkv(c["P"], M, C, heads)
    for v in staging_variants(dtype, C):
        set_variant(monkeypatch, v)
        for name, got, ref in zip("qkv", run_qkv(c, dtype, M, C, heads), refs):
            assert_exact(f"uf_qkv_fwd/{TAG[dtype]}/M{M}C{C}h{heads}/{v}/{name}", got.reshape(ref.shape), ref, dtype)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_qkv_rejections_and_rounding(dtype):
    """M that is not whole 64-token windows: UF_ERR_SHAPE; a head width other than 16 / 32 / 64: UF_ERR_UNSUPPORTED; the rounding mode of the store"""
    buf = torch.zeros(1000 * 96, dtype=dtype, device="cuda")
    bias = torch.zeros(96, device="cuda")
    for M in X.QKV_REJECTED_M:
        assert status("uf_qkv_fwd", buf.data_ptr(), buf.data_ptr(), bias.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), M, 32, 1, dt(dtype), st()) == X.UF_ERR_SHAPE
    assert status("uf_qkv_fwd", buf.data_ptr(), buf.data_ptr(), bias.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 64, 32, 4, dt(dtype), st()) == X.UF_ERR_UNSUPPORTED
    if dtype in HALF:
        for M in (64, 192):
            C, heads = 32, 2                                     # head width 16: the query scale 1/4 is exact, only the store rounds
            c = X.gemm_rounding_case(dtype, M, 3 * C, C)
            assert X.rounding_profile(c["P"], dtype)["away"] > 0
            for name, got, ref in zip("qkv", run_qkv(c, dtype, M, C, heads), X.ref_qkv(c["P"], M, C, heads)):
                assert_exact(f"uf_qkv_fwd/{TAG[dtype]}/rounding/M{M}/{name}", got.reshape(ref.shape), ref, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# samplers, stem and head
# ---------------------------------------------------------------------------------------------------------------------------
def run_downsample(c, dtype, B, H, W, C, fm):
    from uformer_amd import ops, packing
    M, Mo = B * H * W, B * (H // 2) * (W // 2)
    x = Strided(M, C, data=X.to_rows(c["x"]))
    w = packing.pack_downsample(dev(c["wd"]), dtype).contiguous()
    assert torch.equal(w.double().cpu(), c["wd"].permute(0, 2, 3, 1).reshape(2 * C, -1))
    bias = dev(c["bd"])
    out = Strided(Mo, 2 * C, off=8)
    if fm is None:
        call("uf_downsample_fwd", x.ptr(), x.ld, w.data_ptr(), bias.data_ptr(), out.ptr(), out.ld, B, H, W, C, dt(dtype), st())
    else:
        w_fm = ops.pack_weight_fm(w) if fm else None
        call("uf_downsample_fm_fwd", x.ptr(), x.ld, w.data_ptr(), None if w_fm is None else w_fm.data_ptr(), bias.data_ptr(), out.ptr(), out.ld, B, H, W, C, dt(dtype), st())
    assert out.intact() and x.intact()
    return out.live()


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C", [(B, H, W, C) for B in X.SAMPLER_B for (H, W) in X.SAMPLER_MAPS for C in X.SAMPLER_C] + X.DOWN_PATCH_CASES)
def test_downsample_and_upsample(dtype, B, H, W, C):
    """uf_downsample_fwd and uf_downsample_fm_fwd (with and without the fragment-major weight) agree with each other and with the reference;
    uf_upsample_fwd writes the right half of a concat buffer whose left half holds the sentinel"""
    from uformer_amd import packing
    c = X.sampler_case(B, H, W, C)
    tag = f"{TAG[dtype]}/B{B}H{H}W{W}C{C}"
    ref = X.to_rows(c["down"])
    d0 = run_downsample(c, dtype, B, H, W, C, None)
    assert_exact(f"uf_downsample_fwd/{tag}", d0, ref, F32)
    for fm in ([False, True] if dtype in HALF and C % 8 == 0 else [False]):
        d1 = run_downsample(c, dtype, B, H, W, C, fm)
        assert_exact(f"uf_downsample_fm_fwd/{tag}/fm{int(fm)}", d1, ref, F32)
        assert torch.equal(d0.view(torch.int32), d1.view(torch.int32))
    if (B, H, W, C) in X.DOWN_PATCH_CASES:
        return
    M, Co = B * H * W, C // 2
    x = Strided(M, C, data=X.to_rows(c["x"]))
    w = packing.pack_upsample(dev(c["wu"]), dtype).contiguous()
    out = Strided(4 * M, Co, pad=0, off=Co)                      # columns [Co, 2 Co) of rows of 2 Co
    call("uf_upsample_fwd", x.ptr(), x.ld, w.data_ptr(), dev(c["bu"]).data_ptr(), out.ptr(), out.ld, B, H, W, C, Co, dt(dtype), st())
    assert out.intact() and x.intact()
    assert_exact(f"uf_upsample_fwd/{tag}", out.live(), X.to_rows(c["up"]), F32)


@pytest.mark.parametrize("E", X.SAMPLER_C)
@pytest.mark.parametrize("H,W", X.STEM_MAPS)
@pytest.mark.parametrize("B", X.SAMPLER_B)
def test_stem(B, H, W, E):
    """uf_input_proj_fwd (conv3x3 + LeakyReLU); f32"""
    from uformer_amd import packing
    c = X.stem_case(B, H, W, E)
    tag = f"f32/B{B}H{H}W{W}E{E}"
    M = B * H * W
    img = flat_guarded(B * 3 * H * W)
    img[:B * 3 * H * W] = dev(c["img"]).reshape(-1)
    out = Strided(M, E, off=E)
    call("uf_input_proj_fwd", img.data_ptr(), keep(packing.pack_input_proj(dev(c["w_in"]))).data_ptr(), dev(c["b_in"]).data_ptr(), out.ptr(), out.ld, B, 3, H, W, E, st())
    assert out.intact()
    assert_exact(f"uf_input_proj_fwd/{tag}", out.live(), X.to_rows(c["stem"]), F32)


@pytest.mark.parametrize("C2", X.HEAD_C)
@pytest.mark.parametrize("H,W", X.STEM_MAPS)
@pytest.mark.parametrize("B", X.SAMPLER_B)
def test_head(B, H, W, C2):
    """uf_output_proj_fwd at every width it supports, with and without the image residual; f32"""
    from uformer_amd import packing
    c = X.head_case(B, H, W, C2)
    n = B * 3 * H * W
    img = dev(c["img"])
    x = Strided(B * H * W, C2, data=X.to_rows(c["x"]))
    wo, bo = keep(packing.pack_output_proj(dev(c["w_out"]))), dev(c["b_out"])
    for add, ref in ((0, c["head"]), (1, c["head_img"])):
        y = flat_guarded(n)
        call("uf_output_proj_fwd", x.ptr(), x.ld, wo.data_ptr(), bo.data_ptr(), img.data_ptr(), y.data_ptr(), B, H, W, C2, add, st())
        assert tail_intact(y, n) and x.intact()
        assert_exact(f"uf_output_proj_fwd/f32/B{B}H{H}W{W}C{C2}/img{add}", y[:n].reshape(B, 3, H, W), ref, F32)


@pytest.mark.parametrize("C2", X.HEAD_C_REJECTED)
def test_head_rejects_other_widths(C2):
    B, H, W = 1, 8, 8
    x, w, bias, img, y = (keep(torch.zeros(n, device="cuda")) for n in (B * H * W * C2, 27 * C2, 3, B * 3 * H * W, B * 3 * H * W))
    for add in (0, 1):
        assert status("uf_output_proj_fwd", x.data_ptr(), C2, w.data_ptr(), bias.data_ptr(), img.data_ptr(), y.data_ptr(), B, H, W, C2, add, st()) == X.UF_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise stencil
# ---------------------------------------------------------------------------------------------------------------------------
def run_dwconv(x64, w64, b64, dtype, B, H, W, C):
    from uformer_amd import packing
    x = dev(X.to_rows(x64), dtype)
    w9 = packing.pack_dwconv(dev(w64))
    out = flat_guarded(B * H * W * C, dtype)
    call("uf_dwconv3x3_fwd", x.data_ptr(), w9.data_ptr(), None if b64 is None else dev(b64).data_ptr(), out.data_ptr(), B, H, W, C, 0, dt(dtype), st())
    assert tail_intact(out, B * H * W * C)
    return out[:B * H * W * C].reshape(B * H * W, C)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C", X.DWCONV_CASES)
def test_dwconv3x3(dtype, B, H, W, C):
    c = X.dwconv_case(B, H, W, C)
    for name, bias in (("plain", None), ("biased", c["bias"])):
        X.check_representable(c[name], dtype, step=0.5)
        assert_exact(f"uf_dwconv3x3_fwd/{TAG[dtype]}/B{B}H{H}W{W}C{C}/{name}", run_dwconv(c["x"], c["w"], bias, dtype, B, H, W, C), X.to_rows(c[name]), dtype, tile=(W, C))


@pytest.mark.parametrize("dtype", HALF, ids=TAG.get)
def test_dwconv3x3_rounding_mode(dtype):
    B, H, W, C = 1, 8, 16, 16
    x, w = X.lattice((B, C, H, W), X.rounding_values(dtype), 35), X.lattice((C, 1, 3, 3), PM1, 36)
    ref = torch.nn.functional.conv2d(x, w, None, padding=1, groups=C)
    prof = X.rounding_profile(ref, dtype)
    assert prof["away"] > 0 and prof["ties"] > 0
    assert_exact(f"uf_dwconv3x3_fwd/{TAG[dtype]}/rounding", run_dwconv(x, w, None, dtype, B, H, W, C), X.to_rows(ref), dtype, tile=(W, C))
    xb, wb, ob = (keep(torch.zeros(n, dtype=t, device="cuda")) for n, t in ((6 * 8 * 16, dtype), (9 * 16, F32), (6 * 8 * 16, dtype)))
    assert status("uf_dwconv3x3_fwd", xb.data_ptr(), wb.data_ptr(), None, ob.data_ptr(), 1, 6, 8, 16, 0, dt(dtype), st()) == X.UF_ERR_SHAPE       # H must be a multiple of 4


# ---------------------------------------------------------------------------------------------------------------------------
# UNet implicit GEMMs
# ---------------------------------------------------------------------------------------------------------------------------
def conv3(x64, wp, bias, aux64, out, B, H, W, cin, cout, epi, acc, dtype):
    x = Strided(B * H * W, cin, pad=4, data=X.to_rows(x64))
    aux = None if aux64 is None else Strided(B * H * W, cout, pad=8, data=X.to_rows(aux64))
    call("uf_conv3x3_fwd", x.ptr(), x.ld, wp.data_ptr(), None if bias is None else bias.data_ptr(), None if aux is None else aux.ptr(), 0 if aux is None else aux.ld,
         out.ptr(), out.ld, B, H, W, cin, cout, epi, acc, dt(dtype), st())
    assert out.intact() and x.intact() and (aux is None or aux.intact())
    return out.live()


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("cin,cout,H,W,B", X.conv3_cases())
def test_conv3x3_every_epilogue(dtype, cin, cout, H, W, B):
    """bias; LeakyReLU; LeakyReLU + aux rows; dgrad with its aux mask -- each with accumulate 0 and 1, into a destination at a column offset"""
    from uformer_amd import packing
    c = X.conv_case(3, B, H, W, cin, cout)
    tag = f"{TAG[dtype]}/{cin}to{cout}/B{B}H{H}W{W}"
    M = B * H * W
    wp, bias = packing.pack_conv(dev(c["w"]), dtype), dev(c["bias"])
    refs = {(0, 0): c["pre"], (0, 1): c["pre_acc"], (1, 0): c["lrelu"], (1, 1): c["lrelu_acc"], (2, 0): c["lrelu_aux"], (2, 1): c["lrelu_aux_acc"]}
    for (epi, acc), ref in refs.items():
        out = Strided(M, cout, pad=8, off=cout, data=c["prev"].permute(0, 2, 3, 1) if acc else None)
        got = conv3(c["x"], wp, bias, c["aux"] if epi == 2 else None, out, B, H, W, cin, cout, epi, acc, dtype)
        assert_exact(f"uf_conv3x3_fwd/{tag}/epi{epi}acc{acc}", got, X.to_rows(ref), F32, tile=(128, 64))
    wt = packing.pack_conv_dgrad(dev(c["w"]), dtype)             # the input gradient of the same conv: cout -> cin
    for acc, ref in ((0, c["dgrad"]), (1, c["dgrad_acc"])):
        out = Strided(M, cin, pad=8, off=8, data=c["prev_in"].permute(0, 2, 3, 1) if acc else None)
        got = conv3(c["dy"], wt, None, c["a"], out, B, H, W, cout, cin, 3, acc, dtype)
        assert_exact(f"uf_conv3x3_fwd/{tag}/epi3acc{acc}", got, X.to_rows(ref), F32, tile=(128, 64))


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("cin,cout", X.CONV_PAIRS)
def test_conv4s2_conv1x1(dtype, cin, cout):
    from uformer_amd import packing
    for (k, H, W, B) in X.conv41_cases(cin, cout):
        fn = "uf_conv4s2_fwd" if k == 4 else "uf_conv1x1_fwd"
        c = X.conv_case(k, B, H, W, cin, cout)
        Ho, Wo = (H // 2, W // 2) if k == 4 else (H, W)
        x = Strided(B * H * W, cin, pad=4, data=X.to_rows(c["x"]))
        out = Strided(B * Ho * Wo, cout, pad=16, off=4)
        call(fn, x.ptr(), x.ld, keep(packing.pack_conv(dev(c["w"]), dtype)).data_ptr(), dev(c["bias"]).data_ptr(), out.ptr(), out.ld, B, H, W, cin, cout, dt(dtype), st())
        assert out.intact() and x.intact()
        assert_exact(f"{fn}/{TAG[dtype]}/{cin}to{cout}/B{B}H{H}W{W}", out.live(), X.to_rows(c["out"]), F32)
    buf = torch.zeros(4096, device="cuda")
    assert status("uf_conv4s2_fwd", buf.data_ptr(), 4, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 4, 1, 5, 6, 4, 4, dt(dtype), st()) == X.UF_ERR_SHAPE     # odd H
    assert status("uf_conv1x1_fwd", buf.data_ptr(), 6, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 4, 1, 4, 4, 6, 4, dt(dtype), st()) == X.UF_ERR_SHAPE     # Cin % 4
    assert status("uf_conv1x1_fwd", buf.data_ptr() + 4, 4, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 4, 1, 4, 4, 4, 4, dt(dtype), st()) == X.UF_ERR_ALIGN


@pytest.mark.parametrize("cout", [16, 32, 96])
@pytest.mark.parametrize("B", X.CONV_B)
def test_conv1x1_nchw(B, cout):
    H, W = X.CONV1_MAP
    img, w, b = X.lattice((B, 3, H, W), PM2, 49, k=2), X.lattice((cout, 3), PM2, 50 + cout), X.lattice((cout,), PM1, 51)
    X.check_accumulation(3, PM2, PM2, addend_steps=4)
    out = Strided(B * H * W, cout, off=4)
    call("uf_conv1x1_nchw_fwd", dev(img).data_ptr(), dev(w).data_ptr(), dev(b).data_ptr(), out.ptr(), out.ld, B, 3, H, W, cout, st())
    assert out.intact()
    assert_exact(f"uf_conv1x1_nchw_fwd/f32/B{B}C{cout}", out.live(), X.to_rows(torch.nn.functional.conv2d(img, w[:, :, None, None], b)), F32)
    assert status("uf_conv1x1_nchw_fwd", out.ptr(), out.ptr(), out.ptr(), out.ptr(), out.ld, B, 5, H, W, cout, st()) == X.UF_ERR_SHAPE                        # Cin <= 4


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("k,stride,pad,nchw,B,H,W,C", X.IM2COL_CASES)
def test_im2col_col2im(dtype, k, stride, pad, nchw, B, H, W, C):
    """the patch matrix of a lattice map; col2im of a lattice patch matrix (with and without accumulate) and of an all-ones one (the tap-count map)"""
    tag = f"{TAG[dtype]}/k{k}s{stride}p{pad}nchw{nchw}/B{B}H{H}W{W}C{C}"
    x64 = X.lattice((B, C, H, W), PM2, 55 + C)
    ref = X.ref_im2col(x64, k, stride, pad)
    Mo, KK = ref.shape
    ldc = (KK + 7) // 8 * 8 + 8
    cols = torch.full((Mo + 2, ldc), SENTINEL, dtype=dtype, device="cuda")
    if nchw:
        x, xp, ldx = dev(x64), None, C
    else:
        xp = Strided(B * H * W, C, pad=4, data=X.to_rows(x64))
    call("uf_im2col", x.data_ptr() if nchw else xp.ptr(), ldx if nchw else xp.ld, cols.data_ptr(), ldc, B, H, W, C, k, stride, pad, nchw, dt(dtype), st())
    s = torch.full((), SENTINEL, dtype=dtype, device="cuda")
    assert bool((cols[Mo:] == s).all()) and (xp is None or xp.intact())
    assert_exact(f"uf_im2col/{tag}", cols[:Mo, :KK], ref, dtype)
    assert bool((cols[:Mo, KK:] == 0).all()), "the padding columns of the patch matrix are zero by contract"
    if dtype in HALF:                                            # values T cannot hold: the cast rounds to nearest even
        xr = X.lattice((B, C, H, W), X.cast_rounding_values(dtype), 56)
        src = dev(xr) if nchw else dev(X.to_rows(xr))
        c2 = torch.zeros(Mo, ldc, dtype=dtype, device="cuda")
        call("uf_im2col", src.data_ptr(), C, c2.data_ptr(), ldc, B, H, W, C, k, stride, pad, nchw, dt(dtype), st())
        assert_exact(f"uf_im2col/{tag}/rounding", c2[:, :KK], X.ref_im2col(xr, k, stride, pad), dtype)
    for name, d64 in (("lattice", X.lattice((Mo, KK), PM2, 57 + KK)), ("ones", torch.ones(Mo, KK, dtype=torch.float64))):
        dc = torch.full((Mo, ldc), SENTINEL, dtype=dtype, device="cuda")
        dc[:, :KK] = dev(d64, dtype)
        want = X.ref_col2im(d64, B, H, W, C, k, stride, pad)
        base = X.lattice((B, C, H, W), PM2, 58)
        for acc in (0, 1):
            if nchw:
                dx = flat_guarded(B * C * H * W)
                if acc:
                    dx[:B * C * H * W] = dev(base).reshape(-1)
                call("uf_col2im", dc.data_ptr(), ldc, dx.data_ptr(), C, B, H, W, C, k, stride, pad, 1, acc, dt(dtype), st())
                assert tail_intact(dx, B * C * H * W)
                got, r = dx[:B * C * H * W].reshape(B, C, H, W), want + (base if acc else 0)
            else:
                dxs = Strided(B * H * W, C, pad=4, off=4, data=X.to_rows(base) if acc else None)
                call("uf_col2im", dc.data_ptr(), ldc, dxs.ptr(), dxs.ld, B, H, W, C, k, stride, pad, 0, acc, dt(dtype), st())
                assert dxs.intact()
                got, r = dxs.live(), X.to_rows(want + (base if acc else 0))
            assert_exact(f"uf_col2im/{tag}/{name}/acc{acc}", got, r, F32)


# ---------------------------------------------------------------------------------------------------------------------------
# backward contractions and reductions (each also bit-identical when run twice)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("M,N,K", X.WGRAD_CASES)
def test_linear_wgrad(dtype, M, N, K):
    c = X.wgrad_case(M, N, K)
    dy, x = Strided(M, N, dtype, pad=8, data=c["dy"]), Strided(M, K, dtype, pad=16, off=8, data=c["x"])
    nb = max(16, L().uf_linear_wgrad_workspace_bytes(M, N, K))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    for with_bias in (1, 0):
        def run():
            dW, db = flat_guarded(N * K), flat_guarded(N)
            call("uf_linear_wgrad", dy.ptr(), dy.ld, x.ptr(), x.ld, dW.data_ptr(), db.data_ptr() if with_bias else None, M, N, K, dt(dtype), ws.data_ptr(), nb, st())
            assert tail_intact(dW, N * K) and tail_intact(db, N if with_bias else 0) and dy.intact() and x.intact()
            return dW[:N * K].reshape(N, K), db[:N]
        dW, db = twice(run)
        assert_exact(f"uf_linear_wgrad/{TAG[dtype]}/M{M}N{N}K{K}/bias{with_bias}/dW", dW, c["dW"], F32, tile=(64, 64))
        if with_bias:
            assert_exact(f"uf_linear_wgrad/{TAG[dtype]}/M{M}N{N}K{K}/bias{with_bias}/db", db, c["db"], F32)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("M,N", X.ROWS_SUM_CASES)
def test_rows_sum(dtype, M, N):
    x64 = X.lattice((M, N), PM2, 59 + M)
    X.check_accumulation(M, PM2)
    x = Strided(M, N, dtype, pad=8, data=x64)
    nb = max(16, L().uf_rows_sum_workspace_bytes(M, N))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

    def run():
        out = flat_guarded(N)
        call("uf_rows_sum", x.ptr(), x.ld, out.data_ptr(), M, N, dt(dtype), ws.data_ptr(), nb, st())
        assert tail_intact(out, N) and x.intact()
        return [out[:N]]
    assert_exact(f"uf_rows_sum/{TAG[dtype]}/M{M}N{N}", twice(run)[0], x64.sum(0), F32)
    assert status("uf_rows_sum", x.ptr(), x.ld + 1, ws.data_ptr(), M, N, dt(dtype), ws.data_ptr(), nb, st()) == X.UF_ERR_SHAPE


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C", X.DWCONV_CASES)
def test_dwconv3x3_wgrad(dtype, B, H, W, C):
    c = X.dwconv_case(B, H, W, C)
    h, dc = dev(X.to_rows(c["x"]), dtype), dev(X.to_rows(c["dc"]), dtype)
    nb = max(16, L().uf_dwconv3x3_wgrad_workspace_bytes(C, dt(dtype)))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

    def run():
        dw, db = flat_guarded(9 * C), flat_guarded(C)
        call("uf_dwconv3x3_wgrad", h.data_ptr(), dc.data_ptr(), dw.data_ptr(), db.data_ptr(), B, H, W, C, dt(dtype), ws.data_ptr(), nb, st())
        assert tail_intact(dw, 9 * C) and tail_intact(db, C)
        return dw[:9 * C].reshape(9, C), db[:C]
    dw, db = twice(run)
    assert_exact(f"uf_dwconv3x3_wgrad/{TAG[dtype]}/B{B}H{H}W{W}C{C}/dw9", dw, c["dw9"], F32)
    assert_exact(f"uf_dwconv3x3_wgrad/{TAG[dtype]}/B{B}H{H}W{W}C{C}/dbias", db, c["dbias"], F32)


@pytest.mark.parametrize("nchw,B,H,W,cin,cout,masked", X.CONV3_BWD_CASES)
def test_conv3x3_bwd(nchw, B, H, W, cin, cout, masked):
    """the stem / head backward (all f32), token-row and NCHW forms, with and without the activation mask (slope 1/2: exact, see exact_lattice)"""
    c = X.conv3_bwd_case(nchw, B, H, W, cin, cout, masked)
    x = dev(c["x"]) if nchw else dev(X.to_rows(c["x"]))
    dy, w = dev(X.to_rows(c["dy"])), dev(c["w"])
    act = dev(X.to_rows(c["act"])) if masked else None
    nb = max(16, L().uf_conv3x3_bwd_workspace_bytes(B, H, W, cin, cout))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    n = B * cin * H * W

    def run():
        dx, dW, db = flat_guarded(n), flat_guarded(cout * cin * 9), flat_guarded(cout)
        call("uf_conv3x3_bwd", x.data_ptr(), nchw, dy.data_ptr(), None if act is None else act.data_ptr(), X.CONV3_BWD_SLOPE, w.data_ptr(), dx.data_ptr(), dW.data_ptr(),
             db.data_ptr(), B, H, W, cin, cout, ws.data_ptr(), nb, st())
        assert tail_intact(dx, n) and tail_intact(dW, cout * cin * 9) and tail_intact(db, cout)
        return dx[:n], dW[:cout * cin * 9].reshape(cout, cin, 3, 3), db[:cout]
    dx, dW, db = twice(run)
    tag = f"f32/nchw{nchw}/B{B}H{H}W{W}/{cin}to{cout}/mask{masked}"
    assert_exact(f"uf_conv3x3_bwd/{tag}/dx", dx.reshape(B, cin, H, W) if nchw else dx.reshape(B * H * W, cin), c["dx"] if nchw else X.to_rows(c["dx"]), F32)
    assert_exact(f"uf_conv3x3_bwd/{tag}/dW", dW, c["dW"], F32)
    assert_exact(f"uf_conv3x3_bwd/{tag}/db", db, c["db"], F32)
    if not nchw:                                                 # the mask is folded on the NCHW (InputProj) form only
        assert status("uf_conv3x3_bwd", x.data_ptr(), 0, dy.data_ptr(), dy.data_ptr(), 0.5, w.data_ptr(), None, ws.data_ptr(), ws.data_ptr(), B, H, W, cin, cout,
                      ws.data_ptr(), nb, st()) == X.UF_ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,cin", X.DOWN_BWD_CASES)
def test_downsample_bwd(dtype, B, H, W, cin):
    from uformer_amd import packing
    c = X.down_bwd_case(B, H, W, cin)
    X.check_representable(c["taps"], dtype)
    cout, M, Mo = 2 * cin, B * H * W, B * (H // 2) * (W // 2)
    x = Strided(M, cin, pad=4, data=X.to_rows(c["x"]))
    dy = dev(X.to_rows(c["dy"]))
    wpt = packing.pack_downsample(dev(c["w"]), dtype).t().contiguous()
    nb = L().uf_downsample_bwd_workspace_bytes(B, H, W, cin, cout, dt(dtype))
    ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) // 256 * 256
    for acc in (0, 1):
        def run():
            dx = Strided(M, cin, pad=4, off=4, data=X.to_rows(c["base"]) if acc else None)
            dW, db = flat_guarded(cout * 16 * cin), flat_guarded(cout)
            call("uf_downsample_bwd", x.ptr(), x.ld, dy.data_ptr(), wpt.data_ptr(), dx.ptr(), dx.ld, acc, dW.data_ptr(), db.data_ptr(), B, H, W, cin, cout, dt(dtype), wp, nb, st())
            assert dx.intact() and x.intact() and tail_intact(dW, cout * 16 * cin) and tail_intact(db, cout)
            return dx.live().contiguous(), dW[:cout * 16 * cin].reshape(cout, 16 * cin), db[:cout]
        dx, dW, db = twice(run)
        tag = f"{TAG[dtype]}/B{B}H{H}W{W}C{cin}/add{acc}"
        assert_exact(f"uf_downsample_bwd/{tag}/dx", dx, X.to_rows(c["dx"] + (c["base"] if acc else 0)), F32)
        assert_exact(f"uf_downsample_bwd/{tag}/dW", dW, c["dW"].permute(0, 2, 3, 1).reshape(cout, -1), F32)
        assert_exact(f"uf_downsample_bwd/{tag}/db", db, c["db"], F32)
    if dtype in HALF and (B, H, W, cin) == X.DOWN_BWD_CASES[0]:
        # the layer input is cast to T on its way into the patch matrix (uf_im2col inside): values T cannot hold must round to nearest even there, and the weight
        # gradient is then the exact contraction of the ROUNDED patches (at most Mo x (2^p + 4) steps: condition 1)
        xr = X.lattice((B, cin, H, W), X.cast_rounding_values(dtype), 75)
        prof = X.rounding_profile(xr, dtype)
        assert prof["away"] > 0 and prof["ties"] > 0
        X.check_accumulation(Mo, X.cast_rounding_values(dtype), PM1, addend_steps=Mo)
        xs = Strided(M, cin, pad=4, data=X.to_rows(xr))
        dx = Strided(M, cin, pad=4, off=4)
        dW, db = flat_guarded(cout * 16 * cin), flat_guarded(cout)
        call("uf_downsample_bwd", xs.ptr(), xs.ld, dy.data_ptr(), wpt.data_ptr(), dx.ptr(), dx.ld, 0, dW.data_ptr(), db.data_ptr(), B, H, W, cin, cout, dt(dtype), wp, nb, st())
        assert dx.intact() and xs.intact() and tail_intact(dW, cout * 16 * cin)
        assert_exact(f"uf_downsample_bwd/{TAG[dtype]}/B{B}H{H}W{W}C{cin}/rounding/dW", dW[:cout * 16 * cin].reshape(cout, 16 * cin),
                     X.to_rows(c["dy"]).t() @ X.ref_im2col(xr.to(dtype).double(), 4, 2, 1), F32)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,cin,cout", X.UP_BWD_CASES)
def test_upsample_cat_bwd(dtype, B, H, W, cin, cout):
    from uformer_amd import packing
    c = X.up_bwd_case(B, H, W, cin, cout)
    X.check_representable(c["dx"], dtype)
    M = B * H * W
    d = Strided(4 * M, cout, pad=cout, data=X.to_rows(c["d"]))   # the left half of a 2 Cout-wide concat gradient; the skip half holds the sentinel
    x = dev(X.to_rows(c["x"]))
    wpt = packing.pack_upsample(dev(c["w"]), dtype).t().contiguous()
    nb = L().uf_upsample_cat_bwd_workspace_bytes(B, H, W, cin, cout, dt(dtype))
    ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) // 256 * 256

    def run():
        dx, dW, db = flat_guarded(M * cin), flat_guarded(4 * cout * cin), flat_guarded(cout)
        call("uf_upsample_cat_bwd", d.ptr(), d.ld, x.data_ptr(), cin, wpt.data_ptr(), dx.data_ptr(), dW.data_ptr(), db.data_ptr(), B, H, W, cin, cout, dt(dtype), wp, nb, st())
        assert d.intact() and tail_intact(dx, M * cin) and tail_intact(dW, 4 * cout * cin) and tail_intact(db, cout)
        return dx[:M * cin].reshape(M, cin), dW[:4 * cout * cin].reshape(4 * cout, cin), db[:cout]
    dx, dW, db = twice(run)
    tag = f"{TAG[dtype]}/B{B}H{H}W{W}/{cin}to{cout}"
    assert_exact(f"uf_upsample_cat_bwd/{tag}/dx", dx, X.to_rows(c["dx"]), F32)
    assert_exact(f"uf_upsample_cat_bwd/{tag}/dW", dW, c["dW"].permute(2, 3, 1, 0).reshape(4 * cout, cin), F32)
    assert_exact(f"uf_upsample_cat_bwd/{tag}/db", db, c["db"], F32)
    assert status("uf_upsample_cat_bwd", d.ptr(), d.ld, x.data_ptr(), cin + 8, wpt.data_ptr(), dx.data_ptr(), dW.data_ptr(), db.data_ptr(), B, H, W, cin, cout, dt(dtype), wp, nb,
                  st()) == X.UF_ERR_SHAPE                        # x rows must be dense


@pytest.mark.parametrize("heads", X.RPB_HEADS)
def test_rpb_table_grad(heads):
    """against an index-sum through the relative-position index of an 8 x 8 window"""
    db64 = X.lattice((heads, 64, 64), PM2, 65 + heads)
    ref = torch.zeros(225, heads, dtype=torch.float64).index_add_(0, X.rpb_index(8).reshape(-1), db64.permute(1, 2, 0).reshape(4096, heads))
    db = dev(db64)

    def run():
        out = flat_guarded(225 * heads)
        call("uf_rpb_table_grad", db.data_ptr(), out.data_ptr(), heads, st())
        assert tail_intact(out, 225 * heads)
        return [out[:225 * heads].reshape(225, heads)]
    assert_exact(f"uf_rpb_table_grad/f32/h{heads}", twice(run)[0], ref, F32)


@pytest.mark.parametrize("nwin,heads", X.RPB4_CASES)
def test_rpb4_table_grad(nwin, heads):
    ds64 = X.lattice((nwin, heads, 16, 16), PM2, 66 + nwin)
    X.check_accumulation(16 * nwin, PM2)
    ref = torch.zeros(49, heads, dtype=torch.float64).index_add_(0, X.rpb_index(4).reshape(-1), ds64.sum(0).permute(1, 2, 0).reshape(256, heads))
    ds = dev(ds64)

    def run():
        out = flat_guarded(49 * heads)
        call("uf_rpb4_table_grad", ds.data_ptr(), out.data_ptr(), nwin, heads, st())
        assert tail_intact(out, 49 * heads)
        return [out[:49 * heads].reshape(49, heads)]
    assert_exact(f"uf_rpb4_table_grad/f32/w{nwin}h{heads}", twice(run)[0], ref, F32)
    assert status("uf_rpb4_table_grad", ds.data_ptr(), ds.data_ptr(), 0, heads, st()) == X.UF_ERR_SHAPE


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C,windowed,shift", X.STREAM_CASES)
def test_residual_combine_and_grad_fork(dtype, B, H, W, C, windowed, shift):
    M = B * H * W
    tag = f"{TAG[dtype]}/B{B}H{H}W{W}C{C}/win{windowed}s{shift}"
    tok = X.window_tokens(B, H, W, shift) if windowed else torch.arange(M)
    scale = torch.tensor([X.SCALES[(i + 1) % 4] for i in range(B)], dtype=torch.float64)
    a64, b64, g2 = X.lattice((M, C), PM2, 67), X.lattice((M, C), PM2, 68), X.lattice((M, C), PM2, 69)
    for sc in (None, scale):
        s_tok = torch.ones(M, dtype=torch.float64) if sc is None else sc[tok // (H * W)]
        sp = None if sc is None else dev(sc).data_ptr()
        for with_a in (1, 0):
            for b_f32 in ((0, 1) if dtype != F32 else (1,)):
                def run():
                    out = flat_guarded(M * C)
                    call("uf_residual_combine", dev(a64).data_ptr() if with_a else None, dev(b64, F32 if b_f32 else dtype).data_ptr(), b_f32, out.data_ptr(), sp, B, H, W, C,
                         windowed, shift, dt(dtype), st())
                    assert tail_intact(out, M * C)
                    return [out[:M * C].reshape(M, C)]
                ref = torch.zeros(M, C, dtype=torch.float64)
                ref[tok] = (a64[tok] if with_a else 0) + s_tok[:, None] * b64
                assert_exact(f"uf_residual_combine/{tag}/scale{int(sc is not None)}a{with_a}f32b{b_f32}", twice(run)[0], ref, F32, tile=(64, C))
        for with_g2 in (1, 0):
            def run():
                so, co = flat_guarded(M * C), flat_guarded(M * C, dtype)
                call("uf_grad_fork", dev(a64).data_ptr(), dev(g2).data_ptr() if with_g2 else None, so.data_ptr(), co.data_ptr(), sp, B, H, W, C, windowed, shift, dt(dtype), st())
                assert tail_intact(so, M * C) and tail_intact(co, M * C)
                return so[:M * C].reshape(M, C), co[:M * C].reshape(M, C)
            so, co = twice(run)
            t = a64 + (g2 if with_g2 else 0)
            assert_exact(f"uf_grad_fork/{tag}/scale{int(sc is not None)}g2{with_g2}/sum", so, t, F32, tile=(64, C))
            assert_exact(f"uf_grad_fork/{tag}/scale{int(sc is not None)}g2{with_g2}/cast", co, t[tok] * s_tok[:, None], dtype, tile=(64, C))
    if dtype in HALF:                                            # the cast rounds to nearest even: 2^p + 1, 2^p + 3, ... under scales 1/2, 1, 2
        p = X.OUT_STEPS[dtype]
        g1, g2r = X.lattice((M, C), (-p, p), 70), X.lattice((M, C), (-5, -3, -1, 1, 3, 5), 71)
        co = flat_guarded(M * C, dtype)
        call("uf_grad_fork", dev(g1).data_ptr(), dev(g2r).data_ptr(), None, co.data_ptr(), dev(scale).data_ptr(), B, H, W, C, windowed, shift, dt(dtype), st())
        ref = (g1 + g2r)[tok] * scale[tok // (H * W)][:, None]
        assert X.rounding_profile(ref, dtype)["away"] > 0
        assert_exact(f"uf_grad_fork/{tag}/rounding", co[:M * C].reshape(M, C), ref, dtype, tile=(64, C))
    if not windowed and H % 8:
        buf = torch.zeros(M * C, device="cuda")
        assert status("uf_residual_combine", None, buf.data_ptr(), 1, buf.data_ptr(), None, B, H, W, C, 1, 4, dt(dtype), st()) == X.UF_ERR_SHAPE
        assert status("uf_grad_fork", buf.data_ptr(), None, None, buf.data_ptr(), None, B, H, W, C, 1, 4, dt(dtype), st()) == X.UF_ERR_SHAPE


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("nwin,heads", X.MERGE_CASES)
def test_qkv_grad_merge(dtype, nwin, heads):
    """the head merge; the query third is multiplied by float32(32 ** -0.5) in float32 and then stored as T"""
    C, M = 32 * heads, 64 * nwin
    dq, dk, dvt = X.lattice((nwin, heads, 64, 32), PM2, 72), X.lattice((nwin, heads, 64, 32), PM2, 73), X.lattice((nwin, heads, 32, 64), PM2, 74)
    qs = torch.tensor(32.0 ** -0.5, dtype=torch.float32)
    ref = torch.cat([(dq.float() * qs).permute(0, 2, 1, 3).reshape(M, C).double(), dk.permute(0, 2, 1, 3).reshape(M, C), dvt.permute(0, 3, 1, 2).reshape(M, C)], 1)

    def run():
        out = flat_guarded(M * 3 * C, dtype)
        call("uf_qkv_grad_merge", dev(dq, dtype).data_ptr(), dev(dk, dtype).data_ptr(), dev(dvt, dtype).data_ptr(), out.data_ptr(), nwin, heads, 32, dt(dtype), st())
        assert tail_intact(out, M * 3 * C)
        return [out[:M * 3 * C].reshape(M, 3 * C)]
    assert_exact(f"uf_qkv_grad_merge/{TAG[dtype]}/w{nwin}h{heads}", twice(run)[0], ref, dtype, tile=(64, C))
    buf = torch.zeros(64, dtype=dtype, device="cuda")
    for hd in (16, 64):
        assert status("uf_qkv_grad_merge", buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 1, hd, dt(dtype), st()) == X.UF_ERR_SHAPE


def test_report_lists_every_entry_point(request):
    """nothing compared differs, and once every test function of this file has run in this process, every listed entry point has been compared.  The
    same check runs again when the module's fixture is torn down (_dump_report), so it does not rest on this test being the last one to run."""
    check_report(request, exclude=request.node.name)
