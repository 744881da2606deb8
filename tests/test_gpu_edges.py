"""Edge tests through the C ABI (include/uformer_hip.h), helpers in tests/edge_cases.py.

Part A, memory discipline (bit-exact, no tolerances): every entry point that takes a leading dimension is called on strided views
inside allocations whose every other element is one NaN bit pattern, and on contiguous buffers.  The live output must be
bit-identical, every poisoned element outside an output view must still hold the pattern, and no NaN may reach the live output.
Workspaces are filled with 0x00 and with 0xFF bytes (NaN in all three types): same bits out, guard bytes behind them untouched.

Part B, hard inputs gated row by row against float64: kernel worst row <= 4 x the worst row of the CPU emulation of the kernel's
arithmetic (floor 2 ulp of the output type); ratios go to $UF_REPORT_DIR/parity_edges.json.
"""
import ctypes
import json
import os

import pytest
import torch

import edge_cases as E
from edge_cases import BF16, F16, F32, PoisonedView

pytestmark = pytest.mark.gpu

HALF = [BF16, F16]
MODES = [F32, BF16, F16]
MAPS = [(8, 8), (16, 16), (8, 24)]
B = 2
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_report():
    """the measured kernel / emulation figures go to $UF_REPORT_DIR/parity_edges.json when that variable names a directory"""
    yield
    out = os.environ.get("UF_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_edges.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def lib():
    from uformer_amd import _lib
    return _lib.load()


def call(name, *args):
    from uformer_amd import _lib
    _lib.check(getattr(lib(), name)(*args), name)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dt_of(dtype):
    from uformer_amd import ops
    return ops.uf_dtype(dtype)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def pv(edge, rows, C, dtype, mode, data=None, **kw):
    """a PoisonedView on the GPU: ``mode`` when ``edge``, else the contiguous buffer of the comparison call"""
    p = PoisonedView(rows, C, dtype, mode if edge else "plain", "cuda", **(kw if edge else {}))
    return p if data is None else p.fill(data.cuda())


def both(run):
    """run(edge) -> (outputs {name: PoisonedView}, inputs [PoisonedView]).  The three assertions of Part A."""
    ref, _ = run(False)
    got, ins = run(True)
    torch.cuda.synchronize()
    for name, g in got.items():
        assert g.G > 0 or g.ld > g.C, f"{name}: the edge call must have something to protect"
        assert torch.equal(g.live_bits(), ref[name].live_bits()), f"{name}: strided / poisoned call differs from the contiguous call"
        assert g.guard_intact(), f"{name}: wrote outside its view"
        assert not torch.isnan(g.live().float()).any(), f"{name}: a poisoned value reached the result"
    for i, p in enumerate(ins):
        assert p.guard_intact(), f"input {i}: its allocation was written"


def ws_bytes_pair(nbytes):
    """the two workspaces of the poisoning runs: (buffer, guard) filled with 0x00 and with 0xFF"""
    return [E.poisoned_bytes(int(nbytes), 4096, fill, "cuda") for fill in (0x00, 0xFF)]


def guard_ok(guard):
    return bool((guard == 0xA5).all())


def block_module(C, H, W, heads, shift, win=8, modulator=True, seed=0):
    from uformer_amd import model
    torch.manual_seed(seed + C + shift)
    blk = model.LeWinTransformerBlock(C, (H, W), heads, win_size=win, shift_size=shift, modulator=modulator)
    with torch.no_grad():
        for n, p in blk.named_parameters():                      # biases and tables away from their zero initial values
            if p.dim() == 1 or "table" in n:
                p.add_(0.1 * torch.randn(p.shape))
    return blk.cuda().eval()


# ---------------------------------------------------------------------------------------------------------------------------
# Part A: forward entry points
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("windowed,shift", [(0, 0), (1, 4)])
def test_layernorm_fwd_strided(dtype, H, W, windowed, shift):
    C, M = 32, B * H * W
    x = torch.randn(M, C, generator=gen(1)) * 2 + 0.5
    gm, bt = (t.cuda() for t in E.ln_affine(C))
    mod = torch.randn(64, C, generator=gen(2)).cuda() if windowed else None

    def run(edge):
        xi, out = pv(edge, M, C, F32, "cat", x), pv(edge, M, C, dtype, "guard")
        call("uf_layernorm_fwd", xi.ptr(), xi.ld, gm.data_ptr(), bt.data_ptr(), None if mod is None else mod.data_ptr(), out.ptr(), B, H, W, C,
             windowed, shift, dt_of(dtype), stream())
        return {"out": out}, [xi]
    both(run)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W,shift", [(8, 8, 0), (16, 16, 4), (8, 24, 4)])
@pytest.mark.parametrize("C,heads", [(32, 1), (64, 1), (256, 8)])
def test_ln_fused_projections_strided(dtype, H, W, shift, C, heads):
    from uformer_amd import ops
    M = B * H * W
    x = torch.randn(M, C, generator=gen(3)) * 1.5 + 0.3
    gm, bt = (t.cuda() for t in E.ln_affine(C))
    mod = (0.5 * torch.randn(64, C, generator=gen(4))).cuda()
    wq, bq = E.gemm_weights(3 * C, C, dtype, 5)
    w1, b1 = E.gemm_weights(4 * C, C, dtype, 6)
    wq_fm, w1_fm, bq, b1 = ops.pack_weight_fm(wq.cuda()), ops.pack_weight_fm(w1.cuda()), bq.cuda(), b1.cuda()

    def run_qkv(edge):
        xi = pv(edge, M, C, F32, "cat", x)
        q, k, vt = (pv(edge, M, C, dtype, "guard") for _ in range(3))
        call("uf_ln_qkv_fwd", xi.ptr(), xi.ld, gm.data_ptr(), bt.data_ptr(), mod.data_ptr(), wq_fm.data_ptr(), bq.data_ptr(), q.ptr(), k.ptr(), vt.ptr(),
             B, H, W, C, heads, shift, dt_of(dtype), stream())
        return {"q": q, "k": k, "vt": vt}, [xi]

    def run_l1(edge):
        xi, out = pv(edge, M, C, F32, "cat", x), pv(edge, M, 4 * C, dtype, "guard")
        call("uf_ln_linear_gelu_fwd", xi.ptr(), xi.ld, gm.data_ptr(), bt.data_ptr(), w1_fm.data_ptr(), b1.data_ptr(), out.ptr(), M, 4 * C, C, dt_of(dtype), stream())
        return {"h1": out}, [xi]
    both(run_qkv)
    both(run_l1)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C", [32, 128])
def test_dwconv_linear2_strided(dtype, H, W, C):
    from uformer_amd import ops
    M, hid = B * H * W, 4 * C
    h1 = torch.randn(M, hid, generator=gen(7))
    x = torch.randn(M, C, generator=gen(8))
    w9, bdw = (torch.randn(9, hid, generator=gen(9)) / 3).cuda(), (0.1 * torch.randn(hid, generator=gen(10))).cuda()
    w2, b2 = E.gemm_weights(C, hid, dtype, 11)
    w2_fm, b2 = ops.pack_weight_fm(w2.cuda()), b2.cuda()

    def run(edge):
        hi, xi = pv(edge, M, hid, dtype, "guard", h1), pv(edge, M, C, F32, "cat", x)
        call("uf_dwconv_linear2_fwd", hi.ptr(), w9.data_ptr(), bdw.data_ptr(), w2_fm.data_ptr(), b2.data_ptr(), xi.ptr(), xi.ld, B, H, W, C, dt_of(dtype), stream())
        return {"x": xi}, [hi]
    both(run)


@pytest.mark.parametrize("H,W", [(8, 8), (16, 16), (8, 24), (13, 70)])
def test_stem_and_head_strided(H, W):
    from uformer_amd import packing
    E_, M = 32, B * H * W
    img = torch.rand(B, 3, H, W, generator=gen(12))
    w27 = packing.pack_input_proj(torch.randn(E_, 3, 3, 3, generator=gen(13)) * 0.2).cuda()
    bias = (0.1 * torch.randn(E_, generator=gen(14))).cuda()
    xo = torch.randn(M, 2 * E_, generator=gen(15))
    wo = packing.pack_output_proj(torch.randn(3, 2 * E_, 3, 3, generator=gen(16)) * 0.1).cuda()
    bo = (0.1 * torch.randn(3, generator=gen(17))).cuda()

    def run_in(edge):
        im, out = pv(edge, B * 3 * H, W, F32, "guard", img), pv(edge, M, E_, F32, "cat")
        call("uf_input_proj_fwd", im.ptr(), w27.data_ptr(), bias.data_ptr(), out.ptr(), out.ld, B, 3, H, W, E_, stream())
        return {"tokens": out}, [im]

    def run_out(edge):
        xi, im, out = pv(edge, M, 2 * E_, F32, "strided", xo), pv(edge, B * 3 * H, W, F32, "guard", img), pv(edge, B * 3 * H, W, F32, "guard")
        call("uf_output_proj_fwd", xi.ptr(), xi.ld, wo.data_ptr(), bo.data_ptr(), im.ptr(), out.ptr(), B, H, W, 2 * E_, 1, stream())
        return {"image": out}, [xi, im]
    both(run_in)
    both(run_out)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W", [(4, 4), (8, 8), (4, 12)])
@pytest.mark.parametrize("Cin,Cout", [(64, 32), (512, 256)])
def test_upsample_fwd_into_left_half_of_concat_buffer(dtype, H, W, Cin, Cout):
    """the model's exact use: output into columns [0, Cout) of a 2 Cout-wide buffer whose right half (the skip) is poisoned"""
    from uformer_amd import packing
    M = B * H * W
    x = torch.randn(M, Cin, generator=gen(18))
    w = packing.pack_upsample(torch.randn(Cin, Cout, 2, 2, generator=gen(19)) / Cin ** 0.5, dtype).cuda()
    bias = (0.1 * torch.randn(Cout, generator=gen(20))).cuda()

    def run(edge):
        xi, out = pv(edge, M, Cin, F32, "strided", x), pv(edge, 4 * M, Cout, F32, "cat_left")
        call("uf_upsample_fwd", xi.ptr(), xi.ld, w.data_ptr(), bias.data_ptr(), out.ptr(), out.ld, B, H, W, Cin, Cout, dt_of(dtype), stream())
        return {"up": out}, [xi]
    both(run)


# ---------------------------------------------------------------------------------------------------------------------------
# Part A: blocks in place at ld = 2C on the right half of a concat buffer, workspace poisoned both ways
# ---------------------------------------------------------------------------------------------------------------------------
def _block_runs(entry, bp, x, H, W, C, dtype, extra=()):
    M = B * H * W
    nbytes = lib().uf_block_workspace_bytes(M, C, dt_of(dtype))
    wss = ws_bytes_pair(nbytes)

    def make(flip):
        def run(edge):
            xi = pv(edge, M, C, F32, "cat", x)
            which = int(edge) ^ flip
            ws, _ = wss[which]
            ws[:nbytes].fill_(0xFF if which else 0x00)
            call(entry, bp, xi.ptr(), xi.ld, B, H, W, C, *extra, dt_of(dtype), ws.data_ptr(), nbytes, stream())
            return {"x": xi}, []
        return run
    both(make(0))                                                # contiguous on the 0x00 workspace, strided on the 0xFF one
    both(make(1))                                                # and the other way round: every result has the same bits
    assert all(guard_ok(g) for _, g in wss), f"{entry}: wrote behind its workspace"


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W,shift", [(8, 8, 0), (16, 16, 4), (8, 24, 4), (16, 16, 0)])
@pytest.mark.parametrize("C,heads", [(32, 1), (128, 4), (256, 8), (64, 1)])
def test_lewin_block_entry_points_in_place_on_concat_half(dtype, H, W, shift, C, heads):
    """uf_lewin_attn_fwd, uf_leff_fwd, uf_lewin_block_fwd, uf_lewin_block_train_fwd: C = 32 / 128 / 256 on the fused kernels (attn_block
    changes form at C >= 256), C = 64 with one head of 64 channels on the unfused route."""
    blk = block_module(C, H, W, heads, shift)
    bp = blk._pack(dtype)
    x = torch.randn(B * H * W, C, generator=gen(21))
    drop = torch.tensor([1.25, 0.0]).cuda()
    _block_runs("uf_lewin_attn_fwd", bp, x, H, W, C, dtype, (None, 0))
    _block_runs("uf_leff_fwd", bp, x, H, W, C, dtype)
    _block_runs("uf_lewin_block_fwd", bp, x, H, W, C, dtype, (None, 0))
    if C // heads == 32:                                         # DropPath scales need the fused attention kernel: head_dim 32 (f32: C <= 256)
        _block_runs("uf_lewin_block_train_fwd", bp, x, H, W, C, dtype, (drop.data_ptr(), drop.data_ptr()))


@pytest.mark.parametrize("dtype", MODES)
def test_lewin_block_with_user_mask_in_place_on_concat_half(dtype):
    """a caller mask sends the block down the unfused route: shift-4 windows that also carry a dense user mask"""
    H = W = 16
    C, heads = 32, 1
    blk = block_module(C, H, W, heads, 4)
    um = torch.where(torch.rand(4, 64, 64, generator=gen(22)) < 0.3, -100.0, 0.0)
    um[:, :, 0] = 0
    um = um.cuda().contiguous()
    _block_runs("uf_lewin_block_fwd", blk._pack(dtype), torch.randn(B * H * W, C, generator=gen(23)), H, W, C, dtype, (um.data_ptr(), 4))


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W", [(8, 8), (4, 12)])
def test_lewin_block4_in_place_on_concat_half(dtype, H, W):
    from uformer_amd import model
    C, heads = 64, 2
    torch.manual_seed(4)
    blk = model.LeWinTransformerBlock(C, (4, 4), heads).cuda().eval()
    _block_runs("uf_lewin_block4_fwd", blk._pack(dtype), torch.randn(B * H * W, C, generator=gen(24)), H, W, C, dtype, (None, None))


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("H,W,shift", [(8, 8, 0), (16, 16, 4), (8, 24, 4)])
@pytest.mark.parametrize("C,heads", [(32, 1), (128, 4), (256, 8)])
def test_lewin_attn_train_fwd_strided(dtype, H, W, shift, C, heads):
    blk = block_module(C, H, W, heads, shift)
    bp = blk._pack(dtype)
    M = B * H * W
    x = torch.randn(M, C, generator=gen(25))
    drop = torch.tensor([1.25, 0.0]).cuda()

    def run(edge):
        xi, x1 = pv(edge, M, C, F32, "cat", x), pv(edge, M, C, F32, "strided")
        o = {n: pv(edge, M, C, dtype, "guard") for n in ("xn", "q", "k", "vt", "o", "z")}
        o["a1"] = pv(edge, M, 4 * C, dtype, "guard")
        call("uf_lewin_attn_train_fwd", bp, xi.ptr(), xi.ld, x1.ptr(), x1.ld, B, H, W, C, drop.data_ptr(), dt_of(dtype),
             *[o[n].ptr() for n in ("xn", "q", "k", "vt", "o", "z", "a1")], stream())
        o["x1"] = x1
        return o, [xi]
    both(run)


# ---------------------------------------------------------------------------------------------------------------------------
# Part A: backward entry points
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W,windowed,shift", [(8, 8, 0, 0), (16, 16, 1, 4), (8, 24, 1, 4)])
@pytest.mark.parametrize("C", [32, 256])
def test_layernorm_bwd_strided_and_poisoned(dtype, H, W, windowed, shift, C):
    """uf_layernorm_bwd_fused / _cast: strided x, dy, add and dx; dgamma / dbeta / cast_out pre-filled with poison (OVERWRITTEN);
    workspace 0x00 and 0xFF."""
    M = B * H * W
    x = torch.randn(M, C, generator=gen(26)) * 1.7 + 0.3
    dy = torch.randn(M, C, generator=gen(27))
    add = torch.randn(M, C, generator=gen(28))
    gm = E.ln_affine(C)[0].cuda()
    scale = torch.tensor([1.25, 0.5]).cuda()
    nbytes = max(16, lib().uf_layernorm_bwd_workspace_bytes(M, C))
    wss = ws_bytes_pair(nbytes)

    def make(cast):
        def run(edge):
            xi, dyi, addi = pv(edge, M, C, F32, "cat", x), pv(edge, M, C, dtype, "strided", dy), pv(edge, M, C, F32, "cat", add)     # add shares ld_dx with dx
            dx, dg, db = pv(edge, M, C, F32, "cat"), pv(True, 1, C, F32, "guard"), pv(True, 1, C, F32, "guard")
            ws, _ = wss[int(edge)]
            ws[:nbytes].fill_(0xFF if edge else 0x00)
            head = (xi.ptr(), xi.ld, gm.data_ptr(), dyi.ptr(), dyi.ld, int(dtype == F32), addi.ptr(), dx.ptr(), dx.ld, dg.ptr(), db.ptr(), B, H, W, C, windowed, shift, dt_of(dtype))
            outs = {"dx": dx, "dgamma": dg, "dbeta": db}
            if cast:
                outs["cast"] = co = pv(True, M, C, dtype, "guard")
                call("uf_layernorm_bwd_cast", *head, co.ptr(), scale.data_ptr(), 1, shift, ws.data_ptr(), nbytes, stream())
            else:
                call("uf_layernorm_bwd_fused", *head, ws.data_ptr(), nbytes, stream())
            return outs, [xi, dyi, addi]
        return run
    both(make(False))
    both(make(True))
    assert all(guard_ok(g) for _, g in wss)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("M,N,K", [(64, 96, 32), (333, 48, 16), (1000, 256, 256)])
def test_linear_wgrad_and_rows_sum_strided_and_poisoned(dtype, M, N, K):
    dy = torch.randn(M, N, generator=gen(29))
    x = torch.randn(M, K, generator=gen(30))
    nb = max(16, lib().uf_linear_wgrad_workspace_bytes(M, N, K))
    nr = max(16, lib().uf_rows_sum_workspace_bytes(M, N))
    wss, wsr = ws_bytes_pair(nb), ws_bytes_pair(nr)

    def run_w(edge):
        dyi, xi = pv(edge, M, N, dtype, "strided", dy), pv(edge, M, K, dtype, "cat", x)
        dW, db = pv(True, N, K, F32, "guard"), pv(True, 1, N, F32, "guard")
        call("uf_linear_wgrad", dyi.ptr(), dyi.ld, xi.ptr(), xi.ld, dW.ptr(), db.ptr(), M, N, K, dt_of(dtype), wss[int(edge)][0].data_ptr(), nb, stream())
        return {"dW": dW, "db": db}, [dyi, xi]

    def run_s(edge):
        dyi, out = pv(edge, M, N, dtype, "strided", dy), pv(True, 1, N, F32, "guard")
        call("uf_rows_sum", dyi.ptr(), dyi.ld, out.ptr(), M, N, dt_of(dtype), wsr[int(edge)][0].data_ptr(), nr, stream())
        return {"sum": out}, [dyi]
    both(run_w)
    both(run_s)
    assert all(guard_ok(g) for _, g in wss + wsr)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W", [(8, 8), (16, 16), (8, 24)])
@pytest.mark.parametrize("Cin,acc", [(32, 0), (32, 1), (128, 1)])
def test_downsample_bwd_strided_and_poisoned(dtype, H, W, Cin, acc):
    from uformer_amd import packing
    Cout, M, Mo = 2 * Cin, B * H * W, B * (H // 2) * (W // 2)
    x = torch.randn(M, Cin, generator=gen(31))
    dy = torch.randn(Mo, Cout, generator=gen(32)).cuda()
    base = torch.randn(M, Cin, generator=gen(33))
    wpt = packing.pack_downsample((torch.randn(Cout, Cin, 4, 4, generator=gen(34)) * (16 * Cin) ** -0.5).cuda(), dtype).t().contiguous()
    nbytes = lib().uf_downsample_bwd_workspace_bytes(B, H, W, Cin, Cout, dt_of(dtype))
    wss = ws_bytes_pair(nbytes)

    def run(edge):
        xi = pv(edge, M, Cin, F32, "cat", x)
        dx = pv(edge, M, Cin, F32, "cat", base if acc else None)       # without accumulate: the live view stays poisoned, dx is OVERWRITTEN
        dW, db = pv(True, Cout, 16 * Cin, F32, "guard"), pv(True, 1, Cout, F32, "guard")
        call("uf_downsample_bwd", xi.ptr(), xi.ld, dy.data_ptr(), wpt.data_ptr(), dx.ptr(), dx.ld, acc, dW.ptr(), db.ptr(), B, H, W, Cin, Cout, dt_of(dtype),
             wss[int(edge)][0].data_ptr(), nbytes, stream())
        return {"dx": dx, "dW": dW, "db": db}, [xi]
    both(run)
    assert all(guard_ok(g) for _, g in wss)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W", [(8, 8), (4, 12)])
@pytest.mark.parametrize("Cin,Cout", [(64, 32), (512, 256)])
def test_upsample_cat_bwd(dtype, H, W, Cin, Cout):
    """the gradient of a 2 Cout-wide concat buffer whose right half (the skip's gradient) is poisoned; dx, dW_pk, db pre-filled with
    poison; workspace both ways; and dx, dW_pk, db against float64 autograd of conv_transpose2d(k = 2, s = 2) on the T-rounded operands.
    Tolerances (of the max, as tests/test_gpu_bwd.py): dx bf16 8e-3 / f16 2e-3 = pick(dtype, ., 8e-3) of
    test_downsample_input_gradient_patch_form, which runs the 2-byte types only; dx f32 2e-4 = TOL[float32] there, the gate of the
    input gradient in test_linear_wgrad_and_input_grad (its 1e-6 compares two routes of the same rounded products, and a float32 sum
    over K = 4 Cout = 1024 terms measures 1.5e-6 against float64); dW, db 2e-4 / 2e-3 / 5e-4 = pick(dtype, 2e-4, 2e-3) of
    test_linear_wgrad_and_input_grad."""
    from uformer_amd import packing
    M = B * H * W
    x = torch.randn(M, Cin, generator=gen(35))
    d = torch.randn(4 * M, Cout, generator=gen(36))
    w = torch.randn(Cin, Cout, 2, 2, generator=gen(37)) / Cin ** 0.5
    wpt = packing.pack_upsample(w.cuda(), dtype).t().contiguous()
    nbytes = lib().uf_upsample_cat_bwd_workspace_bytes(B, H, W, Cin, Cout, dt_of(dtype))
    wss = ws_bytes_pair(nbytes)
    keep = {}

    def run(edge):
        di = pv(edge, 4 * M, Cout, F32, "cat_left", d)
        xi = pv(edge, M, Cin, F32, "guard", x)                           # x rows must be dense: ld_x == Cin by contract
        dx, dW, db = pv(True, M, Cin, F32, "guard"), pv(True, 4 * Cout, Cin, F32, "guard"), pv(True, 1, Cout, F32, "guard")
        call("uf_upsample_cat_bwd", di.ptr(), di.ld, xi.ptr(), Cin, wpt.data_ptr(), dx.ptr(), dW.ptr(), db.ptr(), B, H, W, Cin, Cout, dt_of(dtype),
             wss[int(edge)][0].data_ptr(), nbytes, stream())
        keep.update(dx=dx, dW=dW, db=db)
        return {"dx": dx, "dW": dW, "db": db}, [di, xi]
    both(run)
    assert all(guard_ok(g) for _, g in wss)
    # a strided x is rejected before any launch (UF_REQUIRE ld_x == Cin)
    assert lib().uf_upsample_cat_bwd(keep["dx"].ptr(), 2 * Cout, keep["dx"].ptr(), Cin + 16, wpt.data_ptr(), keep["dx"].ptr(), keep["dW"].ptr(), keep["db"].ptr(),
                                     B, H, W, Cin, Cout, dt_of(dtype), wss[0][0].data_ptr(), nbytes, stream()) == -1
    rq = E.rnd(dtype)
    xr = rq(x).double().reshape(B, H, W, Cin).permute(0, 3, 1, 2).requires_grad_(True)
    wr = rq(w).double().requires_grad_(True)
    br = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv_transpose2d(xr, wr, br, stride=2)
    y.backward(rq(d).double().reshape(B, 2 * H, 2 * W, Cout).permute(0, 3, 1, 2))
    rdx = xr.grad.permute(0, 2, 3, 1).reshape(M, Cin)
    rdW = wr.grad.permute(2, 3, 1, 0).reshape(4 * Cout, Cin)
    rel = lambda a, b: float((a.double().cpu() - b).abs().max() / b.abs().max())            # noqa: E731
    tx = {F32: 2e-4, BF16: 8e-3, F16: 2e-3}[dtype]
    tw = {F32: 2e-4, BF16: 2e-3, F16: 5e-4}[dtype]
    ex, ew, eb = rel(keep["dx"].live(), rdx), rel(keep["dW"].live(), rdW), rel(keep["db"].live().reshape(-1), br.grad)
    print(f"upsample_cat_bwd {E.TAG[dtype]} {Cin}->{Cout} {H}x{W}: dx {ex:.3e} dW {ew:.3e} db {eb:.3e}")
    assert ex < tx and ew < tw and eb < tw, (ex, ew, eb)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("H,W", [(8, 8), (4, 12)])
def test_window4_attention_strided(dtype, H, W):
    C, heads, M = 64, 2, B * H * W
    qkv = torch.randn(M, 3 * C, generator=gen(38))
    do = torch.randn(M, C, generator=gen(39))
    rpb4 = torch.randn(heads, 49, generator=gen(40)).cuda()
    nwin = B * (H // 4) * (W // 4)

    def run_f(edge):
        qi, o = pv(edge, M, 3 * C, dtype, "strided", qkv), pv(edge, M, C, dtype, "cat")
        call("uf_window4_attention_fwd", qi.ptr(), qi.ld, rpb4.data_ptr(), o.ptr(), o.ld, B, H, W, C, heads, dt_of(dtype), stream())
        return {"o": o}, [qi]

    def run_b(edge):
        qi, doi = pv(edge, M, 3 * C, dtype, "strided", qkv), pv(edge, M, C, dtype, "cat", do)
        dq, ds = pv(edge, M, 3 * C, dtype, "strided"), pv(True, nwin * heads * 16, 16, F32, "guard")
        call("uf_window4_attention_bwd", qi.ptr(), qi.ld, rpb4.data_ptr(), doi.ptr(), doi.ld, dq.ptr(), dq.ld, ds.ptr(), B, H, W, C, heads, dt_of(dtype), stream())
        return {"dqkv": dq, "dscore": ds}, [qi, doi]
    both(run_f)
    both(run_b)


# ---------------------------------------------------------------------------------------------------------------------------
# Part A: workspace poisoning of the composite entry points
# ---------------------------------------------------------------------------------------------------------------------------
def _model_twice(m, x, monkeypatch):
    """two forwards of a whole model on workspaces this test owns (0x00, then 0xFF): same bits, guard bytes untouched"""
    outs, guards = [], []
    for fill in (0x00, 0xFF):
        def own(need, device, fill=fill):
            buf, guard = E.poisoned_bytes(int(need), 4096, fill, device)
            guards.append((buf, guard))
            return buf[:need]
        monkeypatch.setattr(m, "_workspace", own)
        with torch.no_grad():
            outs.append(m(x))
        torch.cuda.synchronize()
    assert len(guards) == 2 and all(guard_ok(g) for _, g in guards), "the model wrote behind its workspace"
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the result depends on the initial contents of the workspace"


@pytest.mark.parametrize("dtype", MODES)
def test_uformer_fwd_does_not_depend_on_workspace_contents(dtype, monkeypatch):
    from uformer_amd import model, spec
    cfg = spec.arch_config("tiny", img_size=128)
    m = model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), modulator=cfg.modulator,
                      compute_dtype=dtype).eval()
    m.load_state_dict(spec.synth_state_dict(cfg, 7), strict=True)
    _model_twice(m.cuda(), spec.synth_input(1, 128, 128, 7).cuda(), monkeypatch)


@pytest.mark.parametrize("dtype", MODES)
def test_uformer_win4_fwd_does_not_depend_on_workspace_contents(dtype, monkeypatch):
    from uformer_amd import model, spec
    cfg = spec.arch_config("tiny", img_size=64)
    m = model.Uformer(img_size=64, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), modulator=cfg.modulator,
                      compute_dtype=dtype).eval()
    m.load_state_dict(spec.synth_state_dict(cfg, 8), strict=True)
    _model_twice(m.cuda(), spec.synth_input(1, 64, 64, 8).cuda(), monkeypatch)


@pytest.mark.parametrize("dtype", MODES)
def test_unet_fwd_does_not_depend_on_workspace_contents(dtype, monkeypatch):
    from uformer_amd import model
    torch.manual_seed(9)
    m = model.UNet(dim=16, compute_dtype=dtype).eval().cuda()
    _model_twice(m, torch.rand(1, 3, 32, 32, generator=gen(9)).cuda(), monkeypatch)


@pytest.mark.parametrize("dtype", MODES)
def test_block_backward_does_not_depend_on_workspace_or_output_contents(dtype):
    """uf_lewin_block_bwd: workspace 0x00 / 0xFF, dx and every parameter gradient pre-filled with NaN (OVERWRITTEN by contract)"""
    from uformer_amd import _lib, ops, spec, train
    H, C, heads, shift = 16, 64, 2, 4
    cfg = spec.arch_config("tiny32", 128)
    sd = {k: v.cuda() for k, v in spec.synth_state_dict(cfg, 11).items()}
    pk = train.BlockPack(sd, "decoderlayer_3.blocks.0.", heads, shift, dtype, fused=False)
    M = B * H * H
    x, dy = torch.randn(M, C, generator=gen(41)).cuda(), torch.randn(M, C, generator=gen(42)).cuda()
    drop = torch.tensor([[1.25, 0.0], [0.0, 1.25]]).cuda()
    nbytes = ops.lewin_block_bwd_workspace_bytes(B, H, H, C, heads, dtype)
    res = []
    for (ws, guard), fill in zip(ws_bytes_pair(nbytes), (0.0, float("nan"))):
        flat, g, views = ops._block_grads(C, heads, True, "cuda")
        flat.fill_(fill)
        dx = torch.full((M, C), fill, device="cuda")
        _lib.check(lib().uf_lewin_block_bwd(ctypes.byref(pk.train_params), x.data_ptr(), dy.data_ptr(), dx.data_ptr(), drop[0].data_ptr(), drop[1].data_ptr(),
                                            ctypes.byref(g), B, H, H, C, dt_of(dtype), ws.data_ptr(), nbytes, stream()), "uf_lewin_block_bwd")
        torch.cuda.synchronize()
        assert guard_ok(guard)
        res.append((dx, views))
    assert torch.isfinite(res[1][0]).all() and torch.equal(res[0][0], res[1][0])
    for k, v in res[0][1].items():
        assert torch.isfinite(res[1][1][k]).all() and torch.equal(v, res[1][1][k]), k


@pytest.mark.parametrize("dtype", MODES)
def test_dwconv3x3_bwd_does_not_depend_on_workspace_or_output_contents(dtype):
    Hh, W, C = 8, 24, 128
    dc = torch.randn(B, Hh, W, C, generator=gen(43)).to(dtype).cuda()
    pre = torch.randn(B, Hh, W, C, generator=gen(44)).to(dtype).cuda()
    w9f = (torch.randn(9, C, generator=gen(45)) / 3).cuda()
    nbytes = max(16, lib().uf_dwconv3x3_bwd_workspace_bytes(C, dt_of(dtype)))
    res = []
    for ws, guard in ws_bytes_pair(nbytes):
        da, dw9, db = pv(True, B * Hh * W, C, dtype, "guard"), pv(True, 9, C, F32, "guard"), pv(True, 1, C, F32, "guard")
        call("uf_dwconv3x3_bwd", dc.data_ptr(), w9f.data_ptr(), pre.data_ptr(), da.ptr(), dw9.ptr(), db.ptr(), B, Hh, W, C, dt_of(dtype), ws.data_ptr(), nbytes, stream())
        torch.cuda.synchronize()
        assert guard_ok(guard)
        res.append((da, dw9, db))
    for a, b in zip(*res):
        assert a.guard_intact() and b.guard_intact() and not torch.isnan(b.live().float()).any() and torch.equal(a.live_bits(), b.live_bits())


# ---------------------------------------------------------------------------------------------------------------------------
# Part B: hard inputs, gated row by row against float64
# ---------------------------------------------------------------------------------------------------------------------------
def record(name, got, emu, exact, out_dtype):
    """the per-row metric of the kernel and of the emulation, their ratio into the report, and the gate"""
    k, e = float(E.row_err(got.cpu(), exact).max()), float(E.row_err(emu, exact).max())
    lim = E.gate(e, out_dtype)
    REPORT[name] = {"kernel": k, "emulation": e, "ratio": (k / e if e > 0 else (0.0 if k == 0 else float("inf"))), "gate": lim}
    print(f"{name}: kernel {k:.3e} emulation {e:.3e} gate {lim:.3e}")
    return k <= lim, f"{name}: kernel worst row {k:.3e} > gate {lim:.3e} (emulation {e:.3e})"


def assert_all(results):
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("C", E.LN_CS)
def test_layernorm_hard_rows(dtype, C):
    """uf_layernorm_fwd, uf_ln_qkv_fwd (value third, unwindowed map of 128 tokens = 2 windows in raster = window order at W = 8) and
    uf_ln_linear_gelu_fwd on every LayerNorm class"""
    from uformer_amd import ops
    gm, bt = E.ln_affine(C)
    heads = max(1, C // 32)
    w1, b1 = E.gemm_weights(4 * C, C, dtype, 50 + C)
    wq, bq = E.gemm_weights(3 * C, C, dtype, 51 + C)
    res = []
    for cls in E.LN_CLASSES:
        x = E.ln_rows(cls, C)
        exact, emu = E.ln_ref(x, gm, bt), E.ln_emu(x, gm, bt, dtype)
        got = ops.layernorm(x.cuda(), gm.cuda(), bt.cuda(), B=1, H=16, W=8, dtype=dtype)
        res.append(record(f"layernorm_fwd/{cls}/C{C}/{E.TAG[dtype]}", got.float(), emu, exact, dtype))
        # LN2 -> linear1 -> GELU: reference = float64 of the same composition on the T-valued weight; the GELU form is the type's
        h_exact = E.gelu_ref(E.linear_ref(exact, w1, b1), dtype)
        h_emu = E.gelu_emu(E.linear_emu(emu, w1, b1), dtype)
        got = ops.ln_linear_gelu(x.cuda(), gm.cuda(), bt.cuda(), w1.cuda(), b1.cuda())
        res.append(record(f"ln_linear_gelu_fwd/{cls}/C{C}/{E.TAG[dtype]}", got.float(), h_emu, h_exact, dtype))
        # LN1 -> q | k | v: 16x8 map, shift 0 = windows (0..63), (64..127) in raster order
        y_exact = E.linear_ref(exact, wq, bq)
        y_emu = E.rnd(dtype)(E.linear_emu(emu, wq, bq))
        q, k, vt = ops.ln_qkv(x.cuda(), gm.cuda(), bt.cuda(), wq.cuda(), bq.cuda(), heads, B=1, H=16, W=8)
        hd = C // heads
        kk = k.float().cpu().permute(0, 2, 1, 3).reshape(128, C)
        vv = vt.float().cpu().permute(0, 3, 1, 2).reshape(128, C)
        res.append(record(f"ln_qkv_fwd.k/{cls}/C{C}/{E.TAG[dtype]}", kk, y_emu[:, C:2 * C], y_exact[:, C:2 * C], dtype))
        res.append(record(f"ln_qkv_fwd.v/{cls}/C{C}/{E.TAG[dtype]}", vv, y_emu[:, 2 * C:], y_exact[:, 2 * C:], dtype))
        qq = q.float().cpu().permute(0, 2, 1, 3).reshape(128, C)
        res.append(record(f"ln_qkv_fwd.q/{cls}/C{C}/{E.TAG[dtype]}", qq, E.rnd(dtype)(E.linear_emu(emu, wq, bq)[:, :C] * hd ** -0.5), y_exact[:, :C] * hd ** -0.5, dtype))
    assert_all(res)


@pytest.mark.parametrize("C", E.LN_CS)
def test_layernorm_backward_hard_rows(C):
    from uformer_amd import ops
    gm, _ = E.ln_affine(C)
    dy = torch.randn(E.LN_ROWS, C, generator=gen(C))
    res = []
    for cls in E.LN_CLASSES:
        x = E.ln_rows(cls, C)
        exact, emu = E.ln_bwd_ref(x, gm, dy), E.ln_bwd_ref(x, gm, dy, torch.float32)
        got = ops.layernorm_bwd(x.cuda(), gm.cuda(), dy.cuda())
        for name, g_, e_, x_ in zip(("dx", "dgamma", "dbeta"), got, emu, exact):
            if name != "dx":                                    # one row each: the whole vector is the row
                g_, e_, x_ = g_.reshape(1, -1), e_.reshape(1, -1), x_.reshape(1, -1)
            res.append(record(f"layernorm_bwd.{name}/{cls}/C{C}/f32", g_.float(), e_, x_, F32))
    assert_all(res)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("cls", E.GELU_CLASSES)
def test_gelu_family_hard_grid(dtype, cls):
    """uf_gelu_fwd, uf_gelu_bwd, uf_dwconv3x3_gelu_fwd (centre tap 1: the stencil is the identity), uf_dwconv3x3_mul_dgelu and
    uf_linear_mul_dgelu (identity weight) on the grid: finite in, finite out, within the gate"""
    from uformer_amd import ops
    x = E.gelu_grid(cls, dtype)                                 # (64, 64), T-valued
    R, C = x.shape
    dy = torch.ones_like(x)
    xa, dya = x.to(dtype).cuda(), dy.to(dtype).cuda()
    f_exact, f_emu = E.gelu_ref(x, dtype), E.gelu_emu(x, dtype)
    g_exact, g_emu = E.gelu_grad_ref(x, dtype), E.gelu_grad_emu(x, dy, dtype)
    res = [record(f"gelu_fwd/{cls}/{E.TAG[dtype]}", ops.gelu(xa).float(), f_emu, f_exact, dtype),
           record(f"gelu_bwd/{cls}/{E.TAG[dtype]}", ops.gelu_bwd(xa, dya).float(), g_emu, g_exact, dtype)]
    w9 = torch.zeros(9, C)
    w9[4] = 1.0
    zero = torch.zeros(C)
    got = ops.dwconv3x3_gelu(xa.reshape(1, 8, 8, C), w9.cuda(), zero.cuda())
    res.append(record(f"dwconv3x3_gelu_fwd/{cls}/{E.TAG[dtype]}", got.reshape(R, C).float(), f_emu, f_exact, dtype))
    got = ops.dwconv3x3_mul_dgelu(dya.reshape(1, 8, 8, C), w9.cuda(), xa.reshape(1, 8, 8, C))
    res.append(record(f"dwconv3x3_mul_dgelu/{cls}/{E.TAG[dtype]}", got.reshape(R, C).float(), g_emu, g_exact, dtype))
    da, _, _ = ops.dwconv3x3_bwd(dya.reshape(1, 8, 8, C), w9.cuda(), xa.reshape(1, 8, 8, C))
    res.append(record(f"dwconv3x3_bwd.da/{cls}/{E.TAG[dtype]}", da.reshape(R, C).float(), g_emu, g_exact, dtype))
    got = ops.linear_mul_dgelu(dya, torch.eye(C).to(dtype).cuda(), zero.cuda(), xa)
    res.append(record(f"linear_mul_dgelu/{cls}/{E.TAG[dtype]}", got.float(), g_emu, g_exact, dtype))
    assert_all(res)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("hd", [16, 32, 64])
def test_attention_core_hard_rows(dtype, heads, hd):
    from uformer_amd import ops
    res = []
    for cls in E.ATT_CLASSES:
        case = E.attention_case(cls, heads, hd, dtype)
        exact, emu = E.attention_ref(case), E.attention_emu(case, dtype)
        got = ops.window_attention_core(case["q"].cuda(), case["k"].cuda(), case["vt"].cuda(), case["bias"].cuda(), H=E.ATT_H, W=E.ATT_W,
                                        shift=case["shift"], mask=None if case["mask"] is None else case["mask"].cuda())
        res.append(record(f"window_attention_fwd/{cls}/h{heads}_d{hd}/{E.TAG[dtype]}", got.float(), emu, exact, dtype))
    assert_all(res)


@pytest.mark.parametrize("dtype", MODES)
def test_window4_attention_hard_rows(dtype):
    """uf_window4_attention_fwd, C = 64 with 2 heads on the 2 x 2 windows of an 8 x 8 map"""
    from uformer_amd import ops
    res = []
    for cls in E.ATT4_CLASSES:
        case = E.attention4_case(cls, 2, 32, dtype)
        got = ops.window4_attention(case["qkv"].cuda(), case["rpb4"].cuda(), 1, E.ATT4_H, E.ATT4_W, 2)
        res.append(record(f"window4_attention_fwd/{cls}/h2_d32/{E.TAG[dtype]}", got.float(), E.attention4_emu(case, dtype), E.attention4_ref(case)[0], dtype))
    assert_all(res)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("hd", [16, 32, 64])
def test_attention_backward_hard_rows(dtype, heads, hd):
    """uf_window_attention_bwd: dq (wrt the scaled q), dk, dv^T row by row (rows of head_dim values), dbias row by row"""
    from uformer_amd import ops
    do = torch.randn(E.ATT_NW * 64, heads * hd, generator=gen(hd)).to(dtype)
    res = []
    for cls in E.ATT_CLASSES:
        case = E.attention_case(cls, heads, hd, dtype)
        exact, emu = E.attention_bwd(case, do, None), E.attention_bwd(case, do, dtype)
        dq, dk, dvt, dbias = ops.window_attention_bwd(case["q"].cuda(), case["k"].cuda(), case["vt"].cuda(), case["bias"].cuda(), do.cuda(), E.ATT_H, E.ATT_W,
                                                      shift=case["shift"], mask=None if case["mask"] is None else case["mask"].cuda())
        got = (dq.float().cpu(), dk.float().cpu(), dvt.float().cpu().transpose(-1, -2), dbias.float().cpu())
        for name, g_, e_, x_, od in zip(("dq", "dk", "dv", "dbias"), got, emu, exact, (dtype, dtype, dtype, F32)):
            res.append(record(f"window_attention_bwd.{name}/{cls}/h{heads}_d{hd}/{E.TAG[dtype]}", g_.reshape(x_.shape), e_, x_, od))
    assert_all(res)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("C", E.LN_CS)
def test_lewin_block_hard_layernorm_rows(dtype, C):
    """the LN1 and LN2 inside uf_lewin_block_fwd (the fused kernels carry their own LayerNorm code): 2 images of 8 x 8 tokens = 128 rows
    of every LayerNorm class through a whole block, against the float64 block; emulation = oracle/bf16_budget.py's block with every
    rounding point of the type on, float32, halving-tree LayerNorm sums"""
    heads = max(1, C // 32)
    blk = block_module(C, 8, 8, heads, 0)
    p = E.block_params({k: v.detach().cpu() for k, v in blk.state_dict().items()}, dtype)
    res = []
    for cls in E.LN_CLASSES:
        x = E.ln_rows(cls, C).reshape(2, 64, C)
        with torch.no_grad():
            got = blk(x.cuda(), None, dtype)
        res.append(record(f"lewin_block_fwd/{cls}/C{C}/{E.TAG[dtype]}", got.float().reshape(-1, C), E.block_emu(x, p, heads, dtype).reshape(-1, C),
                          E.block_ref(x, p, heads, dtype).reshape(-1, C), F32))
    assert_all(res)


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("C", E.LN_CS)
def test_layernorm_backward_fused_hard_rows(dtype, C):
    """uf_layernorm_bwd_fused as the block backward calls it: dy of the operand type in WINDOW order (16 x 8 map, shift 4), a second
    gradient added into dx"""
    from oracle import uformer_oracle as O
    from uformer_amd import ops
    gm, _ = E.ln_affine(C)
    idx = torch.from_numpy(O.window_partition_index(1, 16, 8, 8, 4))
    dy_tok = torch.randn(E.LN_ROWS, C, generator=gen(C)).to(dtype)           # T-valued, token order
    add = torch.randn(E.LN_ROWS, C, generator=gen(C + 1))
    res = []
    for cls in E.LN_CLASSES:
        x = E.ln_rows(cls, C)
        exact, emu = E.ln_bwd_ref(x, gm, dy_tok), E.ln_bwd_ref(x, gm, dy_tok, torch.float32)
        exact, emu = (exact[0] + add.double(),) + exact[1:], (emu[0] + add,) + emu[1:]
        got = ops.layernorm_bwd_fused(x.cuda(), gm.cuda(), dy_tok[idx].cuda(), 1, 16, 8, add=add.cuda(), windowed=True, shift=4)
        for name, g_, e_, x_ in zip(("dx", "dgamma", "dbeta"), got, emu, exact):
            if name != "dx":
                g_, e_, x_ = g_.reshape(1, -1), e_.reshape(1, -1), x_.reshape(1, -1)
            res.append(record(f"layernorm_bwd_fused.{name}/{cls}/C{C}/{E.TAG[dtype]}", g_.float(), e_, x_, F32))
    assert_all(res)
