"""attn_block at C <= 64 in its wave-per-window forms (UF_VARIANT "attn=4": one wave per window, "attn=5": two) against the first form
("attn=0"): the block's new rows AND h1 = GELU(linear1(LN2(rows))) must be equal bit for bit (torch.equal), through uf_lewin_attn_fwd
(the kernel without its fc1 phase) and uf_lewin_block_fwd (with it; h1 is read back from the workspace).

The selector is read with getenv on every call, so the variants are flipped inside one process.  Shapes are the smallest at which the forms can
go wrong: one head and two heads, 4 windows and 3 windows of a rectangular map, shifted windows (the last window row / column take the mask
branch), modulator on and off, one image and three, both 2-byte operand types, the stream at row stride 2C inside a concat buffer, and poisoned
pad columns + workspace (a tile index that belongs to another window, or a row read past the window, then shows up as NaN or as different bits).
"""
import os

import pytest
import torch

import edge_cases as E
from edge_cases import BF16, F16, F32, PoisonedView

pytestmark = pytest.mark.gpu

FIRST, WAVE1, WAVE2 = "attn=0", "attn=4", "attn=5"
WIDTHS = [(32, 1), (64, 2)]
MAPS = [(16, 16), (8, 24)]


class variant:
    """UF_VARIANT for the calls inside the block (None: the key is absent, the shape picks)"""

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


def lib():
    from uformer_amd import _lib
    return _lib.load()


def dt_of(dtype):
    from uformer_amd import ops
    return ops.uf_dtype(dtype)


def block_module(C, H, W, heads, shift, modulator):
    from uformer_amd import model
    torch.manual_seed(7 + C + shift + int(modulator))
    blk = model.LeWinTransformerBlock(C, (H, W), heads, win_size=8, shift_size=shift, modulator=modulator)
    with torch.no_grad():
        for n, p in blk.named_parameters():                      # biases and tables away from their zero initial values
            if p.dim() == 1 or "table" in n:
                p.add_(0.1 * torch.randn(p.shape))
    return blk.cuda().eval()


def run_block(bp, xbuf, ld, B, H, W, C, dtype, ws=None):
    """The kernel with and without its phase 3, in place on ``xbuf`` (an (M, C) f32 view with row stride ``ld``).  uf_lewin_attn_fwd runs it without
    (the attention half alone); uf_lewin_block_fwd runs it with h1 = GELU(linear1(LN2(rows))) and leaves h1 in the workspace (the LeFF
    kernel behind it only reads it).  Returns (rows after the attention half, h1 [M][4C] as bits); xbuf ends as the whole block's output."""
    from uformer_amd import _lib
    M, sz = B * H * W, torch.empty(0, dtype=dtype).element_size()
    nbytes = lib().uf_block_workspace_bytes(M, C, dt_of(dtype))
    if ws is None:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert tuple(xbuf.shape) == (M, C) and xbuf.stride() == (ld, 1)
    rows0 = xbuf.clone()
    _lib.check(lib().uf_lewin_attn_fwd(bp, xbuf.data_ptr(), ld, B, H, W, C, None, 0, dt_of(dtype), ws.data_ptr(), nbytes, st), "uf_lewin_attn_fwd")
    attn_rows = xbuf.clone()
    xbuf.copy_(rows0)
    _lib.check(lib().uf_lewin_block_fwd(bp, xbuf.data_ptr(), ld, B, H, W, C, None, 0, dt_of(dtype), ws.data_ptr(), nbytes, st), "uf_lewin_block_fwd")
    torch.cuda.synchronize()
    off = (M * C * sz + 255) // 256 * 256                        # the workspace's h1 region sits behind its T[M][C] region (256-byte aligned)
    return attn_rows, ws[off:off + M * 4 * C * sz].view(torch.int16).reshape(M, 4 * C).clone()


def run_plain(bp, x, B, H, W, C, dtype, which):
    """-> (rows after the attention half, whole block output, h1 bits) on a contiguous buffer and a zeroed workspace"""
    y = x.clone().cuda()
    with variant(which):
        rows, h1 = run_block(bp, y, C, B, H, W, C, dtype)
    return rows, y, h1


def check_ref(ref, x):
    rows, y, h1 = ref
    assert torch.isfinite(rows).all() and torch.isfinite(y).all() and not torch.equal(rows.cpu(), x)
    assert (h1 != 0).float().mean().item() > 0.9, "the reference run left no h1 in the workspace: the comparison would be empty"


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C,heads", WIDTHS)
def test_wave_forms_equal_first_form(dtype, H, W, C, heads):
    for shift in (0, 4):
        for modulator in (False, True):
            blk = block_module(C, H, W, heads, shift, modulator)
            bp = blk._pack(dtype)
            for B in (1, 3):
                x = torch.randn(B * H * W, C, generator=torch.Generator().manual_seed(11 * B + shift)) * 1.5 + 0.25
                ref = run_plain(bp, x, B, H, W, C, dtype, FIRST)
                check_ref(ref, x)
                for which in (WAVE1, WAVE2):
                    got = run_plain(bp, x, B, H, W, C, dtype, which)
                    tag = f"{which} C={C} {H}x{W} shift={shift} modulator={modulator} B={B}"
                    assert torch.equal(got[0], ref[0]), f"{tag}: rows after the attention half differ from the first form"
                    assert torch.equal(got[1], ref[1]), f"{tag}: block output differs from the first form"
                    assert torch.equal(got[2], ref[2]), f"{tag}: h1 differs from the first form"


@pytest.mark.parametrize("C,heads", WIDTHS)
def test_wave_forms_at_row_stride_2c(C, heads):
    """the stream as encoder stages run: the right half of a 2C-wide concat buffer; the left half must stay as it was"""
    B, H, W, dtype = 3, 8, 24, BF16
    blk = block_module(C, H, W, heads, 4, True)
    bp = blk._pack(dtype)
    M = B * H * W
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(5))
    left = torch.randn(M, C, generator=torch.Generator().manual_seed(6))
    ref = run_plain(bp, x, B, H, W, C, dtype, FIRST)
    check_ref(ref, x)
    for which in (WAVE1, WAVE2):
        buf = torch.cat([left, x], dim=1).cuda().contiguous()
        with variant(which):
            rows, h1 = run_block(bp, buf[:, C:], 2 * C, B, H, W, C, dtype)
        assert torch.equal(rows, ref[0]), f"{which}: rows at stride 2C differ from the contiguous first form"
        assert torch.equal(buf[:, C:], ref[1]), f"{which}: block output at stride 2C differs from the contiguous first form"
        assert torch.equal(buf[:, :C].cpu(), left), f"{which}: the other half of the concat buffer was written"
        assert torch.equal(h1, ref[2]), f"{which}: h1 differs"


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("C,heads", WIDTHS)
def test_wave_forms_on_poisoned_memory(dtype, C, heads):
    """pad columns, guard rows and the whole workspace hold NaN patterns beforehand: same bits out, nothing outside the view written"""
    B, H, W = 3, 8, 24
    blk = block_module(C, H, W, heads, 4, True)
    bp = blk._pack(dtype)
    M = B * H * W
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(9))
    ref = run_plain(bp, x, B, H, W, C, dtype, FIRST)
    check_ref(ref, x)
    nbytes = lib().uf_block_workspace_bytes(M, C, dt_of(dtype))
    for which in (WAVE1, WAVE2):
        xi = PoisonedView(M, C, F32, "cat", "cuda").fill(x.cuda())
        ws, guard = E.poisoned_bytes(int(nbytes), 4096, 0xFF, "cuda")
        with variant(which):
            rows, h1 = run_block(bp, xi.view, xi.ld, B, H, W, C, dtype, ws=ws)
        assert torch.equal(rows, ref[0]), f"{which}: rows after the attention half differ from the first form on clean memory"
        assert torch.equal(xi.live(), ref[1]), f"{which}: block output differs from the first form on clean memory"
        assert not torch.isnan(xi.live()).any(), f"{which}: a poisoned value reached the rows"
        assert xi.guard_intact(), f"{which}: wrote outside the view"
        assert torch.equal(h1, ref[2]), f"{which}: h1 differs from the first form on a zeroed workspace"
        assert bool((guard == 0xA5).all()), f"{which}: wrote behind the workspace"


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_whole_model_default_selection_equals_first_form(dtype):
    """tiny embed-32 model at 128 x 128, batch 2: whatever forms the shapes pick, the output is the first form's"""
    from uformer_amd import model, spec
    cfg = spec.arch_config("tiny32", img_size=128)
    sd = spec.synth_state_dict(cfg, 1234)
    x = spec.synth_input(2, 128, 128, 1234).cuda()
    m = model.Uformer(img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
                      modulator=cfg.modulator, compute_dtype=dtype).eval()
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    out = {}
    for which in (None, FIRST, WAVE1, WAVE2):
        with variant(which), torch.no_grad():
            out[which] = m(x)
        torch.cuda.synchronize()
    assert torch.isfinite(out[FIRST]).all()
    assert torch.equal(out[None], out[FIRST]), "default selection differs from the first form"
    assert torch.equal(out[WAVE1], out[FIRST]), "one wave per window everywhere it is built differs from the first form"
    assert torch.equal(out[WAVE2], out[FIRST]), "two waves per window everywhere it is built differs from the first form"
