"""CPU: rectangular inputs (H != W).  The rectangle-general composition (tests/rect_composition.py) is pinned to the oracle at H == W and
checked for transpose equivariance; the whole-model plan is checked through the C ABI (uf_uformer_workspace_bytes needs no device memory);
the Python surface refuses to guess the shape of a non-square token map."""
import ctypes

import pytest
import torch

import rect_composition as R
from oracle import uformer_oracle as O
from uformer_amd import spec


def _sd(cfg, seed=1234):
    return spec.synth_state_dict(cfg, seed)


def _fwd(x, sd, cfg, fn, mask=None):
    return fn(x, sd, img_size=cfg.img_size, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads, dd_in=cfg.dd_in, mask=mask)


@pytest.mark.parametrize("ctor", [128, 256])
@pytest.mark.parametrize("with_mask", [False, True])
def test_composition_equals_oracle_on_square_inputs(ctor, with_mask):
    cfg = spec.arch_config("tiny32", img_size=ctor)
    sd = _sd(cfg)
    x = spec.synth_input(1, ctor, ctor, 77)
    mask = None
    if with_mask:
        g = torch.Generator().manual_seed(5)
        mask = (torch.rand(1, 1, ctor, ctor, generator=g) > 0.5).float()
    with torch.no_grad():
        ref = _fwd(x, sd, cfg, O.uformer_forward, mask)
        got = _fwd(x, sd, cfg, R.uformer_forward, mask)
    assert (got - ref).abs().max().item() <= 1e-6


@pytest.mark.parametrize("ctor", [128, 256])
def test_composition_is_transpose_equivariant(ctor):
    """uformer(x^T; weights^T) == uformer(x; weights)^T on a 128 x 256 map (at ctor 256 the bottleneck is 8 x 16 with shift 4: one
    window tall).  Independent of any oracle: a mix-up of H and W breaks it."""
    cfg = spec.arch_config("tiny32", img_size=ctor)
    sd = _sd(cfg)
    x = spec.synth_input(1, 128, 256, 78)
    with torch.no_grad():
        y = _fwd(x, sd, cfg, R.uformer_forward)
        yt = _fwd(x.transpose(-1, -2).contiguous(), R.transpose_state_dict(sd), cfg, R.uformer_forward)
    assert y.shape == (1, 3, 128, 256) and yt.shape == (1, 3, 256, 128)
    assert (yt.transpose(-1, -2) - y).abs().max().item() <= 1e-5
    # and the shift really matters at the one-window-tall bottleneck: without the transposed tables the result differs
    with torch.no_grad():
        yw = _fwd(x.transpose(-1, -2).contiguous(), sd, cfg, R.uformer_forward)
    assert (yw.transpose(-1, -2) - y).abs().max().item() > 1e-4


def _plan_bytes(embed_dim, B, H, W, sz):
    """uf_uformer_workspace_bytes restated per axis: 4 decoder concat buffers, the bottleneck stream, the largest block scratch, slack."""
    al = lambda n: (n + 255) // 256 * 256                                   # noqa: E731
    mult, div = [1, 2, 4, 8, 16, 16, 8, 4, 2], [1, 2, 4, 8, 16, 8, 4, 2, 1]
    C = [embed_dim * m for m in mult]
    M = [B * (H // d) * (W // d) for d in div]
    blk = max(al(M[s] * C[s] * sz) + 2 * al(M[s] * 4 * C[s] * sz) for s in range(9))
    off = sum(al(M[5 + k] * C[5 + k] * 4) for k in range(4)) + al(M[4] * C[4] * 4)
    return off + blk + 256 * 256


def _desc(embed_dim):
    from uformer_amd import _lib
    d = _lib.ModelDesc()
    d.embed_dim, d.dd_in, d.in_chans = embed_dim, 3, 3
    return d


# recorded from the library before rectangular inputs existed (square plans must not change)
SQUARE_BYTES = {(32, 1, 128, 2): 26935296, (32, 16, 256, 2): 1719730176, (32, 2, 1280, 4): 9148891136, (16, 8, 512, 2): 1719730176}


def test_workspace_bytes_follow_the_per_axis_plan():
    from uformer_amd import _lib
    from uformer_amd._lib import UF_BF16, UF_F32
    lib = _lib.load()
    for e, B, X, sz in SQUARE_BYTES:
        dt = UF_BF16 if sz == 2 else UF_F32
        assert lib.uf_uformer_workspace_bytes(ctypes.byref(_desc(e)), B, X, X, dt) == SQUARE_BYTES[(e, B, X, sz)] == _plan_bytes(e, B, X, X, sz)
    for (H, W) in ((768, 1280), (1280, 768), (128, 256), (384, 128)):
        for dt, sz in ((UF_BF16, 2), (UF_F32, 4)):
            got = lib.uf_uformer_workspace_bytes(ctypes.byref(_desc(32)), 2, H, W, dt)
            assert got == _plan_bytes(32, 2, H, W, sz), (H, W, got, _last_error())


def _last_error():
    from uformer_amd import _lib
    return _lib.last_error()


@pytest.mark.parametrize("H,W,name", [(256, 200, "W=200"), (192, 256, "H=192"), (0, 128, "H=0")])
def test_plan_names_the_failing_dimension(H, W, name):
    from uformer_amd import _lib
    from uformer_amd._lib import UF_BF16
    assert _lib.load().uf_uformer_workspace_bytes(ctypes.byref(_desc(32)), 1, H, W, UF_BF16) == 0
    assert name in _last_error(), _last_error()


def test_module_forwards_do_not_guess_a_rectangular_shape():
    from uformer_amd import model, train
    from uformer_amd._lib import UformerHipError
    assert train.block_hw(256, None) == (16, 16)
    assert train.block_hw(128, (8, 16)) == (8, 16)
    with pytest.raises(UformerHipError, match="not a square map"):
        train.block_hw(128, None)
    with pytest.raises(UformerHipError, match="does not match"):
        train.block_hw(128, (8, 8))
    x = torch.zeros(1, 8 * 16, 32)
    for mod in (model.Downsample(32, 64), model.Upsample(32, 16), model.LeFF(32, 128)):
        with pytest.raises(UformerHipError, match="not a square map"):
            mod(x)
    blk = model.LeWinTransformerBlock(32, (16, 16), 1, shift_size=4).eval()
    with torch.no_grad(), pytest.raises(UformerHipError, match="not a square map"):
        blk(x)


def test_restore_rejects_an_unknown_canvas():
    from uformer_amd import infer
    with pytest.raises(ValueError, match="canvas"):
        infer.restore(None, torch.zeros(1, 3, 8, 8), canvas="circle")
