"""GPU: the residual epilogue of uf_dwconv_linear2_fwd at C >= 128 INSIDE the persistent walk, to the bit, and the refusal of uf_debug_set_tbuf
by a library built without kernel stamps.

At C >= 128 the consumer waves of the kernel add linear2's result to residual rows they fetch in the epilogue (narrower widths request them an
interval ahead).  The cases have more tiles than resident workgroups, so a workgroup's accumulators and rows roll over to a second (or third)
tile; tests/test_gpu_saturated.py walks only at C <= 64.  Inputs are the saturated lattice of tests/saturated_lattice.py: the output is exact in
float32, no tolerance appears here, every element is compared with torch.equal.

  (13, 64, 64, 128)  832 tiles   both C = 128 forms walk (512 / 768 resident workgroups)
  (9, 64, 64, 256)   576 tiles   the 4-consumer form walks two tiles, "leff2=1" three
  (5, 64, 64, 512)   320 tiles   one workgroup per CU, two tiles

Each case runs on a dense stream (row stride C between poisoned guard rows) and once more as the upper half of a 2C-wide buffer whose other
half holds NaN patterns that must come back bit for bit.
"""
import pytest
import torch

import saturated_lattice as S
from edge_cases import PoisonedView
from exact_lattice import BF16, F16, F32, MODES, TAG, UF_ERR_UNSUPPORTED
from test_gpu_saturated import call, dense, dev, dt, fm, st, variant

pytestmark = pytest.mark.gpu

CASES = [(13, 64, 64, 128), (9, 64, 64, 256), (5, 64, 64, 512)]
VARIANTS = [None, "leff2=1", "leff2=2", "persist=0"]


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C", CASES, ids=["C128", "C256", "C512"])
def test_epilogue_in_persistent_walk(dtype, B, H, W, C):
    c = S.leff2_case(B, H, W, C, dtype)
    M = B * H * W
    want = c["out"].to(F32)
    assert torch.equal(want.double(), c["out"]), "the reference is not a float32 lattice"
    w9, bdw, b2, w2 = dev(c["w9"]), dev(c["bdw"]), dev(c["b2"]), fm(c["w2"], dtype)
    hi, x0 = dense(M, 4 * C, dtype, c["h1"]), dev(c["x"])
    want = want.cuda()
    for v in VARIANTS:
        if v is not None and dtype == F32 and v.startswith("leff2"):
            continue                                                     # the eight-producer-wave forms exist for the 2-byte types only
        for mode in ("guard", "cat"):                                    # row stride C, then the upper half of a 2C-wide buffer
            xi = PoisonedView(M, C, F32, mode, "cuda").fill(x0)
            with variant(v):
                call("uf_dwconv_linear2_fwd", hi.ptr(), w9.data_ptr(), bdw.data_ptr(), w2.data_ptr(), b2.data_ptr(), xi.ptr(), xi.ld, B, H, W, C, dt(dtype), st())
            tag = f"{TAG[dtype]} {B}x{H}x{W} C={C} {v} ld={xi.ld}"
            assert torch.equal(xi.live(), want), f"{tag}: output differs from the float64 reference"
            assert xi.guard_intact(), f"{tag}: wrote outside the rows (guard rows or the other half of the buffer)"
            assert hi.guard_intact(), f"{tag}: wrote around the hidden tensor"


def test_default_build_refuses_stamp_buffer():
    """a library built without kernel stamps refuses a stamp buffer, never writes to it, and accepts NULL"""
    from uformer_amd import _lib, model
    lib = _lib.load()
    tb = torch.full((65536 * 8 + 4096 * 8,), 0xFF, dtype=torch.uint8, device="cuda")     # stamps + census entries of a few workgroups, as scripts/ubench.py sizes it
    rc = lib.uf_debug_set_tbuf(tb.data_ptr())
    if rc == 0:
        lib.uf_debug_set_tbuf(None)
        pytest.skip("the loaded library is a diagnostic build (UF_STAMPS=1)")
    try:
        assert rc == UF_ERR_UNSUPPORTED
        assert "UF_STAMPS" in _lib.last_error()
        B, H, W, C, dtype = 1, 8, 8, 32, BF16
        torch.manual_seed(3)
        blk = model.LeWinTransformerBlock(C, (H, W), 1, win_size=8, shift_size=0).cuda().eval()
        bp = blk._pack(dtype)
        x = torch.randn(B * H * W, C, generator=torch.Generator().manual_seed(4)).cuda()
        x_in = x.clone()
        nbytes = lib.uf_block_workspace_bytes(B * H * W, C, dt(dtype))
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        call("uf_lewin_block_fwd", bp, x.data_ptr(), C, B, H, W, C, None, 0, dt(dtype), ws.data_ptr(), nbytes, st())
        assert torch.isfinite(x).all() and not torch.equal(x, x_in), "the block did not run"
        assert bool((tb == 0xFF).all()), "a kernel of a default build wrote to the refused stamp buffer"
    finally:
        assert lib.uf_debug_set_tbuf(None) == 0
