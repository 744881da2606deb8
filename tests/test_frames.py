"""CPU: the uint8 frame interface (uf_frames.hip, infer.restore_frames, infer.FrameRestorer) as far as it can be held without a GPU: the
argument refusals of the four entry points (they run before any launch), the ValueErrors of the Python layer, the float64 restatement of the
tile blend against restore_tiled, and the facts about the quantiser reference that make the exact GPU test discriminate."""
import ctypes

import numpy as np
import pytest
import torch

import frames_cases as FC

NULL, SHAPE, UNSUPPORTED = -6, -1, -2
A, Bp, Cp = 4096, 8192, 12288             # stand-ins for device addresses: every refusal happens before anything is dereferenced or launched


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _refused(rc, code, *words):
    from uformer_amd import _lib
    msg = _lib.last_error()
    assert rc == code, (rc, msg)
    for wd in words:
        assert wd in msg, msg


def test_frames_to_canvas_refusals():
    from uformer_amd import _lib
    f = _lib.load().uf_frames_to_canvas
    _refused(f(None, 1, 0, Bp, None, 1, 3, 8, 8, 128, 128, None), NULL, "uf_frames_to_canvas", "null")
    _refused(f(A, 1, 0, None, None, 1, 3, 8, 8, 128, 128, None), NULL, "null")
    _refused(f(A, 1, 0, Bp, None, 1, 0, 8, 8, 128, 128, None), UNSUPPORTED, "C=0")
    _refused(f(A, 1, 0, Bp, None, 1, 9, 8, 8, 128, 128, None), UNSUPPORTED, "C=9")
    _refused(f(A, 1, 1, Bp, None, 1, 2, 8, 8, 128, 128, None), UNSUPPORTED, "swap_rb", "C=2")
    _refused(f(A, 1, 0, Bp, None, 1, 3, 130, 8, 128, 128, None), SHAPE, "smaller than the image", "Xh=128")
    _refused(f(A, 1, 0, Bp, None, 1, 3, 8, 130, 256, 128, None), SHAPE, "smaller than the image", "Xw=128")
    _refused(f(A, 1, 0, Bp, None, 0, 3, 8, 8, 128, 128, None), SHAPE, "B=0")
    _refused(f(A, 1, 0, Bp, None, 8, 4, 8192, 8192, 8192, 8192, None), SHAPE, "2^31")          # exactly 2^31 canvas elements
    _refused(f(A, 1, 0, Bp, None, 2, 8, 8192, 16384, 8192, 16384, None), SHAPE, "2^31")


def test_canvas_to_frames_refusals():
    from uformer_amd import _lib
    f = _lib.load().uf_canvas_to_frames
    _refused(f(None, Bp, 1, 0, 1, 3, 8, 8, 128, 128, None), NULL, "uf_canvas_to_frames", "null")
    _refused(f(A, None, 1, 0, 1, 3, 8, 8, 128, 128, None), NULL, "null")
    _refused(f(A, Bp, 1, 0, 1, 5, 8, 8, 128, 128, None), UNSUPPORTED, "C=5")
    _refused(f(A, Bp, 1, 0, 1, 0, 8, 8, 128, 128, None), UNSUPPORTED, "C=0")
    _refused(f(A, Bp, 0, 1, 1, 1, 8, 8, 128, 128, None), UNSUPPORTED, "swap_rb")
    _refused(f(A, Bp, 1, 0, 1, 3, 8, 200, 128, 128, None), SHAPE, "smaller than the image")
    _refused(f(A, Bp, 1, 0, 8, 4, 8, 8, 8192, 8192, None), SHAPE, "2^31")


def test_tiles_gather_refusals():
    from uformer_amd import _lib
    f = _lib.load().uf_tiles_gather
    _refused(f(None, 1, 1, 0, Bp, Cp, 2, 1, 3, 200, 300, 128, None), NULL, "uf_tiles_gather", "null")
    _refused(f(A, 1, 1, 0, None, Cp, 2, 1, 3, 200, 300, 128, None), NULL, "null")
    _refused(f(A, 1, 1, 0, Bp, None, 2, 1, 3, 200, 300, 128, None), NULL, "null")
    _refused(f(A, 1, 1, 0, Bp, Cp, 2, 1, 9, 200, 300, 128, None), UNSUPPORTED, "C=9")
    _refused(f(A, 1, 1, 1, Bp, Cp, 2, 1, 1, 200, 300, 128, None), UNSUPPORTED, "swap_rb")
    _refused(f(A, 1, 1, 0, Bp, Cp, 2, 1, 3, 200, 300, 100, None), SHAPE, "tile=100", "multiple of 128")
    _refused(f(A, 1, 1, 0, Bp, Cp, 2, 1, 3, 200, 300, 0, None), SHAPE, "multiple of 128")
    _refused(f(A, 1, 1, 0, Bp, Cp, 0, 1, 3, 200, 300, 128, None), SHAPE, "T=0")
    _refused(f(A, 1, 1, 0, Bp, Cp, 1024, 1, 2, 4096, 4096, 1024, None), SHAPE, "2^31")          # exactly 2^31 tile elements
    _refused(f(A, 0, 1, 0, Bp, Cp, 1, 2, 4, 8192, 8192, 128, None), SHAPE, "2^31")              # f32 frames of 2^31 bytes


def test_tiles_blend_refusals():
    from uformer_amd import _lib
    f = _lib.load().uf_tiles_blend
    ys, xs = _ints(0, 72), _ints(0, 86, 172)
    ok = dict(ny=2, nx=3, B=1, C=3, h=200, w=300, tile=128)

    def call(t=A, ys=ys, xs=xs, out=Bp, u8=1, hwc=1, swap=0, **kw):
        a = dict(ok, **kw)
        return f(t, ys, a["ny"], xs, a["nx"], out, u8, hwc, swap, 1, a["B"], a["C"], a["h"], a["w"], a["tile"], None)

    _refused(call(t=None), NULL, "uf_tiles_blend", "null")
    _refused(call(out=None), NULL, "null")
    _refused(call(ys=None), NULL, "null")
    _refused(call(xs=None), NULL, "null")
    _refused(call(C=5), UNSUPPORTED, "C=5", "u8")
    _refused(call(C=9, u8=0), UNSUPPORTED, "C=9", "f32")
    _refused(call(C=2, swap=1), UNSUPPORTED, "swap_rb")
    _refused(call(tile=100), SHAPE, "tile=100", "multiple of 128")
    _refused(call(ny=0), SHAPE, "ny=0")
    _refused(call(nx=65), SHAPE, "nx=65")
    _refused(call(ys=_ints(0, 150)), SHAPE, "y starts")                        # a gap between the tiles
    _refused(call(ys=_ints(8, 72)), SHAPE, "y starts")                         # does not begin at 0
    _refused(call(xs=_ints(0, 86, 171)), SHAPE, "x starts")                    # stops short of the far side
    _refused(call(xs=_ints(0, 172, 86)), SHAPE, "x starts")                    # not ascending
    big_y, big_x = _ints(*range(0, 4096, 512)), _ints(*range(0, 4096, 512))
    _refused(call(ys=big_y, xs=big_x, ny=8, nx=8, B=8, C=4, h=4096, w=4096, tile=1024), SHAPE, "2^31")   # 64 tiles x 8 x 4 x 2^20 = 2^31 elements


def test_python_layer_raises_value_errors_before_touching_a_device():
    from uformer_amd import infer
    m = torch.nn.Identity()
    u8 = torch.zeros(1, 16, 24, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="canvas"):
        infer.restore_frames(m, u8, canvas="round")
    with pytest.raises(ValueError, match="bgr"):
        infer.restore_frames(m, torch.zeros(1, 16, 24, 2, dtype=torch.uint8), bgr=True)
    with pytest.raises(ValueError, match="bgr"):
        infer.restore_frames(m, torch.zeros(1, 2, 16, 24, dtype=torch.uint8), hwc=False, bgr=True)
    with pytest.raises(ValueError, match="uint8"):
        infer.restore_frames(m, u8.float())
    with pytest.raises(ValueError, match=r"\(B,h,w,C\)"):
        infer.restore_frames(m, u8[0])
    with pytest.raises(ValueError, match="multiple of 128"):
        infer.restore_frames(m, u8, tile=100)

    with pytest.raises(ValueError, match="canvas"):
        infer.FrameRestorer(m, (16, 24, 3), canvas="round")
    with pytest.raises(ValueError, match="bgr"):
        infer.FrameRestorer(m, (16, 24, 1), bgr=True)
    for depth in (0, 5, -1):
        with pytest.raises(ValueError, match="depth"):
            infer.FrameRestorer(m, (16, 24, 3), depth=depth)
    with pytest.raises(ValueError, match="frame_shape"):
        infer.FrameRestorer(m, (16, 24))
    with pytest.raises(ValueError, match="multiple of 128"):
        infer.FrameRestorer(m, (16, 24, 3), tile=200)
    r = infer.FrameRestorer(m, (16, 24, 3), batch=2, depth=4)
    with pytest.raises(ValueError, match="uint8"):
        r.submit(np.zeros((2, 16, 24, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="frames must be"):
        r.submit(np.zeros((2, 16, 25, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="frames must be"):
        r.submit(torch.zeros(16, 24, 3, dtype=torch.uint8))                    # the unbatched form is for batch 1 only
    r.close()
    with pytest.raises(RuntimeError, match="closed"):
        r.submit(np.zeros((2, 16, 24, 3), dtype=np.uint8))


@pytest.mark.parametrize("h,w,tile,ov", FC.BLEND_CASES)
def test_blend_restatement_is_restore_tiled(h, w, tile, ov):
    """The float64 restatement the GPU test compares uf_tiles_blend with -- ramps in closed form, the sum over ALL covering tiles -- against
    restore_tiled itself run with a pointwise callable (as tests/test_host_logic.py does), on the tiles gather_ref cuts."""
    from uformer_amd import infer
    seen = []

    def pointwise(t):
        seen.append(t.clone())
        return 0.5 * t + 0.125 * t * t + 0.1

    img = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(h * 1000 + w))
    got = infer.restore_tiled(pointwise, img, tile=tile, min_overlap=ov, max_batch=4, clamp=False)
    ys, xs = infer._starts(h, tile, ov), infer._starts(w, tile, ov)
    tiles = FC.gather_ref(img.numpy(), ys, xs, tile)
    assert np.array_equal(tiles, torch.cat(seen, 0).numpy()), "gather_ref is the tile batch restore_tiled builds"
    t64 = tiles.astype(np.float64)
    ref = FC.blend_ref(0.5 * t64 + 0.125 * t64 * t64 + 0.1, ys, xs, h, w, tile)
    assert np.abs(got.numpy() - ref).max() <= 2e-6
    im64 = img.numpy().astype(np.float64)
    assert np.abs(ref - (0.5 * im64 + 0.125 * im64 * im64 + 0.1)).max() <= 1e-12          # a pointwise model: the blend returns the full-frame result


def test_blend_cases_cover_what_they_claim():
    from uformer_amd import infer
    ys = infer._starts(300, 128, 96)
    assert len(ys) == 7
    cover = np.zeros(300, dtype=int)
    for y in ys:
        cover[y:y + 128] += 1
    assert cover.max() == 5 and cover.min() >= 1
    assert infer._starts(128, 128, 64) == [0] and infer._starts(100, 128, 32) == [0]
    assert infer._starts(130, 128, 126) == [0, 2]


def test_blend_inputs_keep_the_reference_clear_of_half_levels():
    """the u8 blend test excludes pixels whose reference lies within 1e-3 of a half level; the seeded inputs keep that share under its 1 % cap"""
    for i, (h, w, tile, ov) in enumerate(FC.BLEND_CASES):
        t, ys, xs = FC.blend_inputs(h, w, tile, ov, seed=i)
        share = FC.near_half_level(FC.blend_ref(t, ys, xs, h, w, tile)).mean()
        assert share <= 0.01, (h, w, share)


def test_quantiser_reference_facts():
    """What the exact GPU test of uf_canvas_to_frames relies on: the round trip of all 256 levels is the identity; among the 765 tie candidates the
    float32 product lands exactly on a half level 256 times (so the tie rule matters) and decides differently from a float64 product 128 times
    (so the precision of the product matters): a kernel that multiplies in double or rounds half away from zero fails."""
    u = np.arange(256, dtype=np.float32)
    assert np.array_equal(np.rint((u / FC.F255) * FC.F255), u)
    assert np.array_equal(FC.quantise_ref(u / FC.F255), np.arange(256, dtype=np.uint8))
    v = FC.tie_candidates()
    assert v.shape == (765,) and v.dtype == np.float32
    p32 = v * FC.F255
    assert p32.dtype == np.float32
    assert int((p32 - np.floor(p32) == np.float32(0.5)).sum()) == 256
    p64 = v.astype(np.float64) * 255.0
    assert int((np.rint(p32) != np.rint(p64)).sum()) == 128
    away = np.floor(p32 + np.float32(0.5))                                     # half away from zero on the float32 product
    assert int((away != np.rint(p32)).sum()) > 0
    h = FC.hard_values()
    q = FC.quantise_ref(h)
    assert q[np.isnan(h)].tolist() == [0] and q[h == np.inf].tolist() == [255] and q[h == -np.inf].tolist() == [0]
    assert np.array_equal(q[:765], np.rint(p32).astype(np.uint8))
