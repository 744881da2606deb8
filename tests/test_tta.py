"""CPU: the geometric self-ensemble (uf_tta_gather, uf_tta_merge, infer.restore_ensemble) as far as it can be held without a GPU: the restatement
the GPU tests compare the kernels with (tests/tta_cases.py) against the oracle's transforms, the argument refusals of the two entry points (they
run before any launch) and the ValueErrors of the Python layer."""
import ctypes

import pytest
import torch

import tta_cases as TC

NULL, SHAPE, UNSUPPORTED = -6, -1, -2
A, Bp, Cp = 4096, 8192, 12288             # stand-ins for device addresses: every refusal happens before anything is dereferenced or launched


def _ints(*v):
    return (ctypes.c_int * max(1, len(v)))(*v)


def _refused(rc, code, *words):
    from uformer_amd import _lib
    msg = _lib.last_error()
    assert rc == code, (rc, msg)
    for wd in words:
        assert wd in msg, msg


def test_transforms_are_the_oracles():
    from oracle import uformer_oracle as O
    for (h, w) in [(5, 9), (9, 5), (1, 1), (4, 4)]:
        x = torch.arange(2 * 3 * h * w, dtype=torch.float64).reshape(2, 3, h, w)
        for k in range(8):
            assert torch.equal(TC.transform(x, k), O.augment(x, k)), (h, w, k)


def test_inverse_after_transform_is_the_identity_on_non_square_arrays():
    for (h, w) in [(5, 9), (9, 5), (1, 7)]:
        x = torch.arange(3 * h * w, dtype=torch.float64).reshape(1, 3, h, w)
        for k in range(8):
            t = TC.transform(x, k)
            assert tuple(t.shape[-2:]) == ((w, h) if k % 2 else (h, w))
            assert torch.equal(TC.inverse(t, k), x), (h, w, k)
            assert torch.equal(TC.transform(TC.inverse(x.transpose(-1, -2) if k % 2 else x, k), k), x.transpose(-1, -2) if k % 2 else x)
    assert [k for k in range(8) if TC.INVERSE[k] != k] == [1, 3]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("canvas", ["square", "rect"])
def test_a_per_pixel_model_gets_its_single_result_back_bit_for_bit(canvas, dtype):
    img = torch.rand(2, 3, 37, 150, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dtype)
    one = TC.single(TC.per_pixel, img, canvas)
    assert torch.equal(one, TC.per_pixel(img))
    for n in (8, 4, 2, 1):
        assert torch.equal(TC.ensemble(TC.per_pixel, img, canvas, n), one), n


def test_the_tree_is_what_makes_equal_members_exact():
    """eight equal float32 members: the pairwise sum times 1/8 returns the member, a running sum does not always"""
    v = torch.rand(100000, generator=torch.Generator().manual_seed(1), dtype=torch.float32)
    assert torch.equal(TC.tree_sum([v] * 8) * 0.125, v)
    run = v.clone()
    for _ in range(7):
        run = run + v
    assert 0.38 < float((run * 0.125 != v).float().mean()) < 0.47            # 41 % of these uniform [0, 1) draws (44 % was found for another draw)


def test_member_batch_order_and_placement():
    img = torch.rand(2, 1, 5, 9, dtype=torch.float64)
    b = TC.member_batch(img, (1, 3), 128, 128)
    assert tuple(b.shape) == (4, 1, 128, 128)
    assert torch.equal(TC.crop(b[2:4], 9, 5), TC.transform(img, 3)) and float(b.sum()) == pytest.approx(float(img.sum()) * 2)
    assert b[0, 0, (128 - 9) // 2, (128 - 5) // 2] == img[0, 0, 4, 0]                      # T_1: member(0, 0) = img(h-1, 0)
    assert TC.canvas_of(100, 200, "rect", 0) == (128, 256) and TC.canvas_of(100, 200, "rect", 1) == (256, 128)
    assert TC.canvas_of(100, 200, "square", 1) == (256, 256)


def test_tta_gather_refusals():
    from uformer_amd import _lib
    f = _lib.load().uf_tta_gather

    def call(src=A, out=Bp, ks=_ints(0, 2, 4, 6), n=4, u8=1, hwc=1, swap=0, B=1, C=3, h=100, w=200, Xh=256, Xw=256):
        return f(src, u8, hwc, swap, out, ks, n, B, C, h, w, Xh, Xw, None)

    _refused(call(src=None), NULL, "uf_tta_gather", "null")
    _refused(call(out=None), NULL, "null")
    _refused(call(ks=None), NULL, "null")
    _refused(call(C=0), UNSUPPORTED, "C=0")
    _refused(call(C=9), UNSUPPORTED, "C=9")
    _refused(call(C=2, swap=1), UNSUPPORTED, "swap_rb", "C=2")
    _refused(call(ks=_ints(0, 2, 8, 6)), UNSUPPORTED, "=8", "0 ... 7")
    _refused(call(ks=_ints(0, -2, 4, 6)), UNSUPPORTED, "=-2")
    _refused(call(ks=_ints(0, 2, 2, 6)), UNSUPPORTED, "ascending")
    _refused(call(ks=_ints(0, 4, 2, 6)), UNSUPPORTED, "ascending")
    _refused(call(ks=_ints(0, 1, 2, 3)), UNSUPPORTED, "parit")
    _refused(call(ks=_ints(1, 3, 5), n=3), UNSUPPORTED, "n=3")
    _refused(call(n=0), UNSUPPORTED, "n=0")
    _refused(call(B=0), SHAPE, "B=0")
    _refused(call(Xh=128, Xw=128), SHAPE, "smaller than the member")
    _refused(call(Xh=128, Xw=256, ks=_ints(1, 3, 5, 7)), SHAPE, "smaller than the member", "h=200 w=100")      # the odd members want 256 x 128
    assert call(src=None, Xh=256, Xw=128, ks=_ints(1, 3, 5, 7)) == NULL                                         # ... which passes the shape checks
    _refused(call(B=8, C=8, h=4096, w=4096, Xh=4096, Xw=4096), SHAPE, "2^31")                                   # 4 x 8 x 8 x 2^24 = 2^32 elements
    _refused(call(ks=_ints(0), n=1, B=8, C=4, h=8192, w=8192, Xh=8192, Xw=8192), SHAPE, "2^31")                  # exactly 2^31
    big = 2 ** 31 - 1                                                                                           # products that no 64-bit integer holds
    _refused(call(B=big, C=8, Xh=big, Xw=big), SHAPE, "2^31")
    _refused(call(B=big, C=8, h=big, w=big, Xh=big, Xw=big, ks=_ints(1, 3, 5, 7)), SHAPE, "2^31")


def test_tta_merge_refusals():
    from uformer_amd import _lib
    f = _lib.load().uf_tta_merge
    E, O = _ints(0, 2, 4, 6), _ints(1, 3, 5, 7)

    def call(even=A, kse=E, ne=4, Xh=128, Xw=256, odd=Bp, kso=O, no=4, Xoh=256, Xow=128, out=Cp, u8=1, hwc=1, swap=0, B=1, C=3, h=100, w=200):
        return f(even, kse, ne, Xh, Xw, odd, kso, no, Xoh, Xow, out, u8, hwc, swap, 1, B, C, h, w, None)

    _refused(call(out=None), NULL, "uf_tta_merge", "null")
    _refused(call(even=None), NULL, "null")
    _refused(call(odd=None), NULL, "null")
    _refused(call(kse=None), NULL, "null")
    _refused(call(kso=None), NULL, "null")
    _refused(call(C=5), UNSUPPORTED, "C=5", "u8")
    _refused(call(C=9, u8=0), UNSUPPORTED, "C=9", "f32")
    _refused(call(C=2, swap=1), UNSUPPORTED, "swap_rb")
    _refused(call(even=None, kse=None, ne=0, odd=None, kso=None, no=0), UNSUPPORTED, "n=0")
    _refused(call(ne=2, kse=_ints(0, 4), no=1, kso=_ints(1)), UNSUPPORTED, "n=3")
    _refused(call(ne=5), UNSUPPORTED, "ne=5")
    _refused(call(kse=_ints(0, 2, 4, 8)), UNSUPPORTED, "=8")
    _refused(call(kse=_ints(0, 2, 2, 6)), UNSUPPORTED, "ks_even", "ascending")
    _refused(call(kso=_ints(1, 5, 3, 7)), UNSUPPORTED, "ks_odd", "ascending")
    _refused(call(kse=_ints(0, 2, 4, 5)), UNSUPPORTED, "ks_even", "parit")
    _refused(call(kso=_ints(0, 3, 5, 7)), UNSUPPORTED, "ks_odd", "parit")
    _refused(call(B=0), SHAPE, "B=0")
    _refused(call(Xh=64), SHAPE, "even canvas", "smaller")
    _refused(call(Xoh=128, Xow=256), SHAPE, "odd canvas", "smaller")
    _refused(call(B=8, C=4, u8=0, h=4000, w=4000, Xh=4096, Xw=4096, Xoh=4096, Xow=4096), SHAPE, "2^31")         # 4 x 8 x 4 x 2^24 = 2^31 per buffer
    big = 2 ** 31 - 1                                                                                           # products that no 64-bit integer holds
    _refused(call(B=big, Xh=big, Xw=big, Xoh=big, Xow=big), SHAPE, "2^31")
    _refused(call(B=big, C=4, h=big, w=big, Xh=big, Xw=big, Xoh=big, Xow=big), SHAPE, "2^31")
    # absent buffers are no refusal by themselves: the even four alone reach the null check of the output
    assert call(odd=None, kso=None, no=0, out=None) == NULL


def test_python_layer_refusals_before_touching_a_device():
    from uformer_amd import infer
    m = torch.nn.Identity()
    u8 = torch.zeros(1, 16, 24, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"(?s)ensemble.*tile|tile.*ensemble"):
        infer.restore_frames(m, u8, tile=128, ensemble=8)
    with pytest.raises(ValueError, match=r"(?s)ensemble.*tile|tile.*ensemble"):
        infer.FrameRestorer(m, (16, 24, 3), tile=128, ensemble=8)
    for bad in (3, 0, 16, -1, True, "8"):
        with pytest.raises(ValueError, match="members must be 8, 4, 2 or 1"):
            infer.restore_ensemble(m, torch.zeros(1, 3, 16, 24), members=bad)
        with pytest.raises(ValueError, match="ensemble must be 8, 4, 2 or 1"):
            infer.restore_frames(m, u8, ensemble=bad)
        with pytest.raises(ValueError, match="ensemble must be 8, 4, 2 or 1"):
            infer.FrameRestorer(m, (16, 24, 3), ensemble=bad)
    with pytest.raises(ValueError, match="canvas must be 'square' or 'rect'"):
        infer.restore_ensemble(m, torch.zeros(1, 3, 16, 24), canvas="round")
    with pytest.raises(ValueError, match="canvas must be 'square' or 'rect'"):
        infer.restore_frames(m, u8, canvas="round", ensemble=8)
    with pytest.raises(ValueError, match=r"\(B,C,h,w\)"):
        infer.restore_ensemble(m, torch.zeros(3, 16, 24))
    # the existing checks keep their words and their order
    with pytest.raises(ValueError, match="frames must be uint8"):
        infer.restore_frames(m, u8.float(), ensemble=8)
    with pytest.raises(ValueError, match="tile must be a multiple of 128"):
        infer.restore_frames(m, u8, tile=100, ensemble=8)
    assert infer.ENSEMBLE_MEMBERS == TC.MEMBERS
    r = infer.FrameRestorer(m, (16, 24, 3), ensemble=4)
    assert r._kw["ensemble"] == 4
    r.close()
