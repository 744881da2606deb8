"""GPU: the geometric self-ensemble (uf_tta_gather, uf_tta_merge, infer.restore_ensemble, restore_frames / FrameRestorer with ensemble=).

  * uf_tta_gather, exact: every member equals uf_expand_canvas of T_k(planes) -- f32 and u8 sources, interleaved / planar / BGR, inside NaN / 0xA5
    guarded buffers at odd sizes and alignments, on the square canvas (eight members in two calls) and on the rect canvas with its swapped partner;
  * uf_tta_merge, exact against the restatement (tests/tta_cases.py) evaluated in f32 in the same tree order, on synthetic member canvases that
    are NaN outside the image regions; f32 with and without clamp, u8 through the numpy quantiser;
  * the {0}-only calls against the four existing entry points, the refusals with the output untouched;
  * restore_ensemble on a small model against the restatement's merge of the same model call, a per-pixel model, restore_frames and FrameRestorer."""
import ctypes
import math

import numpy as np
import pytest
import torch

import frames_cases as FC
import tta_cases as TC
from uformer_amd import spec

pytestmark = pytest.mark.gpu

POISON = 0xA5
NAN = float("nan")
EVEN, ODD = (0, 2, 4, 6), (1, 3, 5, 7)


def guarded(shape, dtype, guard, fill):
    """a contiguous view of `shape` inside a larger buffer filled with `fill`, `guard` elements in front and behind: (view, whole buffer)"""
    n = int(np.prod(shape))
    whole = torch.full((guard + n + guard,), fill, dtype=dtype, device="cuda")
    return whole[guard:guard + n].view(shape), whole


def guards_intact(whole, guard, fill):
    a, b = whole[:guard], whole[-guard:]
    if isinstance(fill, float) and math.isnan(fill):
        return bool(torch.isnan(a).all() and torch.isnan(b).all())
    return bool((a == fill).all() and (b == fill).all())


def u8_frames(B, C, h, w, hwc, seed):
    """every one of the 256 values (as far as the frame has room), shuffled"""
    rng = np.random.default_rng(seed)
    v = np.resize(np.arange(256, dtype=np.uint8), B * C * h * w)
    rng.shuffle(v)
    return v.reshape((B, h, w, C) if hwc else (B, C, h, w))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def unchanged(a, b):
    return same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)


def same_values(a, b):
    """equal where both are numbers, NaN in the same places"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


def sources(B, C, h, w):
    """(source tensor as the kernel takes it, hwc, swap_rb, f32 planes (B,C,h,w) in the model's channel order on the GPU)"""
    f32 = torch.rand(B, C, h, w, generator=torch.Generator().manual_seed(C * 100 + B)) * 1.5 - 0.25
    yield f32, False, False, f32.cuda()
    for hwc in (True, False):
        for swap in ((False, True) if C >= 3 else (False,)):
            f = u8_frames(B, C, h, w, hwc, seed=C * 10 + B)
            yield torch.from_numpy(f), hwc, swap, torch.from_numpy(FC.frames_as_planes(f, hwc, swap).astype(np.float32) / FC.F255).cuda()


@pytest.mark.parametrize("h,w", TC.SHAPES)
def test_gather_is_expand_canvas_of_the_transformed_planes(h, w):
    from uformer_amd import ops
    X = TC.canvas_of(h, w, "square", 0)[0]
    rect = TC.canvas_of(h, w, "rect", 0)
    calls = [(EVEN, X, X), (ODD, X, X), (EVEN, rect[0], rect[1] + 128), (ODD, rect[1] + 128, rect[0]),       # square; rect and its swapped partner
             ((0, 4), h, w), ((3,), w, h)]                                                                    # the member's own size: no padding at all
    for C in (1, 3, 4, 6):
        for B in (1, 3):
            for (src, hwc, swap, planes) in sources(B, C, h, w):
                g_in = 61 if B == 3 else 64                                            # a source pointer that is not 16-byte aligned
                fin, fin_whole = guarded(src.shape, src.dtype, g_in, POISON if src.dtype == torch.uint8 else NAN)
                fin.copy_(src)
                before = fin_whole.clone()
                for (ks, Xh, Xw) in calls:
                    want = torch.cat([ops.expand_canvas(TC.transform(planes, k).contiguous(), Xh, Xw, with_mask=False)[0] for k in ks], 0)
                    g_out = 63 if (B == 3 and hwc) else 64                             # ... and a canvas pointer that is not
                    out, o_whole = guarded((len(ks) * B, C, Xh, Xw), torch.float32, g_out, NAN)
                    assert ops.tta_gather(fin, ks, Xh, Xw, hwc=hwc, swap_rb=swap, out=out) is out
                    tag = (C, B, str(src.dtype), hwc, swap, ks, Xh, Xw)
                    assert torch.equal(out, want), tag
                    assert guards_intact(o_whole, g_out, NAN), tag
                assert unchanged(fin_whole, before), "the source is only read"
    # the wrapper allocates when no buffer is given
    got = ops.tta_gather(planes, ODD, X, X)
    assert tuple(got.shape) == (4 * 3, 6, X, X) and torch.equal(got, TC.member_batch(planes, ODD, X, X))


def member_canvases(B, C, h, w, ks, Xh, Xw, pool, shift):
    """host buffer (len(ks)*B, C, Xh, Xw): member m's region holds values of `pool`, everything else is NaN"""
    buf = torch.full((len(ks) * B, C, Xh, Xw), NAN, dtype=torch.float32)
    for m, k in enumerate(ks):
        hk, wk = (w, h) if k % 2 else (h, w)
        region = torch.from_numpy(np.resize(np.roll(pool, shift + 131 * k), B * C * h * w).reshape(B, C, hk, wk).copy())
        y0, x0 = (Xh - hk) // 2, (Xw - wk) // 2
        buf[m * B:(m + 1) * B, :, y0:y0 + hk, x0:x0 + wk] = region
    return buf


MERGE_SETS = [(EVEN, ODD), (EVEN, ()), ((0, 4), ()), ((0,), ()), ((), (3,)), ((0, 4), (1, 3)), ((), ODD), ((6,), (7,))]


@pytest.mark.parametrize("h,w", TC.SHAPES)
def test_merge_is_the_restated_tree_mean(h, w):
    from uformer_amd import ops
    pool = np.concatenate([FC.hard_values(), np.random.default_rng(5).random(3000, dtype=np.float32) * np.float32(1.4) - np.float32(0.2)])
    X = TC.canvas_of(h, w, "square", 0)[0]
    rect = TC.canvas_of(h, w, "rect", 0)
    for C, B in ((1, 1), (3, 3), (4, 1), (6, 3)):
        for case, (ke, ko) in enumerate(MERGE_SETS):
            square = case % 2 == 0
            (Xh, Xw), (Xoh, Xow) = ((X, X), (X, X)) if square else ((rect[0], rect[1] + 128), (rect[1] + 128, rect[0]))
            g = 63 if B == 3 else 64
            ne, no = len(ke), len(ko)
            if square:                                                                 # the two halves of one buffer
                whole_shape = ((ne + no) * B, C, X, X)
                both, whole = guarded(whole_shape, torch.float32, g, NAN)
                both.copy_(member_canvases(B, C, h, w, tuple(ke) + tuple(ko), X, X, pool, 7 * C + B))
                even, odd = (both[:ne * B] if ne else None), (both[ne * B:] if no else None)
                wholes = [whole]
            else:
                even = odd = None
                wholes = []
                if ne:
                    even, we = guarded((ne * B, C, Xh, Xw), torch.float32, g, NAN)
                    even.copy_(member_canvases(B, C, h, w, ke, Xh, Xw, pool, 7 * C + B))
                    wholes.append(we)
                if no:
                    odd, wo = guarded((no * B, C, Xoh, Xow), torch.float32, g, NAN)
                    odd.copy_(member_canvases(B, C, h, w, ko, Xoh, Xow, pool, 11 * C + B))
                    wholes.append(wo)
            before = [x.clone() for x in wholes]
            outputs = {k: even[m * B:(m + 1) * B] for m, k in enumerate(ke)} | {k: odd[m * B:(m + 1) * B] for m, k in enumerate(ko)}
            mean = TC.merge({k: v.cpu() for k, v in outputs.items()}, h, w).cuda()      # f32, the kernel's tree, IEEE arithmetic of the host
            assert mean.dtype == torch.float32 and tuple(mean.shape) == (B, C, h, w)
            tag = (C, B, ke, ko, square)
            out, o_whole = guarded((B, C, h, w), torch.float32, 61, NAN)
            assert ops.tta_merge(even, ke, odd, ko, h, w, u8=False, clamp=False, out=out) is out
            assert same_values(out, mean), tag
            assert guards_intact(o_whole, 61, NAN), tag
            assert same_values(ops.tta_merge(even, ke, odd, ko, h, w, u8=False, clamp=True), torch.clamp(mean, 0, 1)), tag
            if C <= 4:
                q = FC.quantise_ref(mean.cpu().numpy())
                for hwc in (True, False):
                    for swap in ((False, True) if C >= 3 else (False,)):
                        want = FC.planes_as_frames(q, hwc, swap)
                        frames, f_whole = guarded(want.shape, torch.uint8, 61, POISON)
                        ops.tta_merge(even, ke, odd, ko, h, w, u8=True, hwc=hwc, swap_rb=swap, out=frames)
                        got = frames.cpu().numpy()
                        assert np.array_equal(got, want), (tag, hwc, swap, int((got != want).sum()))
                        assert guards_intact(f_whole, 61, POISON), tag
            for x, b4 in zip(wholes, before):
                assert same_bits(x, b4), "the member canvases are only read"
    if (h, w) == TC.SHAPES[-1]:
        assert torch.isnan(mean).any() and h * w >= FC.hard_values().size, "the largest shape holds every hard value"


@pytest.mark.parametrize("h,w", TC.SHAPES)
def test_the_identity_member_alone_is_the_existing_entry_points(h, w):
    from uformer_amd import ops
    pool = np.concatenate([FC.hard_values(), np.random.default_rng(6).random(2000, dtype=np.float32) * np.float32(1.4) - np.float32(0.2)])
    X = TC.canvas_of(h, w, "square", 0)[0]
    for (Xh, Xw) in ((h, w), (X, X), (X, X + 128)):
        for C, B in ((1, 1), (3, 3), (4, 2)):
            for (src, hwc, swap, planes) in sources(B, C, h, w):
                src = src.cuda()
                if src.dtype == torch.uint8:
                    want = ops.frames_to_canvas(src, Xh, Xw, hwc=hwc, swap_rb=swap)[0]
                else:
                    want = ops.expand_canvas(src, Xh, Xw, with_mask=False)[0]
                assert same_bits(ops.tta_gather(src, (0,), Xh, Xw, hwc=hwc, swap_rb=swap), want), (C, B, hwc, swap, Xh, Xw)
            canvas = member_canvases(B, C, h, w, (0,), Xh, Xw, pool, C).cuda()
            for clamp in (False, True):
                assert same_bits(ops.tta_merge(canvas, (0,), None, (), h, w, u8=False, clamp=clamp), ops.crop_clamp_canvas(canvas, h, w, clamp)), (C, B, Xh, Xw, clamp)
            for hwc in (True, False):
                for swap in ((False, True) if C >= 3 else (False,)):
                    assert torch.equal(ops.tta_merge(canvas, (0,), None, (), h, w, u8=True, hwc=hwc, swap_rb=swap),
                                       ops.canvas_to_frames(canvas, h, w, hwc=hwc, swap_rb=swap)), (C, B, Xh, Xw, hwc, swap)


def test_refusals_leave_the_output_untouched():
    from uformer_amd import _lib
    lib = _lib.load()
    NULL, SHAPE, UNSUPPORTED = -6, -1, -2
    B, C, h, w = 1, 3, 20, 40
    src = torch.zeros(B, h, w, C, dtype=torch.uint8, device="cuda")
    out = torch.full((4 * B, C, 128, 128), NAN, dtype=torch.float32, device="cuda")
    ints = lambda *v: (ctypes.c_int * max(1, len(v)))(*v)

    def gather(src=src.data_ptr(), out=out.data_ptr(), ks=ints(0, 2, 4, 6), n=4, swap=0, B=B, C=C, h=h, w=w, Xh=128, Xw=128):
        return lib.uf_tta_gather(src, 1, 1, swap, out, ks, n, B, C, h, w, Xh, Xw, None)

    for rc, code in ((gather(src=None), NULL), (gather(ks=None), NULL), (gather(C=9), UNSUPPORTED), (gather(C=2, swap=1), UNSUPPORTED),
                     (gather(ks=ints(0, 2, 4, 9)), UNSUPPORTED), (gather(ks=ints(0, 2, 2, 4)), UNSUPPORTED), (gather(ks=ints(2, 0, 4, 6)), UNSUPPORTED),
                     (gather(ks=ints(0, 1, 2, 3)), UNSUPPORTED), (gather(ks=ints(0, 2, 4), n=3), UNSUPPORTED), (gather(Xh=16), SHAPE),
                     (gather(ks=ints(1, 3, 5, 7), Xh=32, Xw=128), SHAPE), (gather(B=1 << 20, Xh=1 << 12, Xw=1 << 12), SHAPE)):
        assert rc == code, (rc, code, _lib.last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())

    members = torch.zeros(4 * B, C, 128, 128, dtype=torch.float32, device="cuda")
    res = torch.full((B, h, w, C), POISON, dtype=torch.uint8, device="cuda")
    E, O = ints(0, 2, 4, 6), ints(1, 3, 5, 7)

    def merge(even=members.data_ptr(), kse=E, ne=4, odd=members.data_ptr(), kso=O, no=4, out=res.data_ptr(), swap=0, B=B, C=C, h=h, w=w, X=128):
        return lib.uf_tta_merge(even, kse, ne, X, X, odd, kso, no, X, X, out, 1, 1, swap, 1, B, C, h, w, None)

    for rc, code in ((merge(even=None), NULL), (merge(kso=None), NULL), (merge(C=5), UNSUPPORTED), (merge(C=2, swap=1), UNSUPPORTED),
                     (merge(kse=ints(0, 2, 4, 8)), UNSUPPORTED), (merge(kso=ints(1, 3, 3, 7)), UNSUPPORTED), (merge(kso=ints(3, 1, 5, 7)), UNSUPPORTED),
                     (merge(kse=ints(0, 2, 3, 6)), UNSUPPORTED), (merge(ne=2, no=1), UNSUPPORTED), (merge(no=0, odd=None, ne=3), UNSUPPORTED),
                     (merge(X=32), SHAPE), (merge(B=1 << 18, X=1 << 12), SHAPE)):
        assert rc == code, (rc, code, _lib.last_error())
    assert merge(out=None) == NULL
    torch.cuda.synchronize()
    assert bool((res == POISON).all())


# ---------------------------------------------------------------------------------------------------------------------------
# composition with a model
# ---------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the model (and the workspaces it keeps per stream) goes when the module is done: later modules hold the device memory they measure to a cap"""
    yield
    import gc
    _MODELS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def tiny(dtype):
    """the tiny32 model of tests/test_gpu_frames.py"""
    from uformer_amd import model
    if dtype not in _MODELS:
        cfg = spec.arch_config("tiny32", img_size=128)
        m = model.Uformer(img_size=cfg.img_size, in_chans=cfg.in_chans, dd_in=cfg.dd_in, embed_dim=cfg.embed_dim, depths=list(cfg.depths),
                          num_heads=list(cfg.num_heads), modulator=cfg.modulator, compute_dtype=dtype).eval()
        m.load_state_dict(spec.synth_state_dict(cfg, 5), strict=True)
        _MODELS[dtype] = m.cuda()
    return _MODELS[dtype]


def natural_frames(B, h, w, C, seed):
    """smooth uint8 frames (B,h,w,C): the synthetic test image of the project, quantised"""
    x = spec.synth_input(B, h, w, seed, channels=C).clamp(0, 1)
    return np.ascontiguousarray((x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy())


CASES = [(100, 70, "square"), (100, 200, "rect")]


@pytest.mark.parametrize("h,w,canvas", CASES)
def test_restore_ensemble_is_the_restated_merge_of_the_same_model_calls(h, w, canvas):
    from uformer_amd import infer
    m = tiny(torch.bfloat16)
    img = torch.from_numpy(natural_frames(2, h, w, 3, seed=h).astype(np.float32) / FC.F255).permute(0, 3, 1, 2).contiguous().cuda()
    for members, max_batch in ((8, 16), (8, 4), (4, 8), (2, 2), (1, 8)):
        fed, given = [], []

        def recording(x):
            fed.append(x.clone())
            given.append(m(x))
            return given[-1]

        got = infer.restore_ensemble(recording, img, canvas=canvas, members=members, max_batch=max_batch)
        ks = TC.MEMBERS[members]
        order = [k for k in ks if k % 2 == 0] + [k for k in ks if k % 2]              # [0,2,4,6,1,3,5,7]: the batch order, one canvas shape after the other
        per = max(1, max_batch // 2)
        shapes = [TC.canvas_of(h, w, canvas, k) for k in order]
        # the member batch assembled with torch ops, cut where the canvas shape changes and every `per` members
        want_fed, at = [], 0
        while at < len(order):
            run = [k for k in order[at:] if TC.canvas_of(h, w, canvas, k) == shapes[at]]
            run = order[at:at + len(run)]
            for j in range(0, len(run), per):
                want_fed.append(TC.member_batch(img, run[j:j + per], *shapes[at]))
            at += len(run)
        assert len(fed) == len(want_fed) and all(torch.equal(a, b) for a, b in zip(fed, want_fed)), (members, max_batch, [tuple(f.shape) for f in fed])
        outs = torch.cat([g.float().flatten(1) for g in given], 0)                     # (len(order) * 2, C * Xh * Xw): one row per member image
        outputs = {k: outs[i * 2:(i + 1) * 2].view(2, -1, *shapes[i]) for i, k in enumerate(order)}
        want = torch.clamp(TC.merge(outputs, h, w), 0, 1)
        assert torch.equal(got, want), (members, max_batch)
        assert torch.equal(infer.restore_ensemble(m, img, canvas=canvas, members=members, max_batch=max_batch, clamp=False), TC.merge(outputs, h, w))
    one = infer.restore(m, img, canvas=canvas)
    assert torch.equal(infer.restore_ensemble(m, img, canvas=canvas, members=1), one)
    full = infer.restore_ensemble(m, img, canvas=canvas)
    diff = (full - one).abs().max().item()
    print(f"ensemble vs single {h}x{w} {canvas}: max abs difference {diff:.3e}")
    assert diff > 0, "the network is not equivariant: the ensemble is not the single restoration"


@pytest.mark.parametrize("h,w,canvas", CASES)
def test_a_per_pixel_model_gets_restore_back_bit_for_bit(h, w, canvas):
    from uformer_amd import infer
    img = (torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(w)) * 1.2 - 0.1).cuda()
    for clamp in (True, False):
        one = infer.restore(TC.per_pixel, img, canvas=canvas, clamp=clamp)
        for n in (8, 4, 2, 1):
            assert torch.equal(infer.restore_ensemble(TC.per_pixel, img, canvas=canvas, members=n, clamp=clamp), one), (n, clamp)
    assert torch.equal(infer.restore(TC.per_pixel, img, canvas=canvas, clamp=False), TC.per_pixel(img))


@pytest.mark.parametrize("h,w,canvas", CASES)
def test_restore_frames_ensemble_is_the_quantised_restore_ensemble(h, w, canvas):
    from uformer_amd import infer
    m = tiny(torch.bfloat16)
    f = natural_frames(2, h, w, 3, seed=h + 3)
    for bgr in (False, True):
        planes = torch.from_numpy(FC.frames_as_planes(f, True, bgr).astype(np.float32) / FC.F255).cuda()
        for members in (8, 4):
            restored = infer.restore_ensemble(m, planes, canvas=canvas, members=members, clamp=False).cpu().numpy()
            for hwc in (True, False):
                fin = f if hwc else np.ascontiguousarray(f.transpose(0, 3, 1, 2))
                got = infer.restore_frames(m, torch.from_numpy(fin).cuda(), canvas=canvas, hwc=hwc, bgr=bgr, ensemble=members)
                want = FC.planes_as_frames(FC.quantise_ref(restored), hwc, bgr)
                assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
                assert np.array_equal(got.cpu().numpy(), want), (bgr, members, hwc)
    assert len(np.unique(want)) > 16, "the restored frames are images, not a constant"
    plain = infer.restore_frames(m, torch.from_numpy(f).cuda(), canvas=canvas)
    assert torch.equal(infer.restore_frames(m, torch.from_numpy(f).cuda(), canvas=canvas, ensemble=1), plain)
    assert not torch.equal(infer.restore_frames(m, torch.from_numpy(f).cuda(), canvas=canvas, ensemble=8), plain)


def test_frame_restorer_ensemble_matches_the_synchronous_call_with_frames_in_flight():
    from uformer_amd import infer
    m = tiny(torch.bfloat16)
    h, w = 100, 200
    frames = [natural_frames(1, h, w, 3, seed=300 + i) for i in range(6)]
    want = [infer.restore_frames(m, torch.from_numpy(f).cuda(), canvas="rect", ensemble=8).cpu().numpy() for f in frames]
    assert not np.array_equal(want[0], want[1])
    r = infer.FrameRestorer(m, (h, w, 3), depth=3, canvas="rect", ensemble=8)
    t0, t1, t2 = r.submit(frames[0]), r.submit(frames[1]), r.submit(frames[2])         # three frames in flight
    got = {2: t2.result(), 0: t0.result(), 1: t1.result()}
    for i, y in enumerate(r.map(frames[3:]), start=3):
        got[i] = y
    for i in range(6):
        assert got[i].dtype == np.uint8 and np.array_equal(got[i], want[i]), i
    r.close()
