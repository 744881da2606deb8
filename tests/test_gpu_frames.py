"""GPU: uint8 frames end to end (uf_frames.hip, infer.restore_frames, infer.FrameRestorer).

  * the conversion kernels, exact: uf_frames_to_canvas == uf_expand_canvas of the float frames, uf_canvas_to_frames == the numpy quantiser on hard
    inputs, the round trip is the identity -- inside NaN / 0xA5-filled buffers with guard regions, at odd sizes, offsets and alignments;
  * uf_tiles_blend against the float64 restatement (tests/frames_cases.py, pinned against restore_tiled by tests/test_frames.py) on synthetic tiles;
  * restore_frames == quantiser(infer.restore) bit for bit on a small model, the tiled route against restore_tiled;
  * FrameRestorer == the synchronous restore_frames with several frames in flight."""
import math

import numpy as np
import pytest
import torch

import frames_cases as FC
from uformer_amd import spec

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 13), (130, 257)]
POISON = 0xA5


def canvases(h, w):
    X = int(math.ceil(max(h, w) / 128.0) * 128)
    return [(h, w), (X, X), (int(math.ceil(h / 128.0) * 128), int(math.ceil(w / 128.0) * 128) + 128)]     # the image itself, square, rect (wider than tall)


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
    n = B * C * h * w
    rng = np.random.default_rng(seed)
    v = np.resize(np.arange(256, dtype=np.uint8), n)
    rng.shuffle(v)
    return v.reshape((B, h, w, C) if hwc else (B, C, h, w))


def swaps(C):
    return (False, True) if C >= 3 else (False,)


@pytest.mark.parametrize("h,w", SHAPES)
def test_frames_to_canvas_is_expand_canvas_of_the_float_frames(h, w):
    from uformer_amd import ops
    for C in (1, 3, 4, 6):
        for B in (1, 3):
            for hwc in (True, False):
                for swap in swaps(C):
                    f = u8_frames(B, C, h, w, hwc, seed=C * 10 + B)
                    planes = torch.from_numpy(FC.frames_as_planes(f, hwc, swap).astype(np.float32) / FC.F255).cuda()
                    g_in = 61 if B == 3 else 64                                        # a frame pointer that is not 16-byte aligned
                    fin, fin_whole = guarded(f.shape, torch.uint8, g_in, POISON)
                    fin.copy_(torch.from_numpy(f))
                    for (Xh, Xw) in canvases(h, w):
                        want, want_mask = ops.expand_canvas(planes, Xh, Xw, with_mask=True)
                        g_out = 63 if (B == 3 and hwc) else 64                         # ... and a canvas pointer that is not
                        canvas, c_whole = guarded((B, C, Xh, Xw), torch.float32, g_out, float("nan"))
                        mask, m_whole = guarded((B, 1, Xh, Xw), torch.float32, g_out, float("nan"))
                        ops._launch("uf_frames_to_canvas", fin.device, fin, int(hwc), int(swap), canvas, mask, B, C, h, w, Xh, Xw)
                        tag = (C, B, hwc, swap, Xh, Xw)
                        assert torch.equal(canvas, want), tag
                        assert torch.equal(mask, want_mask), tag
                        assert guards_intact(c_whole, g_out, float("nan")) and guards_intact(m_whole, g_out, float("nan")), tag
                        assert guards_intact(fin_whole, g_in, POISON) and torch.equal(fin.cpu(), torch.from_numpy(f)), tag
                    got, none = ops.frames_to_canvas(fin, *canvases(h, w)[1], hwc=hwc, swap_rb=swap)                 # the wrapper, no mask
                    assert none is None and torch.equal(got, ops.expand_canvas(planes, *canvases(h, w)[1], with_mask=False)[0])


@pytest.mark.parametrize("h,w", SHAPES)
def test_canvas_to_frames_is_the_numpy_quantiser_on_hard_inputs(h, w):
    from uformer_amd import ops
    pool = np.concatenate([FC.hard_values(), np.random.default_rng(5).random(3000, dtype=np.float32) * np.float32(1.4) - np.float32(0.2)])
    for C in (1, 3, 4):
        for B in (1, 3):
            for (Xh, Xw) in canvases(h, w):
                y0, x0 = (Xh - h) // 2, (Xw - w) // 2
                g_c = 63 if B == 3 else 64
                canvas, c_whole = guarded((B, C, Xh, Xw), torch.float32, g_c, float("nan"))          # NaN around the image: a misplaced read shows
                region = np.resize(np.roll(pool, 7 * C + B), B * C * h * w).reshape(B, C, h, w).astype(np.float32)
                canvas[:, :, y0:y0 + h, x0:x0 + w] = torch.from_numpy(region).cuda()
                before = c_whole.clone()
                for hwc in (True, False):
                    for swap in swaps(C):
                        want = FC.planes_as_frames(FC.quantise_ref(region), hwc, swap)
                        g_f = 61 if (B == 3 or hwc) else 64
                        frames, f_whole = guarded(want.shape, torch.uint8, g_f, POISON)
                        ops._launch("uf_canvas_to_frames", canvas.device, canvas, frames, int(hwc), int(swap), B, C, h, w, Xh, Xw)
                        tag = (C, B, hwc, swap, Xh, Xw)
                        got = frames.cpu().numpy()
                        assert np.array_equal(got, want), (tag, int((got != want).sum()))
                        assert guards_intact(f_whole, g_f, POISON), tag
                        assert torch.equal(ops.canvas_to_frames(canvas, h, w, hwc=hwc, swap_rb=swap).cpu(), torch.from_numpy(want)), tag
                assert torch.equal(c_whole.view(torch.int32), before.view(torch.int32)), "the canvas is only read"
    if (h, w) == SHAPES[-1]:
        assert region.size >= FC.hard_values().size, "the largest shape holds every hard value"


@pytest.mark.parametrize("h,w", SHAPES)
def test_round_trip_is_the_identity(h, w):
    from uformer_amd import ops
    for C in (1, 3, 4):
        for hwc in (True, False):
            for swap in swaps(C):
                f = torch.from_numpy(u8_frames(3, C, h, w, hwc, seed=C)).cuda()
                for (Xh, Xw) in canvases(h, w):
                    canvas, _ = ops.frames_to_canvas(f, Xh, Xw, hwc=hwc, swap_rb=swap)
                    assert torch.equal(ops.canvas_to_frames(canvas, h, w, hwc=hwc, swap_rb=swap), f), (C, hwc, swap, Xh, Xw)


def test_tiles_gather_is_the_tile_batch_with_zeros_beyond_the_frame():
    from uformer_amd import infer, ops
    for (h, w, tile, ov) in FC.BLEND_CASES:
        ys, xs = infer._starts(h, tile, ov), infer._starts(w, tile, ov)
        origins = torch.tensor([(y, x) for y in ys for x in xs], dtype=torch.int32).cuda()
        for C, hwc, swap in ((3, True, False), (3, True, True), (1, False, False), (6, False, True), (4, True, True)):
            f = u8_frames(2, C, h, w, hwc, seed=h + C)
            planes = FC.frames_as_planes(f, hwc, swap).astype(np.float32) / FC.F255
            want = torch.from_numpy(FC.gather_ref(planes, ys, xs, tile))
            assert torch.equal(ops.tiles_gather(torch.from_numpy(f).cuda(), origins, tile, hwc=hwc, swap_rb=swap).cpu(), want), (h, w, C, hwc, swap)
            ff = torch.from_numpy(f.astype(np.float32) / FC.F255).cuda()                                           # float32 frames, same layout
            assert torch.equal(ops.tiles_gather(ff, origins, tile, hwc=hwc, swap_rb=swap).cpu(), want), (h, w, C, hwc, swap, "f32")


@pytest.mark.parametrize("case", range(len(FC.BLEND_CASES)))
def test_tiles_blend_vs_float64_restatement(case):
    """f32 output: max |got - ref| <= 2e-6 (the bound the project holds tile mechanics to).  u8 output: equal to the quantised reference wherever
    255 ref is farther than 1e-3 from a half level, at most one level off elsewhere; the excluded share is capped at 1 % (expected ~0.2 %)."""
    from uformer_amd import ops
    h, w, tile, ov = FC.BLEND_CASES[case]
    t, ys, xs = FC.blend_inputs(h, w, tile, ov, seed=case)
    ref = FC.blend_ref(t, ys, xs, h, w, tile)
    tiles, t_whole = guarded(t.shape, torch.float32, 64, float("nan"))
    tiles.copy_(torch.from_numpy(t))
    out, o_whole = guarded(ref.shape, torch.float32, 61, float("nan"))
    assert ops.tiles_blend(tiles, ys, xs, h, w, u8=False, clamp=False, out=out) is out
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    print(f"tiles_blend {FC.BLEND_CASES[case]}: f32 max abs err {err:.3e}")
    assert err <= 2e-6 and guards_intact(o_whole, 61, float("nan"))
    clamped = ops.tiles_blend(tiles, ys, xs, h, w, u8=False, clamp=True)
    assert torch.equal(clamped, out.clamp(0, 1))
    near = FC.near_half_level(ref)
    assert near.mean() <= 0.01
    q = FC.quantise_f64(ref)
    for hwc in (True, False):
        for swap in (False, True):
            want = FC.planes_as_frames(q, hwc, swap)
            loose = FC.planes_as_frames(near, hwc, swap)
            frames, f_whole = guarded(want.shape, torch.uint8, 61, POISON)
            ops.tiles_blend(tiles, ys, xs, h, w, u8=True, hwc=hwc, swap_rb=swap, out=frames)
            got = frames.cpu().numpy()
            assert np.array_equal(got[~loose], want[~loose]), (hwc, swap, int((got != want)[~loose].sum()))
            assert np.abs(got.astype(np.int16) - want.astype(np.int16)).max() <= 1
            assert guards_intact(f_whole, 61, POISON)
    assert guards_intact(t_whole, 64, float("nan"))


# ---------------------------------------------------------------------------------------------------------------------------
# composition with a model
# ---------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the models (and the workspaces they keep per stream) go when the module is done: later modules hold the device memory they measure to a cap"""
    yield
    import gc
    from uformer_amd import infer
    _MODELS.clear()
    infer._ORIGINS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def tiny(dd_in, in_chans, dtype):
    import dataclasses
    from uformer_amd import model
    key = (dd_in, in_chans, dtype)
    if key not in _MODELS:
        cfg = dataclasses.replace(spec.arch_config("tiny32", img_size=128), dd_in=dd_in, in_chans=in_chans)
        m = model.Uformer(img_size=cfg.img_size, in_chans=cfg.in_chans, dd_in=cfg.dd_in, embed_dim=cfg.embed_dim, depths=list(cfg.depths),
                          num_heads=list(cfg.num_heads), modulator=cfg.modulator, compute_dtype=dtype).eval()
        m.load_state_dict(spec.synth_state_dict(cfg, 5), strict=True)
        _MODELS[key] = m.cuda()
    return _MODELS[key]


def natural_frames(B, h, w, C, seed):
    """smooth uint8 frames (B,h,w,C): the synthetic test image of the project, quantised"""
    x = spec.synth_input(B, h, w, seed, channels=C).clamp(0, 1)
    return np.ascontiguousarray((x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("h,w", [(72, 136), (100, 200)])
def test_restore_frames_is_the_quantised_restore(h, w, dtype):
    from uformer_amd import infer
    for (dd_in, in_chans, bgr) in ((3, 3, False), (3, 3, True), (1, 1, False), (6, 3, False)):
        m = tiny(dd_in, in_chans, dtype)
        f = natural_frames(2, h, w, dd_in, seed=h + dd_in)                                                         # (B,h,w,C)
        planes = torch.from_numpy(FC.frames_as_planes(f, True, bgr).astype(np.float32) / FC.F255).cuda()
        for canvas in ("square", "rect"):
            restored = infer.restore(m, planes, canvas=canvas).cpu().numpy()
            for hwc in (True, False):
                fin = f if hwc else np.ascontiguousarray(f.transpose(0, 3, 1, 2))
                got = infer.restore_frames(m, torch.from_numpy(fin).cuda(), canvas=canvas, hwc=hwc, bgr=bgr)
                want = FC.planes_as_frames(FC.quantise_ref(restored), hwc, bgr)
                assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
                assert np.array_equal(got.cpu().numpy(), want), (dd_in, in_chans, bgr, canvas, hwc)
        assert len(np.unique(want)) > 16, "the restored frames are images, not a constant"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_restore_frames_tiled_route_is_restore_tiled(dtype):
    from uformer_amd import infer, ops
    h, w, tile, ov = 200, 300, 128, 32
    m = tiny(3, 3, dtype)
    f = natural_frames(2, h, w, 3, seed=9)
    fd = torch.from_numpy(f).cuda()
    planes = torch.from_numpy(FC.frames_as_planes(f, True, False).astype(np.float32) / FC.F255).cuda()
    fed, given = [], []

    def recording(x):
        fed.append(x.clone())
        given.append(m(x))
        return given[-1]

    ref = infer.restore_tiled(recording, planes, tile=tile, min_overlap=ov)
    ys, xs = infer._starts(h, tile, ov), infer._starts(w, tile, ov)
    origins = torch.tensor([(y, x) for y in ys for x in xs], dtype=torch.int32).cuda()
    assert torch.equal(ops.tiles_gather(fd, origins, tile, hwc=True), torch.cat(fed, 0))
    outs = torch.cat(given, 0)
    blended = ops.tiles_blend(outs, ys, xs, h, w, u8=False, clamp=True)
    err = (blended - ref).abs().max().item()
    print(f"tiled route {dtype}: f32 blend vs restore_tiled {err:.3e}")
    assert err <= 2e-6
    got = infer.restore_frames(m, fd, tile=tile, min_overlap=ov)
    assert torch.equal(got, ops.tiles_blend(outs, ys, xs, h, w, u8=True, hwc=True))                                  # the same tiles through the same blend
    want = FC.quantise_ref(ref.cpu().numpy()).transpose(0, 2, 3, 1)
    assert np.abs(got.cpu().numpy().astype(np.int16) - want.astype(np.int16)).max() <= 1
    # a frame that fits one tile takes the canvas route, as restore_tiled falls back to restore
    small = torch.from_numpy(natural_frames(1, 100, 120, 3, seed=2)).cuda()
    assert torch.equal(infer.restore_frames(m, small, tile=128, canvas="rect"), infer.restore_frames(m, small, canvas="square"))


# ---------------------------------------------------------------------------------------------------------------------------
# FrameRestorer
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 2])
def test_frame_restorer_matches_the_synchronous_path_with_frames_in_flight(batch):
    from uformer_amd import infer
    m = tiny(3, 3, torch.bfloat16)
    h, w = 72, 136
    frames = [natural_frames(batch, h, w, 3, seed=100 + i) for i in range(10)]
    want = [infer.restore_frames(m, torch.from_numpy(f).cuda(), canvas="rect").cpu().numpy() for f in frames]
    assert not np.array_equal(want[0], want[1])
    r = infer.FrameRestorer(m, (h, w, 3), batch=batch, depth=3, canvas="rect")
    t0, t1, t2 = r.submit(frames[0]), r.submit(frames[1]), r.submit(frames[2])
    with pytest.raises(RuntimeError, match="not consumed"):
        r.submit(frames[3])                                                            # its slot still holds frame 0
    pins = [(s["pin_in"].data_ptr(), s["pin_out"].data_ptr(), s["dev_in"].data_ptr(), s["dev_out"].data_ptr()) for s in r._slots]
    assert all(s["pin_in"].is_pinned() and s["pin_out"].is_pinned() for s in r._slots)
    got = {2: t2.result(), 0: t0.result()}                                             # out of order
    view1 = t1.result(copy=False)
    assert np.array_equal(view1, want[1])
    with pytest.raises(RuntimeError, match="consumed"):
        t0.result()
    kept = got[0]
    got[1] = view1.copy()
    pending = {}
    for i in range(3, 10):
        pending[i] = r.submit(frames[i])                                               # reuses the slots of frames i - 3
        if len(pending) == 3:
            for j in sorted(pending, reverse=True):                                    # newest first
                got[j] = pending.pop(j).result()
    for j in sorted(pending):
        got[j] = pending.pop(j).result()
    for i in range(10):
        assert isinstance(got[i], np.ndarray) and got[i].dtype == np.uint8 and np.array_equal(got[i], want[i]), i
    assert np.array_equal(kept, want[0]), "a copy survives the reuse of its slot"
    assert pins == [(s["pin_in"].data_ptr(), s["pin_out"].data_ptr(), s["dev_in"].data_ptr(), s["dev_out"].data_ptr()) for s in r._slots], "steady state allocates nothing"
    # map: in order, depth in flight; CPU tensors come back as tensors; the unbatched form at batch 1
    mapped = list(r.map(torch.from_numpy(f) for f in frames[:5]))
    assert all(isinstance(y, torch.Tensor) and np.array_equal(y.numpy(), want[i]) for i, y in enumerate(mapped))
    if batch == 1:
        y = r.submit(frames[4][0]).result()
        assert y.shape == (h, w, 3) and np.array_equal(y, want[4][0])
    r.drain()
    r.close()
    with pytest.raises(RuntimeError, match="closed"):
        r.submit(frames[0])


def test_frame_restorer_tiled_and_bgr():
    from uformer_amd import infer
    m = tiny(3, 3, torch.bfloat16)
    h, w = 200, 300
    frames = [natural_frames(1, h, w, 3, seed=200 + i) for i in range(4)]
    kw = dict(tile=128, min_overlap=32, bgr=True)
    want = [infer.restore_frames(m, torch.from_numpy(f).cuda(), **kw).cpu().numpy() for f in frames]
    r = infer.FrameRestorer(m, (h, w, 3), depth=2, **kw)
    for i, y in enumerate(r.map(frames)):
        assert np.array_equal(y, want[i]), i
    r.close()
