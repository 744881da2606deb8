"""uint8 frame conversion, tile gather and tile blend (uf_frames.hip) restated in numpy: the references tests/test_frames.py pins on the CPU and
tests/test_gpu_frames.py compares the kernels with.  Importable without a GPU."""
import numpy as np

F255 = np.float32(255)

# (h, w, tile, min_overlap) of the blend tests
BLEND_CASES = [(200, 300, 128, 32),        # two by three tiles
               (128, 300, 128, 64),        # one axis has a single tile
               (130, 130, 128, 126),       # two tiles that share all but two columns
               (300, 300, 128, 96),        # seven starts per axis, up to five tiles over one pixel
               (100, 300, 128, 32)]        # the far side is padded


def quantise_ref(v):
    """img_as_ubyte(clamp(v, 0, 1)) for float32: rint of the FLOAT32 product with 255 (ties to even); NaN gives 0 by definition"""
    v = np.asarray(v, dtype=np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    c = np.minimum(np.maximum(v, np.float32(0)), np.float32(1)).astype(np.float32)
    return np.rint(c * F255).astype(np.uint8)


def tie_candidates():
    """float32((k + 0.5) / 255) and its two float32 neighbours, k = 0 ... 254: 765 values around the rounding ties"""
    mid = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    return np.stack([np.nextafter(mid, np.float32(-1)), mid, np.nextafter(mid, np.float32(2))], 1).reshape(-1).astype(np.float32)


def hard_values():
    """the tie candidates, signed zero, negatives, values above 1, infinities, NaN and denormals"""
    tiny = np.float32(1e-45)
    special = np.array([-0.0, 0.0, -1e-3, -1.0, -3e38, 1.0, 1.0000001, 1.5, 3e38, np.inf, -np.inf, np.nan, tiny, -tiny, 1e-39, -1e-39, 0.5, 0.25], dtype=np.float32)
    return np.concatenate([tie_candidates(), special])


def frames_as_planes(frames, hwc, swap_rb):
    """u8 / float frames (B,h,w,C) or (B,C,h,w) -> planes (B,C,h,w) in the model's channel order"""
    p = np.transpose(frames, (0, 3, 1, 2)) if hwc else frames
    if swap_rb:
        idx = list(range(p.shape[1]))
        idx[0], idx[2] = 2, 0
        p = p[:, idx]
    return np.ascontiguousarray(p)


def planes_as_frames(planes, hwc, swap_rb):
    """the inverse of frames_as_planes (the channel exchange is its own inverse)"""
    if swap_rb:
        idx = list(range(planes.shape[1]))
        idx[0], idx[2] = 2, 0
        planes = planes[:, idx]
    return np.ascontiguousarray(np.transpose(planes, (0, 2, 3, 1)) if hwc else planes)


def gather_ref(planes, ys, xs, tile):
    """restore_tiled's tile batch: (len(ys) * len(xs) * B, C, tile, tile), entry k * B + b = frame b from job k, zero beyond the frame"""
    B, C, h, w = planes.shape
    out = np.zeros((len(ys) * len(xs) * B, C, tile, tile), dtype=planes.dtype)
    for k, (y, x) in enumerate((y, x) for y in ys for x in xs):
        th, tw = min(tile, h - y), min(tile, w - x)
        out[k * B:(k + 1) * B, :, :th, :tw] = planes[:, :, y:y + th, x:x + tw]
    return out


def axis_weights(starts, i, n, tile):
    """restore_tiled.ramp in closed form, float64: the weights of tile i over its min(tile, n - start) columns"""
    start = starts[i]
    size = min(tile, n - start)
    wgt = np.ones(size, dtype=np.float64)
    if i > 0:
        ov = starts[i - 1] + tile - start
        if ov > 0:
            wgt[:ov] = (np.arange(ov) + 0.5) / ov
    if i + 1 < len(starts):
        ov = start + tile - starts[i + 1]
        if ov > 0:
            wgt[size - ov:size] *= 1 - (np.arange(ov) + 0.5) / ov
    return wgt


def blend_ref(tiles_out, ys, xs, h, w, tile):
    """sum_t w_t o_t / sum_t w_t over ALL tiles that cover a pixel, float64; tiles_out (len(ys) * len(xs) * B, C, tile, tile)"""
    tiles_out = np.asarray(tiles_out, dtype=np.float64)
    B = tiles_out.shape[0] // (len(ys) * len(xs))
    num = np.zeros((B, tiles_out.shape[1], h, w), dtype=np.float64)
    den = np.zeros((h, w), dtype=np.float64)
    for iy, y in enumerate(ys):
        wy = axis_weights(ys, iy, h, tile)
        for ix, x in enumerate(xs):
            wx = axis_weights(xs, ix, w, tile)
            k = iy * len(xs) + ix
            wgt = wy[:, None] * wx[None, :]
            th, tw = wgt.shape
            num[:, :, y:y + th, x:x + tw] += tiles_out[k * B:(k + 1) * B, :, :th, :tw] * wgt
            den[y:y + th, x:x + tw] += wgt
    return num / den


def near_half_level(ref, eps=1e-3):
    """pixels of a float64 reference whose 255-fold lies within eps of a half level: there a float32 blend may round the other way"""
    s = np.clip(ref, 0.0, 1.0) * 255.0
    return np.abs(s - np.floor(s) - 0.5) <= eps


def quantise_f64(ref):
    return np.rint(np.clip(ref, 0.0, 1.0) * 255.0).astype(np.uint8)


def blend_inputs(h, w, tile, min_overlap, B=2, C=3, seed=0):
    """seeded synthetic tile outputs in [-0.1, 1.1] for a blend case, with the starts: (tiles_out float32, ys, xs)"""
    from uformer_amd import infer
    ys, xs = infer._starts(h, tile, min_overlap), infer._starts(w, tile, min_overlap)
    rng = np.random.default_rng(1000 + seed)
    t = rng.random((len(ys) * len(xs) * B, C, tile, tile), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    return t, ys, xs
