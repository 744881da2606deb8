"""Geometric self-ensemble (uf_tta_gather, uf_tta_merge, infer.restore_ensemble) restated in torch: the eight transforms as index maps, their
inverses, the placement on the canvas and the balanced pairwise mean.  Every function computes in the dtype it is given (float64 on the CPU tests,
float32 where the GPU tests want the kernel's own arithmetic).  Importable without a GPU."""
import math

import torch

# image sizes of the GPU tests: one and several LDS tiles of the transposing path, ragged edges, h < w and h > w
SHAPES = [(1, 1), (7, 13), (33, 67), (67, 33), (130, 257)]
MEMBERS = {8: (0, 1, 2, 3, 4, 5, 6, 7), 4: (0, 2, 4, 6), 2: (0, 4), 1: (0,)}
INVERSE = (0, 3, 2, 1, 4, 5, 6, 7)       # T_1 and T_3 undo each other, every other T_k undoes itself
# member(my, mx) = img(sy, sx): even k  sy = FY ? h-1-my : my,  sx = FX ? w-1-mx : mx;   odd k  sy = FY ? h-1-mx : mx,  sx = FX ? w-1-my : my
FY = (0, 1, 1, 0, 1, 1, 0, 0)
FX = (0, 0, 1, 1, 0, 1, 1, 0)


def transform(x, k):
    """T_k of (..., h, w) by its index map: (..., h, w) for even k, (..., w, h) for odd k"""
    h, w = x.shape[-2:]
    sy = torch.arange(h, device=x.device)
    sx = torch.arange(w, device=x.device)
    sy = h - 1 - sy if FY[k] else sy
    sx = w - 1 - sx if FX[k] else sx
    if k % 2 == 0:
        return x[..., sy[:, None], sx[None, :]]
    return x[..., sy[None, :], sx[:, None]]


def inverse(x, k):
    return transform(x, INVERSE[k])


def canvas_of(h, w, canvas, k):
    """(Xh, Xw) of member k of an (h, w) image"""
    if canvas == "square":
        X = int(math.ceil(max(h, w) / 128.0) * 128)
        return X, X
    Xh, Xw = int(math.ceil(h / 128.0) * 128), int(math.ceil(w / 128.0) * 128)
    return (Xw, Xh) if k % 2 else (Xh, Xw)


def place(member, Xh, Xw, fill=0.0):
    """the member centred on an (Xh, Xw) canvas of `fill`"""
    hk, wk = member.shape[-2:]
    out = torch.full(tuple(member.shape[:-2]) + (Xh, Xw), fill, dtype=member.dtype, device=member.device)
    y0, x0 = (Xh - hk) // 2, (Xw - wk) // 2
    out[..., y0:y0 + hk, x0:x0 + wk] = member
    return out


def crop(canvas, hk, wk):
    Xh, Xw = canvas.shape[-2:]
    y0, x0 = (Xh - hk) // 2, (Xw - wk) // 2
    return canvas[..., y0:y0 + hk, x0:x0 + wk]


def member_batch(img, ks, Xh, Xw):
    """(len(ks) * B, C, Xh, Xw): entry m * B + b = place(T_ks[m](img[b]))"""
    return torch.cat([place(transform(img, k), Xh, Xw) for k in ks], 0)


def tree_sum(rs):
    """balanced pairwise sum in the given order: ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) for eight"""
    rs = list(rs)
    assert len(rs) in (1, 2, 4, 8)
    while len(rs) > 1:
        rs = [rs[i] + rs[i + 1] for i in range(0, len(rs), 2)]
    return rs[0]


def merge(outputs, h, w):
    """outputs: {k: (B, C, Xh_k, Xw_k) restored canvas of member k} -> unclamped tree mean (B, C, h, w), in the outputs' dtype"""
    ks = sorted(outputs)
    rs = [inverse(crop(outputs[k], *((w, h) if k % 2 else (h, w))), k) for k in ks]
    return tree_sum(rs) * (1.0 / len(ks))


def ensemble(model, img, canvas="square", members=8):
    """the definition, member by member: unclamped"""
    h, w = img.shape[-2:]
    return merge({k: model(place(transform(img, k), *canvas_of(h, w, canvas, k))) for k in MEMBERS[members]}, h, w)


def single(model, img, canvas="square"):
    h, w = img.shape[-2:]
    return crop(model(place(img, *canvas_of(h, w, canvas, 0))), h, w)


def per_pixel(t):
    """a model that acts on every pixel by itself"""
    return 0.5 * t + 0.125 * t * t + 0.1
