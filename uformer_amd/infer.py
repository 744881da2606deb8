"""Arbitrary-resolution inference.

``restore``: exactly the steps the reference's evaluation scripts put around ``Uformer.forward`` -- ``expand2square`` to a square
multiple of 128 (test/test_sidd.py:79-92), forward, ``masked_select`` crop, clamp (:106-109; test/test_gopro_hide.py:77-103) -- with
the pad and the crop + clamp each ONE kernel on the device (``uf_expand2square``, ``uf_crop_clamp``); parity-exact with the
reference pipeline.  ``restore(..., canvas="rect")`` pads each side to its own multiple of 128 instead (``uf_expand_canvas``,
``uf_crop_clamp_canvas``): less padding, but not the reference's protocol.

``restore_tiled``: a capability the reference does not have.  A 1280x720 frame padded to 1280x1280 computes 1.78x the pixels it
needs; here the frame is covered by overlapping SQUARE tiles (multiples of 128) that are restored
independently -- as one batch -- and cross-faded over the overlap.  It is an approximation of the full-frame result (a tile's
border pixels see zero padding / a cut context instead of the neighbouring image), which is why it is opt-in and why the overlap is
wide; ``restore`` stays the reference-exact path.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import torch

from . import ops

Tensor = torch.Tensor


def expand2square(timg: Tensor, factor: float = 128.0) -> Tuple[Tensor, Tensor]:
    """(B,C,h,w) -> zero canvas (B,C,X,X) with the image centred at ((X-h)//2, (X-w)//2), X = max(h,w) rounded up to a
    multiple of ``factor`` (128 = 4 down-samplings x window 8), and the (B,1,X,X) mask of ones over the image: the reference
    helper (written for B = 1) for a batch, one kernel."""
    return ops.expand2square(timg, factor, with_mask=True)


def crop_to_mask(restored: Tensor, h: int, w: int, clamp: bool = False) -> Tensor:
    """Inverse of expand2square for the restored canvas: the (B,C,h,w) region the mask covers
    (``torch.masked_select(restored, mask.bool()).reshape(1,3,h,w)`` in the reference), optionally clamped to [0,1]."""
    return ops.crop_clamp(restored, h, w, clamp)


@torch.no_grad()
def restore(model, img: Tensor, factor: float = 128.0, clamp: bool = True, canvas: str = "square") -> Tensor:
    """Restore images of any (h, w): pad to a canvas of multiples of ``factor``, run ``model``, crop back, clamp to [0,1]
    (test/test_sidd.py:106-109).  ``img``: (B,dd_in,h,w) float32 on the model's device; the result has the model's ``in_chans`` planes.

    ``canvas="square"`` (default): the reference's protocol -- ``expand2square``, one square side X = max(h, w) rounded up to a
    multiple of ``factor``; output identical to the reference pipeline.
    ``canvas="rect"``: each side rounded up to its OWN multiple of ``factor`` (a 720 x 1280 frame runs on 768 x 1280 instead of
    1280 x 1280, 40 % fewer pixels), the image centred the same way on each axis.  This is the reference network's math on a
    different canvas: the convolutions and the windows at the image border see less zero padding, so the output DIFFERS from the
    reference's square-padded result.  The two are equal only when both canvases coincide (e.g. 200 x 136 -> 256 x 256 either way)."""
    if img.dim() != 4:
        raise ValueError(f"restore expects (B,C,h,w), got {tuple(img.shape)}")
    h, w = img.shape[-2:]
    if canvas == "square":
        padded, _ = ops.expand2square(img, factor, with_mask=False)
        return ops.crop_clamp(model(padded), h, w, clamp)
    if canvas == "rect":
        Xh, Xw = int(math.ceil(h / float(factor)) * factor), int(math.ceil(w / float(factor)) * factor)
        padded, _ = ops.expand_canvas(img, Xh, Xw, with_mask=False)
        return ops.crop_clamp_canvas(model(padded), h, w, clamp)
    raise ValueError(f"restore: canvas must be 'square' or 'rect', got {canvas!r}")


def _starts(n: int, tile: int, min_overlap: int) -> List[int]:
    if n <= tile:
        return [0]
    k = max(2, math.ceil((n - min_overlap) / (tile - min_overlap)))
    return sorted({round(i * (n - tile) / (k - 1)) for i in range(k)})


@torch.no_grad()
def restore_tiled(model, img: Tensor, tile: int = 768, min_overlap: int = 128, clamp: bool = True, max_batch: int = 8) -> Tensor:
    """EXPERIMENTAL, beyond the reference (which always pads the whole frame to a square, test/test_sidd.py:106-109): an APPROXIMATION by
    construction -- the network's receptive field spans several hundred pixels, so a tile does not see what the full frame sees.
    The mechanics (cutting, padding, ramps, normalisation) are exact: tests/test_host_logic.py checks them to 2e-6 with a pointwise
    model; against the full-frame result of a real network only a PSNR is reported (tests/test_gpu_tail.py).
    Overlapped-tile restoration of (B,dd_in,h,w) images (the result has the model's ``in_chans`` planes): square ``tile`` x ``tile`` windows (a multiple of 128) at evenly spaced
    positions with at least ``min_overlap`` pixels in common, forwarded in batches of ``max_batch`` tiles, blended with a linear
    ramp across each overlap.  An image that fits one tile takes the reference-exact ``restore`` path."""
    if tile % 128:
        raise ValueError("tile must be a multiple of 128")
    B, C, h, w = img.shape
    if h <= tile and w <= tile:
        return restore(model, img, 128.0, clamp)
    ys, xs = _starts(h, tile, min_overlap), _starts(w, tile, min_overlap)
    acc = None            # (B, in_chans, h, w): sized by the first output, whose plane count is the model's, not the input's
    wsum = torch.zeros((1, 1, h, w), dtype=torch.float32, device=img.device)

    def ramp(n: int, start: int, starts: List[int], size: int) -> Tensor:
        """weight of a tile along one axis: 1 inside, linear ramps over the parts shared with the neighbouring tiles"""
        wgt = torch.ones(size, device=img.device)
        i = starts.index(start)
        if i > 0:
            ov = starts[i - 1] + tile - start
            if ov > 0:
                wgt[:ov] = (torch.arange(ov, device=img.device) + 0.5) / ov
        if i + 1 < len(starts):
            ov = start + tile - starts[i + 1]
            if ov > 0:
                wgt[size - ov:size] = wgt[size - ov:size] * (1 - (torch.arange(ov, device=img.device) + 0.5) / ov)
        return wgt

    jobs = [(y, x) for y in ys for x in xs]
    for j0 in range(0, len(jobs), max(1, max_batch // B)):
        chunk = jobs[j0:j0 + max(1, max_batch // B)]
        tiles = []
        for (y, x) in chunk:
            th, tw = min(tile, h - y), min(tile, w - x)
            t = img[:, :, y:y + th, x:x + tw]
            if th < tile or tw < tile:                       # image smaller than a tile along this axis: zero-pad at the far side
                t = torch.nn.functional.pad(t, (0, tile - tw, 0, tile - th))
            tiles.append(t)
        out = model(torch.cat(tiles, 0).contiguous())
        if acc is None:
            acc = torch.zeros((B, out.shape[1], h, w), dtype=torch.float32, device=img.device)
        for k, (y, x) in enumerate(chunk):
            th, tw = min(tile, h - y), min(tile, w - x)
            wy, wx = ramp(h, y, ys, th), ramp(w, x, xs, tw)
            wgt = (wy[:, None] * wx[None, :])[None, None]
            acc[:, :, y:y + th, x:x + tw] += out[k * B:(k + 1) * B, :, :th, :tw].float() * wgt
            wsum[:, :, y:y + th, x:x + tw] += wgt
    res = acc / wsum
    return torch.clamp(res, 0, 1) if clamp else res


class GraphedForward:
    """Small-batch serving: ``Uformer.forward`` for ONE input shape captured in a HIP graph and replayed.

    The reference's evaluation scripts restore one image per call (test/test_sidd.py:101-107: batch 1), and a forward is ~90 kernel launches:
    at batch 1-4 the launches and the gaps between them are a large part of the step.  ``GraphedForward(model, example)`` runs the forward once
    eagerly on a private stream (packs the weights, allocates that stream's workspace), captures a second run into a ``torch.cuda.CUDAGraph``
    (the library's own side-stream fork / join is followed by the capture, tests/test_gpu_model.py::test_forward_captured_in_a_hip_graph) and
    ``__call__`` copies the new batch into the static input buffer and replays -- bit-identical to the eager forward.  The returned tensor
    is the graph's static output: clone it if it must survive the next call.  Weights are read at replay time (the graph holds
    pointers into the packed-weight buffers): ``__call__`` compares the model's packed-weight cache (keyed by (storage, version) of every parameter) with the one it
    captured and recaptures by itself when the parameters changed; the captured pack is kept alive by this object, so a stale replay can never read freed memory."""

    def __init__(self, model, example: Tensor):
        if not example.is_cuda:
            raise ValueError("GraphedForward needs a CUDA example input")
        self.model = model
        self._x = example.detach().clone()
        self._stream = torch.cuda.Stream(device=example.device)
        self.recapture()

    @torch.no_grad()
    def recapture(self) -> None:
        st = self._stream
        st.wait_stream(torch.cuda.current_stream(self._x.device))
        with torch.cuda.stream(st):
            self.model(self._x)                               # warm-up on the capture stream: packed weights + this stream's workspace
        torch.cuda.current_stream(self._x.device).wait_stream(st)
        torch.cuda.synchronize(self._x.device)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph, stream=st):
            self._y = self.model(self._x)
        # the graph holds raw pointers into THIS pack: keep it alive (an eager forward after a parameter change repacks and would free it under the
        # graph), and remember which pack it is so that __call__ notices the change
        self._captured_pack = self._current_pack()

    def _current_pack(self):
        get = getattr(self.model, "_get_packed", None)
        return get(self._x.device) if get is not None else None

    @torch.no_grad()
    def __call__(self, x: Tensor) -> Tensor:
        if x.shape != self._x.shape or x.dtype != self._x.dtype or x.device != self._x.device:
            raise ValueError(f"GraphedForward was captured for {tuple(self._x.shape)} {self._x.dtype} on {self._x.device}, got {tuple(x.shape)} {x.dtype} on {x.device}")
        if self._current_pack() is not self._captured_pack:
            # parameters changed since the capture (optimizer step, load_state_dict, .to()): _get_packed has just repacked them into NEW buffers, the
            # graph would replay on the old ones and return stale results -- capture again
            self.recapture()
        self._x.copy_(x)
        self._graph.replay()
        return self._y


class PipelinedForward:
    """Throughput serving, beyond the reference (whose scripts restore one batch after the other, test/test_sidd.py:101-107): up to ``depth``
    forwards of successive batches IN FLIGHT at once, each on a stream of its own.

    One forward is a chain of ~90 dependent launches, and the deep stages of a 256 x 256 batch do not fill the chip (Uformer-B at batch 16: 64
    windows in the bottleneck, 256 = one per CU at 32 x 32): with one batch in flight those launches run at the latency of a single window while
    most of the matrix pipes idle.  Batches are independent, so the next batch's high-resolution stages can run beside them.  ``submit(x)``
    enqueues a forward on the next stream of a small ring (ordered behind everything the caller's stream has enqueued so far -- the producer of
    ``x``) and returns a handle; ``handle.result()`` makes the CALLER's stream wait for that forward and returns its output (every handle must be
    consumed).  Results are the
    eager forward's bit for bit (the kernels are batch-size and stream invariant, tests/test_gpu_model.py).  The caller keeps ``x`` alive until
    ``result()``; outputs are fresh tensors.  Parameters must not change while forwards are in flight (the small f32 parameters are read in place,
    and an update enqueued on the caller's stream is not ordered behind the ring streams): consume every handle, or call ``drain()``, first.
    Measured on an MI355X, Uformer-B 256 x 256 bf16 (profiles/r06_run21_pipelined.txt): batch 16: 2419 img/s eager, 2566 with two forwards in flight;
    batch 4: 1190 -> 1836 (2) -> 2177 (3); batch 1: 389 -> 696 (2) -> 945 img/s (3)."""

    class Handle:
        def __init__(self, y: Tensor, ev, stream):
            self._y, self._ev, self._stream = y, ev, stream

        def result(self) -> Tensor:
            cur = torch.cuda.current_stream(self._y.device)
            cur.wait_event(self._ev)
            self._y.record_stream(cur)          # allocated on the ring stream, consumed on the caller's
            return self._y

    def __init__(self, model, depth: int = 2, device=None):
        if depth < 1:
            raise ValueError("depth must be at least 1")
        dev = device if device is not None else next(model.parameters()).device
        self.model, self.depth = model, depth
        self._streams = [torch.cuda.Stream(device=dev) for _ in range(depth)]
        self._k = 0

    @torch.no_grad()
    def submit(self, x: Tensor) -> "PipelinedForward.Handle":
        s = self._streams[self._k % self.depth]
        self._k += 1
        # the operand pack is (re)built HERE, on the caller's stream, which every ring stream waits for -- not inside the forward on one ring stream while
        # the others already read it; the handle keeps the pack it ran on alive (a later repack frees the old buffers only after result())
        get = getattr(self.model, "_get_packed", None)
        pack = get(x.device) if get is not None else None
        s.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(s):
            y = self.model(x)
            ev = torch.cuda.Event()
            ev.record(s)
        x.record_stream(s)
        h = PipelinedForward.Handle(y, ev, s)
        h._pack = pack
        return h

    def drain(self) -> None:
        """the caller's stream waits for every forward submitted so far (before a parameter update, a checkpoint load, ...)"""
        cur = torch.cuda.current_stream(self._streams[0].device)
        for s in self._streams:
            cur.wait_stream(s)

    @torch.no_grad()
    def map(self, batches):
        """Generator: forwards of an iterable of batches, ``depth`` in flight, outputs in order."""
        pending = []
        for x in batches:
            pending.append(self.submit(x))
            if len(pending) >= self.depth:
                yield pending.pop(0).result()
        while pending:
            yield pending.pop(0).result()


# ---------------------------------------------------------------------------------------
# uint8 frames in, uint8 frames out
# ---------------------------------------------------------------------------------------
def _check_frames(frames, hwc: bool, bgr: bool, canvas: str, what: str):
    """(B, C, h, w) of a uint8 frame batch, after the argument checks both frame interfaces share (they run before anything touches a device)"""
    if canvas not in ("square", "rect"):
        raise ValueError(f"{what}: canvas must be 'square' or 'rect', got {canvas!r}")
    if frames.dtype != torch.uint8:
        raise ValueError(f"{what}: frames must be uint8, got {frames.dtype}")
    if frames.dim() != 4:
        raise ValueError(f"{what}: frames must be (B,h,w,C) or (B,C,h,w), got {tuple(frames.shape)}")
    B, a, b, c = frames.shape
    B, C, h, w = (B, c, a, b) if hwc else (B, a, b, c)
    if bgr and C < 3:
        raise ValueError(f"{what}: bgr needs at least 3 channels, the frames have {C}")
    return B, C, h, w


_ORIGINS = {}     # (ys, xs, device) -> int32 (T,2) origins on the device: a handful of frame geometries per process


def _tile_origins(ys, xs, device) -> Tensor:
    key = (tuple(ys), tuple(xs), str(device))
    t = _ORIGINS.get(key)
    if t is None:
        if len(_ORIGINS) >= 64:
            _ORIGINS.clear()
        t = _ORIGINS[key] = torch.tensor([(y, x) for y in ys for x in xs], dtype=torch.int32).to(device)
    return t


# ---------------------------------------------------------------------------------------
# geometric self-ensemble
# ---------------------------------------------------------------------------------------
ENSEMBLE_MEMBERS = {8: (0, 1, 2, 3, 4, 5, 6, 7), 4: (0, 2, 4, 6), 2: (0, 4), 1: (0,)}      # members -> the transforms k of Augment_RGB_torch


def _check_ensemble(members, canvas: str, what: str, name: str = "members"):
    if canvas not in ("square", "rect"):
        raise ValueError(f"{what}: canvas must be 'square' or 'rect', got {canvas!r}")
    if isinstance(members, bool) or members not in ENSEMBLE_MEMBERS:
        raise ValueError(f"{what}: {name} must be 8, 4, 2 or 1, got {members!r}")
    ks = ENSEMBLE_MEMBERS[members]
    return [k for k in ks if k % 2 == 0], [k for k in ks if k % 2]


def _ensemble_members(model, src: Tensor, B: int, h: int, w: int, canvas: str, even, odd, max_batch: int, hwc: bool, swap_rb: bool):
    """The restored members of ``src`` (f32 planes or uint8 frames): (even-k outputs, odd-k outputs or None).  One input buffer per canvas shape --
    on the square canvas both parities share it, in the order [0,2,4,6,1,3,5,7] -- filled by one ``uf_tta_gather`` per parity and forwarded
    ``max(1, max_batch // B)`` members at a time into one output buffer; a buffer that fits one forward is the model's output itself."""
    per = max(1, int(max_batch) // B)
    if canvas == "square":
        X = int(math.ceil(max(h, w) / 128.0) * 128)
        classes = [((X, X), [l for l in (even, odd) if l])]
    else:
        Xh, Xw = int(math.ceil(h / 128.0) * 128), int(math.ceil(w / 128.0) * 128)
        classes = [((Xh, Xw), [even])] + ([((Xw, Xh), [odd])] if odd else [])
    outs = []
    for (Xa, Xb), lists in classes:
        nm, x, m0 = sum(len(l) for l in lists), None, 0
        for l in lists:
            if x is None and len(l) == nm:
                x = ops.tta_gather(src, l, Xa, Xb, hwc, swap_rb)
            else:
                if x is None:
                    x = torch.empty((nm * B, src.shape[3] if hwc else src.shape[1], Xa, Xb), dtype=torch.float32, device=src.device)
                ops.tta_gather(src, l, Xa, Xb, hwc, swap_rb, out=x[m0 * B:(m0 + len(l)) * B])
            m0 += len(l)
        if nm <= per:
            y = model(x)
        else:
            y = None                                                 # (nm*B, in_chans, Xa, Xb): sized by the first output
            for j0 in range(0, nm, per):
                j1 = min(nm, j0 + per)
                o = model(x[j0 * B:j1 * B])
                if y is None:
                    y = torch.empty((nm * B,) + tuple(o.shape[1:]), dtype=torch.float32, device=src.device)
                y[j0 * B:j1 * B].copy_(o)
        m0 = 0
        for l in lists:
            outs.append(y[m0 * B:(m0 + len(l)) * B])
            m0 += len(l)
    return outs[0], (outs[1] if odd else None)


@torch.no_grad()
def restore_ensemble(model, img: Tensor, canvas: str = "square", clamp: bool = True, members: int = 8, max_batch: int = 8) -> Tensor:
    """Geometric self-ensemble, beyond the reference (the "+" variant of restoration papers): ``img`` (B,dd_in,h,w) float32 (any other dtype is converted to float32 first, as ``restore`` converts it) is restored under
    ``members`` of the eight flips and rotations ``T_k`` = ``Augment_RGB_torch.transform<k>`` (utils/dataset_utils.py:8-33) -- 8: all; 4: k = 0, 2,
    4, 6 (no transposed canvas); 2: k = 0, 4; 1: ``restore`` itself -- each result is turned back and the mean is clamped to [0,1]:
    ``clamp01(tree_sum_k T_k^-1(crop(model(pad(T_k(img))))) / n)``, the sum taken pairwise in ascending k in f32 (a model that acts per pixel gets
    its single result back bit for bit).  ``pad`` / ``crop`` are ``restore``'s for the member's own size; on ``canvas="rect"`` the odd members run
    on the swapped canvas.  The members are a batch: one ``uf_tta_gather`` per parity builds it, the model runs ``max(1, max_batch // B)`` members
    per forward, one ``uf_tta_merge`` turns back, sums, scales and clamps."""
    if img.dim() != 4:
        raise ValueError(f"restore_ensemble expects (B,C,h,w), got {tuple(img.shape)}")
    even, odd = _check_ensemble(members, canvas, "restore_ensemble")
    B, _, h, w = img.shape
    ye, yo = _ensemble_members(model, img.to(torch.float32), B, h, w, canvas, even, odd, max_batch, False, False)
    return ops.tta_merge(ye, even, yo, odd, h, w, u8=False, clamp=clamp)


@torch.no_grad()
def restore_frames(model, frames: Tensor, canvas: str = "square", hwc: bool = True, bgr: bool = False, tile: int = None, min_overlap: int = 128,
                   max_batch: int = 8, out: Tensor = None, ensemble: int = None) -> Tensor:
    """``restore`` / ``restore_tiled`` for the pixels every caller starts and ends with: uint8 frames (B,h,w,C) (``hwc``, what a decoder hands over)
    or (B,C,h,w) on the model's device in, uint8 frames of the model's ``in_chans`` channels in the same layout out (into ``out`` when given).
    What the reference's scripts do on the host around the forward -- ``load_img``'s ``/ 255`` (utils/image_utils.py:31-35) and
    ``img_as_ubyte(torch.clamp(restored, 0, 1))`` (test/test_gopro_hide.py:103-110) -- is one launch on each side of the model here
    (``uf_frames_to_canvas``, ``uf_canvas_to_frames``): bit for bit the quantised ``restore(model, frames / 255, canvas=canvas)``.
    ``bgr``: the frames are BGR(A) as cv2 decodes them; the model sees RGB(A) and the result is BGR(A) again.
    ``tile``: frames larger than one ``tile`` x ``tile`` window (a multiple of 128) take ``restore_tiled``'s route -- the same tiles
    (``uf_tiles_gather``), forwarded ``max_batch`` at a time into one tile-output buffer, and the same cross-fade (``uf_tiles_blend``: one launch,
    no accumulator or weight-sum buffer); a frame that fits one tile takes the canvas route, as ``restore_tiled`` falls back to ``restore``
    (on the square canvas).
    ``ensemble``: 8, 4, 2 or 1 members of ``restore_ensemble``, uint8 in and uint8 out through ``uf_tta_gather`` / ``uf_tta_merge``: bit for bit
    the quantised ``restore_ensemble(model, planes, canvas=canvas, members=ensemble, clamp=False)`` of the frames divided by 255 as
    ``uf_frames_to_canvas`` divides them (an IEEE division; ``torch.div(255)`` on the device multiplies by a reciprocal).  Not together with ``tile``."""
    B, C, h, w = _check_frames(frames, hwc, bgr, canvas, "restore_frames")
    if tile is not None and tile % 128:
        raise ValueError("restore_frames: tile must be a multiple of 128")
    if ensemble is not None:
        if tile is not None:
            raise ValueError("restore_frames: ensemble and tile cannot be combined (the self-ensemble of a tiled restoration is not offered)")
        even, odd = _check_ensemble(ensemble, canvas, "restore_frames", "ensemble")
        out_C = int(getattr(model, "in_chans", C))                   # before any forward, as FrameRestorer checks it
        if bgr and out_C < 3:
            raise ValueError(f"restore_frames: bgr needs at least 3 output channels, the model gives {out_C}")
        ye, yo = _ensemble_members(model, frames, B, h, w, canvas, even, odd, max_batch, hwc, bgr)
        return ops.tta_merge(ye, even, yo, odd, h, w, u8=True, hwc=hwc, swap_rb=bgr, out=out)
    if tile is not None and (h > tile or w > tile):
        ys, xs = _starts(h, tile, min_overlap), _starts(w, tile, min_overlap)
        origins = _tile_origins(ys, xs, frames.device)
        T, per = len(ys) * len(xs), max(1, max_batch // B)
        buf = None                                                   # (T*B, in_chans, tile, tile): sized by the first output
        for j0 in range(0, T, per):
            j1 = min(T, j0 + per)
            y = model(ops.tiles_gather(frames, origins[j0:j1], tile, hwc, bgr))
            if buf is None:
                buf = torch.empty((T * B,) + tuple(y.shape[1:]), dtype=torch.float32, device=frames.device)
            buf[j0 * B:j1 * B].copy_(y)
        if bgr and buf.shape[1] < 3:
            raise ValueError(f"restore_frames: bgr needs at least 3 output channels, the model gives {buf.shape[1]}")
        return ops.tiles_blend(buf, ys, xs, h, w, u8=True, hwc=hwc, swap_rb=bgr, out=out)
    if canvas == "square" or tile is not None:
        Xh = Xw = int(math.ceil(max(h, w) / 128.0) * 128)
    else:
        Xh, Xw = int(math.ceil(h / 128.0) * 128), int(math.ceil(w / 128.0) * 128)
    padded, _ = ops.frames_to_canvas(frames, Xh, Xw, hwc, bgr, with_mask=False)
    y = model(padded)
    if bgr and y.shape[1] < 3:
        raise ValueError(f"restore_frames: bgr needs at least 3 output channels, the model gives {y.shape[1]}")
    return ops.canvas_to_frames(y, h, w, hwc, bgr, out=out)


class FrameRestorer:
    """Host uint8 frames in, host uint8 frames out, with the copies overlapped with the forward: ``depth`` (1 ... 4) slots, each with a pinned
    input buffer, a pinned output buffer, device uint8 buffers and a stream of its own, all allocated once (at the first ``submit``).  ``submit(frames)`` copies the
    frames (a numpy array or a CPU tensor, ``(batch,) + frame_shape``, or ``frame_shape`` alone at batch 1) into the slot's pinned buffer and
    enqueues, on the slot's stream, the asynchronous copy to the device, ``restore_frames`` and the asynchronous copy back; it returns a
    ticket.  ``ticket.result()`` waits for that slot and returns the restored frames in the type and rank that were submitted -- a copy, or
    with ``copy=False`` a view of the pinned buffer that stays valid until the slot is used again.  A slot is reused only after its ticket has
    been consumed (``submit`` raises ``RuntimeError`` otherwise); ``map`` keeps ``depth`` frames in flight and yields results in order.
    Results are ``restore_frames``' bit for bit (``ensemble=8``: its self-ensemble route).  Parameters must not change while frames are in flight (``PipelinedForward``'s rule: the
    operand pack is built on the caller's stream, which the slot stream waits for): ``drain()`` first.  No HIP graph is used."""

    MAX_DEPTH = 4      # Uformer keeps 8 workspaces by stream; the library's side streams share the hardware queues with these

    class Ticket:
        def __init__(self, owner, slot, as_numpy, squeeze):
            self._owner, self._slot, self._as_numpy, self._squeeze = owner, slot, as_numpy, squeeze
            self._done = False

        def result(self, copy: bool = True):
            if self._done:
                raise RuntimeError("FrameRestorer: this ticket was consumed already")
            s = self._owner._slots[self._slot]
            s["event"].synchronize()
            self._done = True
            s["ticket"] = None
            t = s["pin_out"][0] if self._squeeze else s["pin_out"]
            if self._as_numpy:
                a = t.numpy()
                return a.copy() if copy else a
            return t.clone() if copy else t

    def __init__(self, model, frame_shape, batch: int = 1, depth: int = 2, canvas: str = "rect", hwc: bool = True, bgr: bool = False, tile: int = None,
                 min_overlap: int = 128, max_batch: int = 8, device=None, ensemble: int = None):
        if not 1 <= int(depth) <= self.MAX_DEPTH:
            raise ValueError(f"FrameRestorer: depth must be 1 ... {self.MAX_DEPTH}, got {depth}")
        if canvas not in ("square", "rect"):
            raise ValueError(f"FrameRestorer: canvas must be 'square' or 'rect', got {canvas!r}")
        frame_shape = tuple(int(v) for v in frame_shape)
        if len(frame_shape) != 3 or min(frame_shape) < 1 or batch < 1:
            raise ValueError(f"FrameRestorer: frame_shape must be (h,w,C) or (C,h,w) and batch positive, got {frame_shape}, batch {batch}")
        C = frame_shape[2] if hwc else frame_shape[0]
        if bgr and C < 3:
            raise ValueError(f"FrameRestorer: bgr needs at least 3 channels, the frames have {C}")
        if tile is not None and tile % 128:
            raise ValueError("FrameRestorer: tile must be a multiple of 128")
        if ensemble is not None:
            if tile is not None:
                raise ValueError("FrameRestorer: ensemble and tile cannot be combined (the self-ensemble of a tiled restoration is not offered)")
            _check_ensemble(ensemble, canvas, "FrameRestorer", "ensemble")
        out_C = int(getattr(model, "in_chans", C))
        if bgr and out_C < 3:
            raise ValueError(f"FrameRestorer: bgr needs at least 3 output channels, the model gives {out_C}")
        self.model, self.batch, self.depth, self.frame_shape = model, int(batch), int(depth), frame_shape
        self._kw = dict(canvas=canvas, hwc=hwc, bgr=bgr, tile=tile, min_overlap=min_overlap, max_batch=max_batch, ensemble=ensemble)
        self._in_shape = (self.batch,) + frame_shape
        self._out_shape = (self.batch,) + (frame_shape[:2] + (out_C,) if hwc else (out_C,) + frame_shape[1:])
        self._device, self.device = device, None
        self._slots, self._closed, self._k = None, False, 0

    def _allocate(self) -> None:
        """the slots, once, at the first submit (so that the argument checks of the constructor and of submit need no device)"""
        dev = torch.device(self._device) if self._device is not None else next(self.model.parameters()).device
        if dev.type != "cuda":
            raise ops.UformerHipError(f"FrameRestorer runs on the GPU only (the model is on {dev}); there is no CPU path")
        self.device = dev
        self._slots = [dict(pin_in=torch.empty(self._in_shape, dtype=torch.uint8).pin_memory(), pin_out=torch.empty(self._out_shape, dtype=torch.uint8).pin_memory(),
                            dev_in=torch.empty(self._in_shape, dtype=torch.uint8, device=dev), dev_out=torch.empty(self._out_shape, dtype=torch.uint8, device=dev),
                            stream=torch.cuda.Stream(device=dev), event=torch.cuda.Event(), ticket=None, pack=None) for _ in range(self.depth)]

    @torch.no_grad()
    def submit(self, frames) -> "FrameRestorer.Ticket":
        if self._closed:
            raise RuntimeError("FrameRestorer: closed")
        as_numpy = not isinstance(frames, torch.Tensor)
        t = torch.from_numpy(frames) if as_numpy else frames
        if t.dtype != torch.uint8:
            raise ValueError(f"FrameRestorer: frames must be uint8, got {t.dtype}")
        squeeze = self.batch == 1 and tuple(t.shape) == self.frame_shape
        if not squeeze and tuple(t.shape) != self._in_shape:
            raise ValueError(f"FrameRestorer: frames must be {self._in_shape}, got {tuple(t.shape)}")
        if t.is_cuda:
            raise ValueError("FrameRestorer takes host frames; restore_frames takes frames on the device")
        if self._slots is None:
            self._allocate()
        s = self._slots[self._k % self.depth]
        if s["ticket"] is not None:
            raise RuntimeError("FrameRestorer: the slot's previous result was not consumed; call result() on its ticket first")
        self._k += 1
        (s["pin_in"][0] if squeeze else s["pin_in"]).copy_(t)
        # the operand pack is (re)built on the caller's stream, which the slot stream waits for, as PipelinedForward.submit does; the slot keeps the pack
        # it ran on alive until it is used again
        get = getattr(self.model, "_get_packed", None)
        s["pack"] = get(self.device) if get is not None else None
        st = s["stream"]
        st.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(st):
            s["dev_in"].copy_(s["pin_in"], non_blocking=True)
            restore_frames(self.model, s["dev_in"], out=s["dev_out"], **self._kw)
            s["pin_out"].copy_(s["dev_out"], non_blocking=True)
            s["event"].record(st)
        s["ticket"] = FrameRestorer.Ticket(self, (self._k - 1) % self.depth, as_numpy, squeeze)
        return s["ticket"]

    def map(self, iterable):
        """Generator: the restored frames of an iterable of frames, ``depth`` in flight, in order (copies)."""
        pending = []
        for frames in iterable:
            if len(pending) >= self.depth:
                yield pending.pop(0).result()
            pending.append(self.submit(frames))
        while pending:
            yield pending.pop(0).result()

    def drain(self) -> None:
        """wait on the host for everything submitted so far (before a parameter update, a checkpoint load, ...); tickets stay valid"""
        for s in self._slots or ():
            s["stream"].synchronize()

    def close(self) -> None:
        """drain and release the buffers; outstanding ``copy=False`` views and tickets become invalid"""
        self.drain()
        self._slots, self._closed = None, True
