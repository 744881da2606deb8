"""GPU: the 14 entry points of uf_train.hip (training tail, metrics, pad / crop, input pipeline) through the C ABI, at chosen placements inside NaN-filled
arenas (tests/tail_cases.py has the emulations, the arena, the comparisons and the case lists, tests/test_tail_reference.py shows on the
CPU that these gates reject stand-in faults).

Gate ZERO (every bit) against a float32 emulation or torch slicing: AdamW (plain and scaled), the loss-scaler kernels, Charbonnier's dy, pad, crop,
crop + augment, MixUp.  Gate 1 ulp of float32: Charbonnier's loss (against the emulated loss), per-image MSE (float64 sums of float32 squares), SSIM
(the float64 oracle).  After every call the guard words around each output are looked at, and const operands' whole arenas.
Figures go to $UF_REPORT_DIR/parity_tail.json."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import tail_cases as T
from tail_cases import A, f32

pytestmark = pytest.mark.gpu
H = T.HYPER
DEV = "cuda"


def L():
    from uformer_amd import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def run(name, *args, expect=T.UF_OK):
    rc = getattr(L(), name)(*args)
    torch.cuda.synchronize()
    assert rc == expect, (name, rc)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    T.WALL["test_gpu_tail_exact.py"] = round(time.time() - t0, 2)
    T.write_report()


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


class Out:
    """an output of n float32 words at element offset ``mod`` (mod 4) of its own arena"""

    def __init__(self, n, mod=0):
        (self.off,), words = T.layout([n], [mod])
        self.n, self.ar = n, T.Arena(words, DEV)
        self.ar.live[self.off:self.off + n] = True
        self.ptr = self.ar.ptr(self.off)

    def get(self, shape=None):
        assert self.ar.guards_intact(), "a word outside the output was written"
        v = self.ar.read(self.off, self.n)
        return v if shape is None else v.reshape(shape)


class In:
    """a const operand inside its own arena; ``check()`` = the whole arena is bit-intact"""

    def __init__(self, values, mod=0):
        v = A(values).reshape(-1)
        (self.off,), words = T.layout([v.size], [mod])
        self.ar = T.Arena(words, DEV)
        self.ar.place(self.off, v)
        self.ptr = self.ar.ptr(self.off)
        self.snap = self.ar.snapshot()

    def check(self):
        assert self.ar.unchanged(self.snap), "a const operand was written"


def workspace(nbytes):
    """``nbytes`` of workspace with 64 guard bytes of 0xA5 behind it"""
    return torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)


def ws_guard_ok(buf, nbytes):
    return bool((buf[nbytes:] == 0xA5).all())


# ==========================================================================================================================================
# uf_adamw_step / uf_adamw_step_scaled
# ==========================================================================================================================================
class AdamwRig:
    """four arenas (p, g, m, v); tensor i of family j sits at an offset = mods[i][j] (mod 4); zero-length entries are NULL pointers"""

    def __init__(self, lengths, mods, data):
        self.lengths, self.n = list(lengths), len(lengths)
        self.ar, self.offs = [], []
        for j in range(4):
            offs, words = T.layout(lengths, [m[j] for m in mods])
            self.ar.append(T.Arena(words, DEV))
            self.offs.append(offs)
        for i, (nn, d) in enumerate(zip(lengths, data)):
            if nn:
                for j, key in enumerate(("p", "g", "m", "v")):
                    self.ar[j].place(self.offs[j][i], d[key][0] if key == "g" else d[key])
        self.ptrs = [(C.c_void_p * self.n)(*[self.ar[j].ptr(self.offs[j][i]) if nn else None for i, nn in enumerate(lengths)]) for j in range(4)]
        self.numel = (C.c_longlong * self.n)(*lengths)

    def set_grads(self, data, s):
        for i, nn in enumerate(self.lengths):
            if nn:
                self.ar[1].write(self.offs[1][i], data[i]["g"][s])

    def call(self, name, *tail):
        snap = self.ar[1].snapshot()
        run(name, self.ptrs[0], self.ptrs[1], self.ptrs[2], self.ptrs[3], self.numel, self.n, *tail)
        assert self.ar[1].unchanged(snap), "the gradient arena was written"
        for j in (0, 2, 3):
            assert self.ar[j].guards_intact(), "pgmv"[j] + ": a guard word was written"

    def read(self):
        return [tuple(self.ar[j].read(self.offs[j][i], nn) for j in (0, 2, 3)) for i, nn in enumerate(self.lengths)]


@functools.lru_cache(maxsize=None)
def trajectory(lengths, seed, setting):
    gs, wd, _ = T.ADAMW_SETTINGS[setting]
    data = T.adamw_setting_data(lengths, seed, setting)
    return data, T.adamw_run_emu(data, wd, gs)


def adamw_three_steps(entry, lengths, mods, seed, setting):
    """three uf_adamw_step calls from the case's start state; every step's p, m, v bit-equal to the emulation.  Returns the final state."""
    gs, wd, _ = T.ADAMW_SETTINGS[setting]
    data, traj = trajectory(tuple(lengths), seed, setting)
    rig = AdamwRig(lengths, mods, data)
    for s in range(3):
        rig.set_grads(data, s)
        rig.call("uf_adamw_step", H["lr"], H["b1"], H["b2"], H["eps"], wd, s + 1, gs, st())
        got = rig.read()
        bad = {(i, "pmv"[k]): d for i in range(len(lengths)) for k in range(3) if (d := T.diff_bits(entry, got[i][k], traj[s][i][k]))}
        assert not bad, (s + 1, bad)
    return got


@pytest.mark.parametrize("setting", list(T.ADAMW_SETTINGS))
@pytest.mark.parametrize("placement", list(T.ADAMW_PLACEMENTS))
def test_adamw_step_bits_at_every_placement(placement, setting):
    """lengths 1 .. 16387 in one call, every tensor at the placement: the 128-bit path (all four aligned), its n % 4 tail, and the scalar path of any
    misaligned operand (a gradient that is a view into a flat all-reduce bucket) compute the emulation's bits"""
    mods = [T.ADAMW_PLACEMENTS[placement]] * len(T.ADAMW_LENGTHS)
    adamw_three_steps("uf_adamw_step", T.ADAMW_LENGTHS, mods, T.ADAMW_SEEDS["placements"], setting)


@pytest.mark.parametrize("placement", [p for p in T.ADAMW_PLACEMENTS if p != "aligned"])
def test_adamw_step_same_bits_aligned_and_misaligned(placement):
    """the same values at an aligned and at a misaligned placement: the same bits, compared with each other (and each with the emulation on the way)"""
    k = len(T.ADAMW_LENGTHS)
    a = adamw_three_steps(None, T.ADAMW_LENGTHS, [T.ADAMW_PLACEMENTS["aligned"]] * k, T.ADAMW_SEEDS["same_bits"], "mixed_signs")
    b = adamw_three_steps(None, T.ADAMW_LENGTHS, [T.ADAMW_PLACEMENTS[placement]] * k, T.ADAMW_SEEDS["same_bits"], "mixed_signs")
    assert sum(T.diff_bits("uf_adamw_step", x, y) for ta, tb in zip(a, b) for x, y in zip(ta, tb)) == 0


@pytest.mark.parametrize("name", [k for k in T.ADAMW_COUNTS if k != "all_empty"])
def test_adamw_step_tensor_counts_and_empty_entries(name):
    """1, 40, 41, 81 tensors (one, one full, two and three launch groups), zero-length entries with NULL pointers in front, between and behind;
    placements rotate from tensor to tensor"""
    lengths = T.ADAMW_COUNTS[name]
    pl = list(T.ADAMW_PLACEMENTS.values())
    adamw_three_steps("uf_adamw_step", lengths, [pl[i % len(pl)] for i in range(len(lengths))], T.ADAMW_SEEDS["counts"], "gs1_wd")


def test_adamw_step_all_entries_empty_is_ok_and_writes_nothing():
    lengths = T.ADAMW_COUNTS["all_empty"]
    rig = AdamwRig(lengths, [(0, 0, 0, 0)] * 3, T.adamw_data(lengths, 1))
    snaps = [a.snapshot() for a in rig.ar]
    rig.call("uf_adamw_step", H["lr"], H["b1"], H["b2"], H["eps"], 0.02, 1, 1.0, st())
    rig.call("uf_adamw_step_scaled", H["lr"], H["b1"], H["b2"], H["eps"], 0.02, 1.0, In(A([1, 1, 0, 0, 0, 0, 0, 0])).ptr, st())
    assert all(a.unchanged(s) for a, s in zip(rig.ar, snaps))


def test_optim_adamw_bucket_view_grads_give_the_same_parameters():
    """through optim.AdamW: gradients that are odd-offset views of one flat buffer (what dist.OverlappedGradientAllReduce leaves in param.grad) vs
    separately allocated gradients -> bit-identical parameters after three steps"""
    from uformer_amd import optim
    shapes = [(1,), (3,), (7, 5), (64,), (8193,), (128, 33), (4, 1, 3, 3), (16387,)]
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=gen) for s in shapes]
    pa, pb = [torch.nn.Parameter(p.clone().to(DEV)) for p in init], [torch.nn.Parameter(p.clone().to(DEV)) for p in init]
    kw = dict(lr=H["lr"], betas=(H["b1"], H["b2"]), eps=H["eps"], weight_decay=0.02)
    oa, ob = optim.AdamW(pa, **kw), optim.AdamW(pb, **kw)
    offs, cur = [], 1
    for p in init:
        offs.append(cur)
        cur += p.numel() + (p.numel() % 2)          # every offset odd
    flat = torch.zeros(cur + 8, device=DEV)
    for step in range(3):
        for i, (a, b, o) in enumerate(zip(pa, pb, offs)):
            gr = (torch.randn(a.shape, generator=gen) * 10.0 ** (i % 5 - 3)).to(DEV)
            flat[o:o + gr.numel()].copy_(gr.reshape(-1))
            a.grad = flat[o:o + gr.numel()].view(a.shape)
            b.grad = gr.clone()
            assert a.grad.data_ptr() % 16 != 0 and b.grad.data_ptr() % 16 == 0
        oa.step(); ob.step()
        for a, b in zip(pa, pb):
            assert T.diff_bits("optim.AdamW(bucket views)", a.detach().cpu().numpy(), b.detach().cpu().numpy()) == 0, step


@pytest.mark.parametrize("placement", list(T.ADAMW_PLACEMENTS))
def test_adamw_step_scaled(placement):
    """found_inf set: p, m, v bit-unchanged.  Clear: for steps taken in {0, 1, 9, 999, 100000} x scale in {65536, 1000} ALL elements of the launch match
    the emulation for one and the same (stepf, bc2s) pair out of {host value, its float32 neighbours}^2 (the device rounds its own double pow / sqrt);
    the pairs that matched are recorded."""
    lengths = T.ADAMW_LENGTHS
    mods = [T.ADAMW_PLACEMENTS[placement]] * len(lengths)
    data = T.adamw_data(lengths, T.ADAMW_SEEDS["scaled"], steps=1)
    for scale in T.SCALED_SCALES:
        for steps in (None,) + T.SCALED_STEPS:
            state = A([scale, f32(1) / f32(scale), 0 if steps is not None else 1, 3, 5 if steps is None else steps, 0, 0, 0])
            sd = In(state)
            rig = AdamwRig(lengths, mods, data)
            before = rig.read()
            rig.call("uf_adamw_step_scaled", H["lr"], H["b1"], H["b2"], H["eps"], 0.02, 1.0, sd.ptr, st())
            sd.check()
            got = rig.read()
            if steps is None:
                assert sum(T.diff_bits("uf_adamw_step_scaled", x, y) for ta, tb in zip(got, before) for x, y in zip(ta, tb)) == 0
                continue
            c0 = T.scaled_consts(H["lr"], H["b1"], H["b2"], H["eps"], 0.02, 1.0, state)
            matched, fewest = [], None
            for idx, pair in enumerate(T.scaled_pairs(c0)):
                c = dict(c0, step=pair[0], bc2s=pair[1])
                n = sum(T.diff_bits(None, x, y) for d, tg in zip(data, got) for x, y in zip(T.adamw_emu(d["p"], d["g"][0], d["m"], d["v"], c), tg))
                fewest = n if fewest is None else min(fewest, n)
                if n == 0:
                    matched.append(idx)
            total = 3 * sum(lengths)
            T.record("uf_adamw_step_scaled", total, 0 if matched else fewest, 0.0)
            T.SCALED_PAIRS.append({"placement": placement, "scale": scale, "steps": steps, "matched": matched, "host_pair_is_index": 0,
                                   "index_means": "3 * i + j: stepf = (host, below, above)[i], bc2s = (host, below, above)[j]"})
            assert matched, (scale, steps, "no candidate pair matches every element; fewest differing", fewest)


# ==========================================================================================================================================
# uf_grad_scaler_check / uf_grad_scaler_update
# ==========================================================================================================================================
CHECK_LENGTHS = [5 if i == 0 else 16387 if i == 41 else 8193 if i == 80 else T.SMALL_LENGTHS[i % len(T.SMALL_LENGTHS)] for i in range(81)]
CHECK_POSITIONS = {"t0[0]": (0, 0), "last[last]": (80, 8192), "t41[8191]": (41, 8191), "t41[8192]": (41, 8192), "t41[16386]": (41, 16386)}
STATE0 = [65536.0, 1 / 65536.0, 0.0, 7.0, 9.0, 1.5, -2.5, 1e-40]


@pytest.fixture(scope="module")
def grad_rig():
    """81 gradients as misaligned views (offset i % 4) inside one NaN arena: a read past a view's end sees NaN and flags falsely"""
    rng = np.random.default_rng(4)
    offs, words = T.layout(CHECK_LENGTHS, [i % 4 for i in range(81)])
    ar = T.Arena(words, DEV)
    for o, n in zip(offs, CHECK_LENGTHS):
        ar.place(o, rng.standard_normal(n).astype(f32))
    ptrs = (C.c_void_p * 81)(*[ar.ptr(o) for o in offs])
    numel = (C.c_longlong * 81)(*CHECK_LENGTHS)
    return ar, offs, ptrs, numel


def scaler_check(grad_rig, state_values):
    ar, offs, ptrs, numel = grad_rig
    state = Out(8)
    state.ar.f[state.off:state.off + 8].copy_(torch.from_numpy(A(state_values)))
    snap = ar.snapshot()
    run("uf_grad_scaler_check", ptrs, numel, 81, state.ptr, st())
    assert ar.unchanged(snap), "the gradient arena was written"
    return state.get()


@pytest.mark.parametrize("pos", list(CHECK_POSITIONS))
@pytest.mark.parametrize("value", ["+inf", "-inf", "nan_ffc00001"])
def test_grad_scaler_check_finds_one_non_finite_element(grad_rig, value, pos):
    ar, offs, _, _ = grad_rig
    t, e = CHECK_POSITIONS[pos]
    bitsv = {"+inf": 0x7F800000, "-inf": 0xFF800000 - (1 << 32), "nan_ffc00001": 0xFFC00001 - (1 << 32)}[value]
    keep = int(ar.bits[offs[t] + e])
    ar.bits[offs[t] + e] = bitsv
    try:
        got = scaler_check(grad_rig, STATE0)
    finally:
        ar.bits[offs[t] + e] = keep
    want = A(STATE0)
    want[2] = 1.0
    assert T.diff_bits("uf_grad_scaler_check", got, want) == 0, got


def test_grad_scaler_check_does_not_flag_finite_extremes_and_keeps_a_set_flag(grad_rig):
    ar, offs, _, _ = grad_rig
    assert T.diff_bits("uf_grad_scaler_check", scaler_check(grad_rig, STATE0), A(STATE0)) == 0           # clean gradients next to NaN guards: no over-read
    vals = A([T.FLT_MAX, -T.FLT_MAX, 1e-45, -1e-40, 1.1754942e-38, -0.0, 0.0])
    keep = ar.snapshot()
    for t in (0, 41, 80):
        n = CHECK_LENGTHS[t]
        ar.f[offs[t]:offs[t] + n].copy_(torch.from_numpy(np.resize(vals, n)))
    try:
        assert T.diff_bits("uf_grad_scaler_check", scaler_check(grad_rig, STATE0), A(STATE0)) == 0
    finally:
        ar.bits.copy_(keep)
    preset = A(STATE0)
    preset[2] = 1.0
    assert T.diff_bits("uf_grad_scaler_check", scaler_check(grad_rig, preset), preset) == 0


@pytest.mark.parametrize("row", range(len(T.SCALER_TABLE)))
def test_grad_scaler_update_table(row):
    values, growth, backoff, interval = T.SCALER_TABLE[row]
    state = Out(8)
    state.ar.f[state.off:state.off + 8].copy_(torch.from_numpy(A(values)))
    run("uf_grad_scaler_update", state.ptr, growth, backoff, interval, st())
    assert T.diff_bits("uf_grad_scaler_update", state.get(), T.scaler_update_emu(values, growth, backoff, interval)) == 0


# ==========================================================================================================================================
# uf_charbonnier_fwd_bwd
# ==========================================================================================================================================
def charbonnier(y, t, eps, gs, with_dy=True, dy_out=None):
    n = y.size
    yi, ti = In(y), In(t)
    dy = (dy_out or Out(n)) if with_dy else None
    loss = Out(1)
    nb = L().uf_charbonnier_workspace_bytes(n)
    ws = workspace(nb)
    run("uf_charbonnier_fwd_bwd", yi.ptr, ti.ptr, dy.ptr if dy else None, loss.ptr, n, eps, gs, ws.data_ptr(), nb, st())
    yi.check(); ti.check()
    assert ws_guard_ok(ws, nb)
    return (dy.get() if dy else None), loss.get()


@pytest.mark.parametrize("kind", T.CHARB_DATA)
@pytest.mark.parametrize("eps,gs", T.CHARB_SETTINGS)
def test_charbonnier_dy_bits_and_loss(kind, eps, gs):
    """dy bit-equal to the emulation, loss within 1 ulp of the emulated loss, two runs bit-identical, dy = NULL gives the same loss bits; n from 1 (tail
    only) to 4 * 2048 * 256 + 7, the first n at which the grid-stride loop wraps"""
    for n in T.CHARB_NS:
        y, t = T.charb_data(kind, n)
        edy, eloss, _ = T.charbonnier_emu(y, t, eps, gs)
        dy, loss = charbonnier(y, t, eps, gs)
        dy2, loss2 = charbonnier(y, t, eps, gs)
        _, loss3 = charbonnier(y, t, eps, gs, with_dy=False)
        assert T.diff_bits("uf_charbonnier_fwd_bwd:dy", dy, edy) == 0, n
        u = float(T.ulp_distance(loss, [eloss])[0])
        T.record("uf_charbonnier_fwd_bwd:loss", 1, int(u > 1), u)
        assert u <= 1.0, (n, loss, eloss)
        assert T.diff_bits(None, dy2, dy) == 0 and T.diff_bits(None, loss2, loss) == 0 and T.diff_bits(None, loss3, loss) == 0, n


@pytest.mark.parametrize("eps,gs", T.CHARB_SETTINGS)
def test_charbonnier_body_and_tail_same_bits(eps, gs):
    """n = 7: elements 0..2 (the 128-bit body) and 4..6 (the scalar tail) hold the same values and must get the same dy"""
    for seed in range(8):
        y, t = T.charb_data("gauss", 7, seed=40 + seed)
        y[4:7], t[4:7] = y[0:3], t[0:3]
        dy, _ = charbonnier(y, t, eps, gs)
        assert T.diff_bits("uf_charbonnier_fwd_bwd:dy", dy[4:7], dy[0:3]) == 0


# ==========================================================================================================================================
# uf_batch_mse / uf_batch_ssim
# ==========================================================================================================================================
def metric(name, a, b, *extra):
    n, Cc, Hh, W = a.shape
    ai, bi, out = In(a), In(b), Out(n, mod=1)
    nb = L().uf_image_metric_workspace_bytes(n, Cc, Hh, W)
    ws = workspace(nb)
    run(name, ai.ptr, bi.ptr, out.ptr, n, Cc, Hh, W, *extra, ws.data_ptr(), nb, st())
    ai.check(); bi.check()
    assert ws_guard_ok(ws, nb)
    return out.get()


@pytest.mark.parametrize("clamp", [0, 1])
@pytest.mark.parametrize("shape", T.MSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_mse_within_1ulp(shape, clamp):
    a, b = T.mse_data(shape)
    assert T.worst_ulp("uf_batch_mse", metric("uf_batch_mse", a, b, clamp), T.mse_ref(a, b, bool(clamp))) <= 1.0


@pytest.mark.parametrize("clamp", [0, 1])
def test_batch_mse_non_finite_pixels(clamp):
    """a NaN pixel makes ITS image NaN under both settings (torch.clamp keeps NaN: a diverged restoration must not score a finite PSNR) and leaves the
    other images' bits alone; under the clamp +inf counts as 1 and -inf as 0"""
    rng = np.random.default_rng(8)
    a = (rng.random((3, 3, 12, 12)) * 1.4 - 0.2).astype(f32)
    b = (a + rng.standard_normal(a.shape).astype(f32) * f32(0.05)).astype(f32)
    clean = metric("uf_batch_mse", a, b, clamp)
    for side in (0, 1):
        x = [a.copy(), b.copy()]
        x[side][1, 2, 5, 7] = np.nan
        got = metric("uf_batch_mse", x[0], x[1], clamp)
        assert np.isnan(got[1]) and T.diff_bits("uf_batch_mse", got[[0, 2]], clean[[0, 2]]) == 0, got
        assert T.worst_ulp("uf_batch_mse", got, T.mse_ref(x[0], x[1], bool(clamp))) <= 1.0
    if clamp:
        x, z = a.copy(), a.copy()
        x[0, 0, 0, 0], x[2, 1, 3, 3] = np.inf, -np.inf
        z[0, 0, 0, 0], z[2, 1, 3, 3] = 1.0, 0.0
        got = metric("uf_batch_mse", x, b, 1)
        assert T.diff_bits("uf_batch_mse", got, metric("uf_batch_mse", z, b, 1)) == 0 and T.worst_ulp("uf_batch_mse", got, T.mse_ref(x, b, True)) <= 1.0


@functools.lru_cache(maxsize=None)
def ssim_case(kind, Cc, Hh, W):
    a, b = T.ssim_pair(kind, Cc, Hh, W, 100 * Hh + W + Cc)
    return a, b, T.ssim_ref(a, b)


@pytest.mark.parametrize("Cc", [1, 3, 4])
@pytest.mark.parametrize("Hh,W", T.SSIM_HW)
def test_batch_ssim_within_1ulp(Hh, W, Cc):
    """one image of every data class, then 65 images cycling through the classes (finalize: more than 64 images), against the float64 oracle"""
    cases = [ssim_case(k, Cc, Hh, W) for k in T.SSIM_DATA]
    for kind, (a, b, ref) in zip(T.SSIM_DATA, cases):
        assert T.worst_ulp("uf_batch_ssim", metric("uf_batch_ssim", a[None], b[None]), [ref]) <= 1.0, kind
        if kind == "identical":
            assert abs(ref - 1.0) <= 1e-12
    a = np.stack([cases[i % len(cases)][0] for i in range(65)])
    b = np.stack([cases[i % len(cases)][1] for i in range(65)])
    assert T.worst_ulp("uf_batch_ssim", metric("uf_batch_ssim", a, b), [cases[i % len(cases)][2] for i in range(65)]) <= 1.0


# ==========================================================================================================================================
# uf_expand2square / uf_expand_canvas / uf_crop_clamp / uf_crop_clamp_canvas
# ==========================================================================================================================================
@pytest.mark.parametrize("shape", T.PAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_expand_and_crop_bits(shape):
    """pad: the whole canvas and mask are written (no NaN pattern survives inside), nothing behind them is, bit-equal to slicing -- NaN, +-inf and -0.0 in
    the image travel unchanged; mask = NULL writes the same canvas.  crop: bit-equal to slicing, and by value + NaN mask to torch.clamp of it."""
    B, Cc, h, w, Xh, Xw = shape
    img = T.pad_image(B, Cc, h, w)
    ref_c, ref_m = T.pad_ref(img, Xh, Xw)
    entries = [("uf_expand_canvas", "uf_crop_clamp_canvas", (Xh, Xw))] + ([("uf_expand2square", "uf_crop_clamp", (Xh,))] if Xh == Xw else [])
    for pad, crop, X in entries:
        src = In(img)
        for with_mask in (True, False):
            canvas, mask = Out(B * Cc * Xh * Xw), Out(B * Xh * Xw, mod=1)
            run(pad, src.ptr, canvas.ptr, mask.ptr if with_mask else None, B, Cc, h, w, *X, st())
            src.check()
            assert T.diff_bits(pad, canvas.get(), ref_c) == 0
            if with_mask:
                assert T.diff_bits(pad, mask.get(), ref_m) == 0
            else:
                assert mask.ar.unchanged(torch.full_like(mask.ar.bits, T.POISON))
        full = T.pad_image(B, Cc, Xh, Xw, seed=17)                # a canvas with something in its border too
        cv = In(full)
        for clamp in (0, 1):
            out = Out(B * Cc * h * w, mod=clamp)
            run(crop, cv.ptr, out.ptr, B, Cc, h, w, *X, clamp, st())
            cv.check()
            want = T.crop_ref(full, h, w, bool(clamp))
            assert (T.diff_values if clamp else T.diff_bits)(crop, out.get(), want) == 0
            if clamp:
                assert T.diff_values(None, want, torch.clamp(torch.from_numpy(T.crop_ref(full, h, w, False)), 0, 1).numpy()) == 0


# ==========================================================================================================================================
# uf_crop_augment_c
# ==========================================================================================================================================
def make_frames(N, Cc, Hh, W, u8):
    """(N + 2) dense frames, CHW: frame 0 and N + 1 are guards (an unclamped index reads them, never memory outside).  f32: index-coded over the whole stack."""
    if u8:
        return np.random.default_rng(N + Cc + Hh).integers(0, 256, (N + 2, Cc, Hh, W), dtype=np.uint8)
    return T.index_frames(N + 2, Cc, Hh, W)


def crop_augment(stack, meta, N, ps, hwc):
    """stack (N + 2, C, H, W) numpy (uint8 or float32); the kernel gets frames 1 .. N"""
    u8 = stack.dtype == np.uint8
    _, Cc, Hh, W = stack.shape
    lay = np.ascontiguousarray(stack.transpose(0, 2, 3, 1)) if hwc else stack
    d = dev(lay)
    snap = d.clone()
    md = dev(meta, np.int32)
    B = meta.shape[0]
    out = Out(B * Cc * ps * ps, mod=3)
    ptr = d.data_ptr() + Cc * Hh * W * d.element_size()
    run("uf_crop_augment_c", ptr, int(u8), int(hwc), out.ptr, md.data_ptr(), B, N, Cc, Hh, W, ps, st())
    assert torch.equal(d, snap) and torch.equal(md.cpu(), torch.from_numpy(np.ascontiguousarray(meta, np.int32)))
    return out.get((B, Cc, ps, ps))


def as_float(stack):
    return stack.astype(f32) / f32(255) if stack.dtype == np.uint8 else stack


@pytest.mark.parametrize("Cc", [1, 3, 4, 6])
@pytest.mark.parametrize("hwc", [0, 1], ids=["chw", "hwc"])
@pytest.mark.parametrize("u8", [0, 1], ids=["f32", "u8"])
def test_crop_augment_bits(u8, hwc, Cc):
    """the 8 transforms twice over, crops that touch every border of a 50 x 57 frame, patch sizes 1, 2, 7, 48; then bad metadata (one bad field per
    entry) must read what the clamped metadata reads"""
    N, Hh, W = T.AUG_FRAME
    stack = make_frames(N, Cc, Hh, W, u8)
    inner = as_float(stack[1:N + 1])
    for ps in T.AUG_PS:
        meta = T.aug_meta(N, Hh, W, ps)
        assert T.diff_bits("uf_crop_augment_c", crop_augment(stack, meta, N, ps, hwc), T.crop_augment_ref(inner, meta, ps)) == 0, ps
    for ps in (7, 48):
        bad = T.bad_meta(N, Hh, W, ps)
        assert T.diff_bits("uf_crop_augment_c", crop_augment(stack, bad, N, ps, hwc), T.crop_augment_ref(inner, T.clamp_meta(bad, N, Hh, W, ps), ps)) == 0, ps


@pytest.mark.parametrize("hwc", [0, 1], ids=["chw", "hwc"])
@pytest.mark.parametrize("Hh,W,ps", [(7, 7, 7), (7, 12, 7)])
def test_crop_augment_patch_as_large_as_the_frame(Hh, W, ps, hwc):
    N = 2
    stack = make_frames(N, 3, Hh, W, False)
    meta = np.array([[i % N, 0, (i * 3) % (W - ps + 1), i] for i in range(8)], np.int32)
    assert T.diff_bits("uf_crop_augment_c", crop_augment(stack, meta, N, ps, hwc), T.crop_augment_ref(stack[1:N + 1], meta, ps)) == 0


def test_crop_augment_all_256_byte_values():
    stack = np.tile(np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16), (3, 1, 1, 1))
    got = crop_augment(stack, np.array([[0, 0, 0, 0]], np.int32), 1, 16, 0)
    assert T.diff_bits("uf_crop_augment_c", got, np.arange(256, dtype=f32) / f32(255)) == 0


def test_crop_augment_grid_wrap():
    """B * C * ps^2 = 2 102 784 > 2048 workgroups x 1024 elements"""
    N, Cc, Hh, W, ps = 2, 6, 150, 160, 148
    stack = make_frames(N, Cc, Hh, W, False)
    meta = np.array([[i % N, i % 3, (5 * i) % 13, i % 8] for i in range(16)], np.int32)
    assert 16 * Cc * ps * ps > 2048 * 1024
    assert T.diff_bits("uf_crop_augment_c", crop_augment(stack, meta, N, ps, 0), T.crop_augment_ref(stack[1:N + 1], meta, ps)) == 0


# ==========================================================================================================================================
# uf_mixup
# ==========================================================================================================================================
def mixup(x, lam, perm):
    """x (B, per) sits between one guard sample either side, inside its arena"""
    B, per = x.shape
    flat, data_off = T.mixup_guarded(x)
    xi = In(flat)
    out = Out(B * per, mod=2)
    ld, pd = dev(lam, f32), dev(perm, np.int32)
    run("uf_mixup", xi.ptr + 4 * data_off, out.ptr, ld.data_ptr(), pd.data_ptr(), B, per, st())
    xi.check()
    return out.get((B, per))


@pytest.mark.parametrize("B,per", T.MIXUP_SHAPES)
def test_mixup_bits(B, per):
    x, lam = T.mixup_data(B, per)
    for name, perm in T.mixup_perms(B).items():
        assert T.diff_bits("uf_mixup", mixup(x, lam, perm), T.mixup_emu(x, lam, perm)) == 0, name


@pytest.mark.parametrize("B,per", [(2, 3), (16, 12288)])
def test_mixup_bad_perm_reads_the_clamped_sample(B, per):
    x, lam = T.mixup_data(B, per)
    lam = np.full(B, 0.3, f32)
    perm = np.arange(B)[::-1].copy()
    perm[0], perm[-1] = -1, B
    assert T.diff_bits("uf_mixup", mixup(x, lam, perm), T.mixup_emu(x, lam, np.clip(perm, 0, B - 1))) == 0


# ==========================================================================================================================================
# a few host-side refusals, by status (valid pointers throughout: a missing check cannot fault)
# ==========================================================================================================================================
def test_refusals():
    y, t, dy, loss = In(np.zeros(16, f32), mod=1), In(np.zeros(16, f32)), Out(16), Out(1)
    nb = L().uf_charbonnier_workspace_bytes(8)
    ws = workspace(nb)
    run("uf_charbonnier_fwd_bwd", y.ptr, t.ptr, dy.ptr, loss.ptr, 8, 1e-3, 1.0, ws.data_ptr(), nb, st(), expect=T.UF_ERR_ALIGN)
    a, out = In(np.zeros(3 * 10 * 16, f32)), Out(1)
    nb = L().uf_image_metric_workspace_bytes(1, 3, 11, 16)
    ws2 = workspace(nb)
    run("uf_batch_ssim", a.ptr, a.ptr, out.ptr, 1, 3, 10, 16, ws2.data_ptr(), nb, st(), expect=T.UF_ERR_SHAPE)
    x = Out(8)
    x.ar.f[x.off:x.off + 8] = 1.0
    lam, perm = dev(np.full(2, 0.5, f32)), dev(np.array([1, 0], np.int32))
    run("uf_mixup", x.ptr, x.ptr, lam.data_ptr(), perm.data_ptr(), 2, 4, st(), expect=T.UF_ERR_NULL)
    for o in (dy, loss, out):
        assert o.ar.unchanged(torch.full_like(o.ar.bits, T.POISON))
    y.check(); t.check(); a.check()
    assert T.diff_bits(None, x.get(), np.ones(8, f32)) == 0
