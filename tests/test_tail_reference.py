"""CPU companion of tests/test_gpu_tail_exact.py: shows that its gates gate something.

1. The emulations of tests/tail_cases.py are right: against torch.optim.AdamW, the float64 oracle, O.mixup, torch.clamp.
2. Stand-in faulty kernels (numpy) are REJECTED by the comparison functions the GPU file uses, on the GPU file's own case data.
3. Conditions on the inputs that the gates rely on."""
import numpy as np
import pytest
import torch

import tail_cases as T
from oracle import uformer_oracle as O
from tail_cases import A, f32, f64

H = T.HYPER


# ---- 1. the emulations are right ------------------------------------------------------------------------------------------------------
ADAMW_TORCH_CASES = [("lengths", s) for s in T.ADAMW_SETTINGS] + [(k, "gs1_wd") for k in T.ADAMW_COUNTS if k != "all_empty"] + [("same_bits", "mixed_signs")]


def _gpu_case(name, setting):
    """(lengths, seed) as tests/test_gpu_tail_exact.py draws them"""
    if name == "lengths":
        return T.ADAMW_LENGTHS, T.ADAMW_SEEDS["placements"]
    if name == "same_bits":
        return T.ADAMW_LENGTHS, T.ADAMW_SEEDS["same_bits"]
    return T.ADAMW_COUNTS[name], T.ADAMW_SEEDS["counts"]


@pytest.mark.parametrize("name,setting", ADAMW_TORCH_CASES)
def test_adamw_emulation_within_1ulp_of_torch_adamw(name, setting):
    """three steps of the emulation vs torch.optim.AdamW (f32, CPU) restarted from the emulation's state each step: each step's p, m, v within 1 ulp on
    all the GPU file's case data, same seeds (measured: m bit-equal -- torch's lerp is the same fused operation --, p and v 0 or 1 ulp: torch orders
    addcmul / addcdiv differently)"""
    gs, wd, _ = T.ADAMW_SETTINGS[setting]
    lengths, seed = _gpu_case(name, setting)
    data = [d for d in T.adamw_setting_data(lengths, seed, setting) if d["p"].size]
    cur = [(d["p"], d["m"], d["v"]) for d in data]
    worst = 0.0
    for s in range(3):
        ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p, _, _ in cur]
        opt = torch.optim.AdamW(ps, lr=H["lr"], betas=(H["b1"], H["b2"]), eps=H["eps"], weight_decay=wd, foreach=False)
        for p_, (_, m, v), d in zip(ps, cur, data):
            opt.state[p_] = {"step": torch.tensor(float(s)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
            p_.grad = torch.from_numpy(d["g"][s] * f32(gs))
        opt.step()
        c = T.adamw_consts(H["lr"], H["b1"], H["b2"], H["eps"], wd, s + 1, gs)
        cur = [T.adamw_emu(p, d["g"][s], m, v, c) for (p, m, v), d in zip(cur, data)]
        for p_, (p, m, v) in zip(ps, cur):
            st = opt.state[p_]
            for got, ref in ((p, p_.detach().numpy()), (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
                worst = max(worst, float(T.ulp_distance(got, ref).max()))
            assert np.all(v >= 0) and np.all(np.isfinite(p)) and np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("n", T.CHARB_NS)
@pytest.mark.parametrize("kind", T.CHARB_DATA)
@pytest.mark.parametrize("eps,gs", T.CHARB_SETTINGS)
def test_charbonnier_emulation_within_1ulp_of_float64(kind, eps, gs, n):
    """The emulated loss against the float64 oracle on the same float32 inputs, 1 ulp of float32.  With the float32 group sums the kernel used to form
    (four values r of three float32 roundings each, three rounded partial sums) the case (gauss, eps 1e-3, n = 4) measured 1.29 ulp; the kernel and
    the emulation now take the loss term in float64, and the figure is the final rounding: at most 0.5 ulp."""
    y, t = T.charb_data(kind, n)
    dy, loss, _ = T.charbonnier_emu(y, t, eps, gs)
    d = y.astype(f64) - t.astype(f64)
    e2 = float(f32(eps) * f32(eps))
    r = np.sqrt(d * d + e2)
    yt, tt = torch.from_numpy(y).double(), torch.from_numpy(t).double()
    assert abs(float(O.charbonnier_loss(yt, tt, eps)) - r.mean()) <= 1e-6 * r.mean()          # the oracle squares eps in double: same formula
    u = T.worst_ulp(None, [loss], [r.mean()])
    print(f"charbonnier emulation vs float64: {kind} eps={eps} n={n}: {u:.3f} ulp")
    assert u <= 1.0, u
    # dy has no bound in the issue; sanity only: d (1), d*d, + eps2, sqrt (r: <= 3 half-ulp steps), gs*d, the quotient -- within 4 ulp of float64
    assert T.worst_ulp(None, dy, float(f32(gs) / f32(n)) * d / r) <= 4.0


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("shape", T.MSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mse_reference_within_1ulp_of_float64(shape, clamp):
    """the reference of the GPU gate (float64 sums of FLOAT32 squares of float32 differences, rounded to float32) against the float64 oracle (exact
    differences and squares) on the GPU file's own data: 1 ulp of float32, and the PSNR that follows from it against O.psnr in float64"""
    a, b = T.mse_data(shape)
    mse32 = T.mse_ref(a, b, clamp).astype(f32)
    u = T.worst_ulp(None, mse32, T.mse_oracle64(a, b, clamp))
    print(f"mse reference vs float64: {shape} clamp={clamp}: {u:.3f} ulp")
    assert u <= 1.0, u
    if clamp and a[0].size <= 4097:                                # myPSNR clamps; O.psnr on float64 tensors is the float64 oracle
        for i in (0, a.shape[0] - 1):
            got = f32(20.0 * np.log10(1.0 / np.sqrt(float(mse32[i]))))
            assert T.worst_ulp(None, [got], [O.psnr(torch.from_numpy(a[i]).double(), torch.from_numpy(b[i]).double())]) <= 1.0


def test_clamp_pad_and_ssim_references_match_torch_and_the_oracle():
    x = T.pad_image(2, 3, 7, 5)
    assert T.diff_bits(None, np.nan_to_num(T.clamp01(x), nan=7.0), np.nan_to_num(torch.clamp(torch.from_numpy(x), 0, 1).numpy(), nan=7.0)) == 0
    assert np.isnan(T.clamp01(x)).sum() == np.isnan(x).sum() == 1
    c, m = T.pad_ref(x[:1], 128, 128)
    oc, om = O.expand2square(torch.from_numpy(x[:1]), 128.0)
    assert T.diff_bits(None, c, oc.numpy()) == 0 and T.diff_bits(None, m, om.numpy()) == 0
    # ssim_ref IS O.ssim behind ssim_sanitize: that step must leave every pixel the oracle defines alone (wrapping values included) and zero the rest
    for kind in T.SSIM_DATA:
        a, _ = T.ssim_pair(kind, 3, 27, 43, 1)
        keep = np.isfinite(a) & (np.abs(a) < 1e6)
        assert T.diff_bits(None, T.ssim_sanitize(a)[keep], a[keep]) == 0 and np.all(T.ssim_sanitize(a)[~keep] == 0)
        assert (kind == "nonfinite") == bool((~keep).any())


def test_mixup_emulation_bit_equal_to_oracle():
    for B, per in T.MIXUP_SHAPES[:-1]:
        x, lam = T.mixup_data(B, per)
        for perm in T.mixup_perms(B).values():
            ref = O.mixup(torch.from_numpy(x).reshape(B, per, 1, 1), torch.from_numpy(lam), torch.from_numpy(perm)).reshape(B, per).numpy()
            assert T.diff_bits(None, T.mixup_emu(x, lam, perm), ref) == 0


def test_scaler_emulation_follows_gradscaler_rules():
    for state, growth, backoff, interval in T.SCALER_TABLE:
        s = T.scaler_update_emu(state, growth, backoff, interval)
        st = A(state)
        assert s[2] == 0 and T.diff_bits(None, s[5:], st[5:]) == 0
        if st[2] != 0:
            assert s[0] == st[0] * f32(backoff) and s[3] == 0 and s[4] == st[4]
        else:
            grew = st[3] + 1 >= interval
            with np.errstate(over="ignore"):
                grown = st[0] * f32(growth)
            assert s[0] == (grown if grew else st[0]) and s[3] == (0 if grew else st[3] + 1) and s[4] == st[4] + 1
        if np.isfinite(s[0]):
            assert s[1] == f32(1.0 / float(s[0]))                    # 1 / scale correctly rounded (double division of a float32, rounded once more: exact enough to pin it)
    assert len(T.SCALER_TABLE) >= 12


# ---- 2. stand-in faults are rejected by the GPU file's comparison functions -----------------------------------------------------------------
def _traj(lengths, seed, setting="gs1_wd", upd=T.adamw_emu):
    gs, wd, _ = T.ADAMW_SETTINGS[setting]
    data = T.adamw_setting_data(lengths, seed, setting)
    return data, T.adamw_run_emu(data, wd, gs, upd=upd)


def _traj_diff(a, b):
    return sum(T.diff_bits(None, x, y) for sa, sb in zip(a, b) for ta, tb in zip(sa, sb) for x, y in zip(ta, tb))


@pytest.mark.parametrize("setting", ["gs1_wd", "gs0.25_wd", "mixed_signs"])
def test_adamw_case_data_tells_the_fused_form_from_the_emulation(setting):
    """the vector path before the fix (p = fma(p, decay, -step q)) differs from the emulation on the case data: the data can tell the two paths apart"""
    data, good = _traj(T.ADAMW_LENGTHS, T.ADAMW_SEEDS["placements"], setting)
    _, fused = _traj(T.ADAMW_LENGTHS, T.ADAMW_SEEDS["placements"], setting, upd=T.adamw_fused_p)
    per_tensor = [sum(T.diff_bits(None, good[s][i][0], fused[s][i][0]) for s in range(3)) for i in range(len(T.ADAMW_LENGTHS))]
    assert sum(per_tensor) >= 1 and all(n >= 1 for n, L in zip(per_tensor, T.ADAMW_LENGTHS) if L >= 8191), per_tensor


@pytest.mark.parametrize("name,setting", [("lengths", "gs1_wd"), ("same_bits", "mixed_signs"), ("count81", "gs1_wd"), ("first_empty", "gs1_wd")])
@pytest.mark.parametrize("fault", [T.adamw_skip_last, T.adamw_chunk_twice])
def test_adamw_element_faults_rejected(fault, name, setting):
    """on the GPU file's own data (same lengths, seeds and settings): the fault shows in EVERY non-empty tensor, whatever its length"""
    lengths, seed = _gpu_case(name, setting)
    _, good = _traj(lengths, seed, setting)
    _, bad = _traj(lengths, seed, setting, upd=fault)
    for i, L in enumerate(lengths):
        n = sum(T.diff_bits(None, x, y) for s in range(3) for x, y in zip(good[s][i], bad[s][i]))
        assert (n >= 1) == (L > 0), (i, L, n)


@pytest.mark.parametrize("name", ["count41", "count81", "empties_interleaved_77_of_90"])
def test_adamw_wrong_first_chunk_rejected(name):
    lengths = T.ADAMW_COUNTS[name]
    data, good = _traj(lengths, T.ADAMW_SEEDS["counts"])
    prev = [(d["p"], d["m"], d["v"]) for d in data]
    bad = [T.adamw_wrong_first_chunk(lengths, good[0], prev)] + good[1:]
    assert _traj_diff(good, bad) >= 1
    live = [n for n in lengths if n > 0]
    assert len(live) > T.AW_MAX


def test_zero_gradient_case_still_moves_the_state():
    data, good = _traj(T.ADAMW_LENGTHS, T.ADAMW_SEEDS["placements"], "zero_grad")
    assert all(T.diff_bits(None, good[0][i][0], data[i]["p"]) >= 1 for i in range(len(data)) if data[i]["p"].size > 8)


def test_scaled_acceptance_rejects_a_wrong_step_count():
    """the 9 candidates absorb one float32 step of the device's double pow / sqrt, not a fault: bias corrections taken at t + 1 instead of t match none of
    them (while they still depend on t: at 100000 both have long been 1).  Neighbouring candidates may match the same launch -- the update is a small
    correction of p -- so the GPU file records every pair that matched."""
    data = T.adamw_data(T.ADAMW_LENGTHS, T.ADAMW_SEEDS["scaled"], steps=1)
    for steps in T.SCALED_STEPS[:-1]:
        for scale in T.SCALED_SCALES:
            mk = lambda k: A([scale, f32(1) / f32(scale), 0, 0, k, 0, 0, 0])        # noqa: E731
            wrong = T.scaled_consts(H["lr"], H["b1"], H["b2"], H["eps"], 0.02, 1.0, mk(steps + 1))
            bad = [T.adamw_emu(d["p"], d["g"][0], d["m"], d["v"], wrong) for d in data]
            c0 = T.scaled_consts(H["lr"], H["b1"], H["b2"], H["eps"], 0.02, 1.0, mk(steps))
            for pair in T.scaled_pairs(c0):
                ref = [T.adamw_emu(d["p"], d["g"][0], d["m"], d["v"], dict(c0, step=pair[0], bc2s=pair[1])) for d in data]
                assert sum(T.diff_bits(None, a[0], b[0]) for a, b in zip(ref, bad)) >= 1, (steps, pair)
    assert T.scaled_consts(H["lr"], H["b1"], H["b2"], H["eps"], 0.02, 1.0, A([1, 1, 1, 0, 0, 0, 0, 0])) is None


def test_found_inf_blind_to_last_chunk_rejected():
    for L in (1, 8191, 8192, 8193, 16387):
        g = [np.zeros(5, f32), np.ones(L, f32)]
        g[1][-1] = np.inf
        st = A([1, 1, 0, 0, 0, 0, 0, 0])
        assert T.found_inf_emu(g, st)[2] == 1
        assert T.diff_bits(None, T.found_inf_blind_last_chunk(g, st), T.found_inf_emu(g, st)) >= 1
    for ok in (T.FLT_MAX, -T.FLT_MAX, f32(1e-45), f32(-1e-40), f32(-0.0)):
        assert T.found_inf_emu([A([ok])], st)[2] == 0
    assert T.found_inf_emu([np.array([0xFFC00001], np.uint32).view(f32)], st)[2] == 1


def test_nan_swallowing_clamp_rejected():
    x = T.pad_image(2, 3, 7, 5)
    assert T.diff_values(None, T.clamp01_nan_to_zero(x), T.clamp01(x)) >= 1
    a = np.random.default_rng(1).random((3, 3, 12, 12)).astype(f32)
    b = a.copy()
    b[1, 0, 3, 3] = np.nan
    good = T.mse_ref(a, b, True)
    with np.errstate(invalid="ignore"):
        bad = ((T.clamp01_nan_to_zero(a) - T.clamp01_nan_to_zero(b)).reshape(3, -1).astype(f64) ** 2).mean(1).astype(f32)
    assert np.isnan(good[1]) and not np.isnan(bad[1]) and T.worst_ulp(None, bad, good) > 1.0
    c = a.copy()
    c[0, 0, 0, 0], c[2, 0, 0, 0] = np.inf, -np.inf
    assert T.clamp01(c)[0, 0, 0, 0] == 1 and T.clamp01(c)[2, 0, 0, 0] == 0


@pytest.mark.parametrize("H_,W_", [(27, 27), (43, 27), (27, 11)])
def test_ssim_tile_dropping_its_last_row_rejected(H_, W_):
    for kind in ("noisy", "identical"):
        a, b = T.ssim_pair(kind, 3, H_, W_, 7)
        assert T.worst_ulp(None, [T.ssim_drop_last_row(a, b)], [T.ssim_ref(a, b)]) > 1.0


@pytest.mark.parametrize("fault", [T.aug_swapped_1_3, T.aug_flip_first])
def test_wrong_transforms_rejected(fault):
    N, Hh, W = T.AUG_FRAME
    fr = T.index_frames(N, 3, Hh, W)
    for ps in T.AUG_PS[1:]:                                    # a 1 x 1 patch has one transform
        meta = T.aug_meta(N, Hh, W, ps)
        assert T.diff_bits(None, T.crop_augment_ref(fr, meta, ps, fault()), T.crop_augment_ref(fr, meta, ps)) >= 1


def test_pad_offset_rounded_up_rejected():
    for B, C, h, w, Xh, Xw in T.PAD_SHAPES[:4]:
        img = T.pad_image(B, C, h, w)
        good, bad = T.pad_ref(img, Xh, Xw), T.pad_ref(img, Xh, Xw, off=T.pad_offset_up)
        assert T.diff_bits(None, bad[0], good[0]) >= 1 and T.diff_bits(None, bad[1], good[1]) >= 1
        assert (Xh - h) % 2 == 1 or (Xw - w) % 2 == 1


# ---- 3. conditions on the inputs --------------------------------------------------------------------------------------------------------
def test_index_coded_frames_are_distinct_integers_below_2_24():
    for shape in ((T.AUG_FRAME[0], 6) + T.AUG_FRAME[1:], (2, 6, 150, 160), (T.AUG_FRAME[0] + 2, 6) + T.AUG_FRAME[1:]):
        fr = T.index_frames(*shape)
        assert fr.max() < 2 ** 24 and np.unique(fr).size == fr.size and np.all(fr == np.rint(fr))


def test_bad_meta_and_perm_stay_inside_the_allocation_even_unclamped():
    N, Hh, W = T.AUG_FRAME
    for C in (1, 3, 4, 6):
        frame = C * Hh * W
        for ps in (7, 48):
            bad = T.bad_meta(N, Hh, W, ps)
            assert T.diff_bits(None, bad.view(f32), T.clamp_meta(bad, N, Hh, W, ps).view(f32)) >= 7        # the entries ARE bad
            for row in bad:
                lo, hi = T.meta_extent(row, C, Hh, W, ps)
                assert -frame <= lo and hi < (N + 1) * frame, (row, lo, hi)       # one guard frame either side holds it
                assert sum(int(a != b) for a, b in zip(row[:3], T.clamp_meta(row, N, Hh, W, ps)[0][:3])) <= 1 and abs(int(row[1]) - int(T.clamp_meta(row, N, Hh, W, ps)[0][1])) <= 4
    for B, per in T.MIXUP_SHAPES:                                                # MixUp: the layout the GPU file builds, one guard sample either side
        flat, off = T.mixup_guarded(np.zeros((B, per), f32))
        assert flat.size == (B + 2) * per
        for p in (-1, B):
            lo, hi = T.perm_extent(p, per, off)
            assert 0 <= lo and hi < flat.size, (B, per, p, lo, hi)
        assert T.perm_extent(-2, per, off)[0] < 0 and T.perm_extent(B + 1, per, off)[1] >= flat.size     # and no further


def test_layout_and_arena():
    offs, words = T.layout([5, 0, 8193], [1, 2, 3])
    assert [o % 4 for o in offs] == [1, 2, 3] and offs[0] >= T.GAP and offs[2] - (offs[0] + 5) >= T.GAP and words >= offs[2] + 8193 + T.GAP
    ar = T.Arena(words)
    ar.place(offs[0], np.arange(5))
    assert ar.guards_intact() and ar.ptr(offs[0]) % 16 == 4
    snap = ar.snapshot()
    ar.f[offs[0] + 5] = 0.0
    assert not ar.guards_intact() and not ar.unchanged(snap)


def test_ulp_gates():
    one = f32(1)
    up = np.nextafter(one, f32(2))
    assert T.worst_ulp(None, [up], [1.0]) == 1.0 and T.worst_ulp(None, [np.nextafter(up, f32(2))], [1.0]) == 2.0
    assert T.worst_ulp(None, [np.nan], [np.nan]) == 0.0 and T.worst_ulp(None, [0.0], [np.nan]) == np.inf and T.worst_ulp(None, [np.nan], [1.0]) == np.inf
    assert T.diff_values(None, [-0.0, np.nan], [0.0, np.nan]) == 0 and T.diff_bits(None, [-0.0], [0.0]) == 1
    assert T.ulp_distance([up], [one])[0] == 1 and T.ulp_distance([f32(-0.0)], [f32(0.0)])[0] == 0
