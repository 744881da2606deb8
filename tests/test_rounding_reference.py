"""CPU: the conditions of the rounding audit (tests/rounding_audit.py) on exactly the cases tests/test_gpu_rounding.py runs, and the
audit's own power: CPU stand-ins of the faults it exists for must fail it, the nearest-even emulation must pass.

Kind A conditions: at most 2 % of a case lies near a midpoint, and the float32 emulation (before the rounding to T) stays within tau / MARGIN of the float64
reference.  Kind B conditions, over three seeds: |b0| <= min_s |b_s| / 8 and |mu0| <= |mu_floor| / 8.
"""
import pytest
import torch

import edge_cases as E
import rounding_audit as RA
from rounding_audit import BF16, F16, HALF, TAG

IDS = TAG.get


def rne(x32, dtype):
    return RA.round_to(x32.float(), dtype)


def kind_a_conditions(name, ref, tau, emu32, dtype, flush=None, abs_floor=None):
    """both conditions, then: the nearest-even emulation passes the audit; a toward-zero and a floor final store fail it"""
    _, _, near, small, _ = RA.classify(ref, tau, dtype, flush, abs_floor)
    ok, worst = RA.emulation_within(emu32, ref, tau, small)
    assert ok, f"{name}: the float32 emulation leaves tau / MARGIN ({worst:.2f} x): the bound is not valid"
    rec = RA.audit_exact(name, rne(emu32, dtype), ref, tau, dtype, flush, abs_floor)
    assert rec["near_share"] <= RA.NEAR_CAP and rec["mismatches"] == 0
    for mode in ("rz", "floor"):
        with pytest.raises(AssertionError, match="not the documented value"):
            RA.audit_exact(name + "/" + mode, RA.round_to(emu32.float(), dtype, mode), ref, tau, dtype, flush, abs_floor)
        assert RA.RECORDS[name + "/" + mode]["mismatches"] > 0.2 * (rec["elements"] - rec["small"]), "a truncating store must change a large share of the elements"
    return rec


# ---------------------------------------------------------------------------------------------------------------------------
# the tools themselves
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_directed_roundings_and_spacing(dtype):
    eps = float(torch.finfo(dtype).eps)
    x = torch.tensor([1 + 0.75 * eps, -(1 + 0.75 * eps), 1 + 0.25 * eps, -(1 + 0.25 * eps), 3.0, 0.0], dtype=torch.float64)
    assert RA.round_to(x, dtype).tolist() == [1 + eps, -(1 + eps), 1.0, -1.0, 3.0, 0.0]
    assert RA.round_to(x, dtype, "rz").tolist() == [1.0, -1.0, 1.0, -1.0, 3.0, 0.0]
    assert RA.round_to(x, dtype, "floor").tolist() == [1.0, -(1 + eps), 1.0, -(1 + eps), 3.0, 0.0]
    t = RA.tiny(dtype)
    assert RA.spacing(torch.tensor([1.0, 1.99, 2.0, -0.75, t, t / 4, 0.0]), dtype).tolist() == [eps, eps, 2 * eps, eps / 2, t * eps, t * eps, t * eps]
    assert RA.gelu_domain(dtype).numel() >= {BF16: 4608, F16: 36864}[dtype] + 5


def test_documented_forms_agree_with_edge_cases():
    """the audit's references are edge_cases' documented forms: the forward to float64 rounding, the gradient up to the 7 digits gelu_grad_t's two constants carry
    (and its clamp u <= 80, which edge_cases.gelu_grad_ref leaves out: compared where it is idle)"""
    x = RA.gelu_domain(F16).double()
    ref = RA.gelu_doc(x)[0]
    assert float(((ref - E.gelu_ref(x, BF16)).abs() / ref.abs().clamp_min(1e-300)).max()) < 1e-12
    idle = (x * (E.GELU_A + E.GELU_B * x * x) < 40) & ((x + 0.752).abs() > 0.05)
    g, g0 = RA.gelu_grad_doc(x)[0], E.gelu_grad_ref(x, BF16)
    rel = (g - g0).abs() / g0.abs()
    assert float(rel[x > -0.5].max()) < 2e-6               # the two terms do not cancel there
    assert float(rel[idle].max()) < 1e-4                    # where they do, the 1e-7 of the constants is amplified


# ---------------------------------------------------------------------------------------------------------------------------
# Kind A
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_gelu_domain_conditions_and_stand_ins(dtype):
    x = RA.gelu_domain(dtype)
    ref, tau, flush, floor = RA.gelu_doc(x)
    kind_a_conditions(f"cpu/gelu_fwd/{TAG[dtype]}", ref, tau, RA.gelu32(x), dtype, flush, floor)
    # the erf form where the sigmoid form is documented, and a constant off in its 4th digit: both are fractions of an ulp of T away
    for label, wrong in (("erf", RA.gelu_erf64(x)), ("constant", RA.gelu_off64(x))):
        with pytest.raises(AssertionError, match="not the documented value"):
            RA.audit_exact(f"cpu/gelu_fwd/{label}/{TAG[dtype]}", wrong.to(dtype), ref, tau, dtype, flush, floor)
    for which in ("one", "seeded"):
        dy = RA.gelu_dy(dtype, which)
        ref, tau = RA.gelu_grad_doc(x, dy)
        kind_a_conditions(f"cpu/gelu_bwd/{which}/{TAG[dtype]}", ref, tau, RA.gelu_grad32(x, dy), dtype)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("M,N,K", sorted({c[:3] for c in RA.EPI_GEMM_CASES}))
def test_gemm_epilogue_conditions(dtype, M, N, K):
    c = RA.epi_gemm_case(M, N, K)
    for t in (c["A"], c["W"], c["pre"], c["g"], c["a"]):
        RA.check_t_exact(t, dtype)
    assert float(c["pre"].abs().max()) >= 6.0 and 1.5 < float(c["pre"].std()) < 3.5, "pre-activations should cover about [-6, 6]"
    ref, tau, flush, floor = RA.gelu_doc(c["pre"])
    kind_a_conditions(f"cpu/linear_gelu/M{M}N{N}K{K}/{TAG[dtype]}", ref, tau, RA.gelu32(c["pre"]), dtype, flush, floor)
    ref, tau = RA.gelu_grad_doc(c["a"], c["g"])
    kind_a_conditions(f"cpu/linear_mul_dgelu/M{M}N{N}K{K}/{TAG[dtype]}", ref, tau, RA.gelu_grad32(c["a"], c["g"]), dtype)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("B,H,W,C", RA.EPI_DWCONV_CASES)
def test_dwconv_epilogue_conditions(dtype, B, H, W, C):
    c = RA.epi_dwconv_case(B, H, W, C)
    for t in (c["x"], c["pre"], c["g"], c["a"], c["dc"]):
        RA.check_t_exact(t, dtype)
    assert float(c["pre"].abs().max()) >= 5.0
    ref, tau, flush, floor = RA.gelu_doc(c["pre"])
    kind_a_conditions(f"cpu/dwconv_gelu/{B}x{H}x{W}x{C}/{TAG[dtype]}", ref, tau, RA.gelu32(c["pre"]), dtype, flush, floor)
    ref, tau = RA.gelu_grad_doc(c["a"], c["g"])
    kind_a_conditions(f"cpu/dwconv_mul_dgelu/{B}x{H}x{W}x{C}/{TAG[dtype]}", ref, tau, RA.gelu_grad32(c["a"], c["g"]), dtype)


def test_dwconv_cases_reach_both_kernels_and_an_all_border_map():
    assert any(W % 8 == 0 for _, _, W, _ in RA.EPI_DWCONV_CASES) and any(W % 8 for _, _, W, _ in RA.EPI_DWCONV_CASES)
    assert (8, 8) in [(H, W) for _, H, W, _ in RA.EPI_DWCONV_CASES] and any(H > 8 and W > 8 for _, H, W, _ in RA.EPI_DWCONV_CASES)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("C", RA.LN_CS)
def test_layernorm_conditions(dtype, C):
    c = RA.ln_case(C)
    assert c["x"].shape[0] == 128
    for name, windowed, shift, mod in RA.LN_MODES:
        ref, tau, emu = RA.ln_doc(c["x"], c["gamma"], c["beta"], c["mod"] if mod else None, windowed, shift, C)
        kind_a_conditions(f"cpu/layernorm/{name}/C{C}/{TAG[dtype]}", ref, tau, emu, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# what the old gate (edge_cases.gate: worst row <= 4 x the emulation's, floor 2 ulp) lets through
# ---------------------------------------------------------------------------------------------------------------------------
OLD_GATE_MISSES = {}


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_old_gate_lets_the_stand_ins_through(dtype):
    """on edge_cases' own GELU grids the old gate passes a toward-zero final store (asserted), and -- recorded in OLD_GATE_MISSES, DESIGN.md 2.3 has the list -- the
    floor store, the erf form and the off constant as well; the audit fails all four on its domain (test_gelu_domain_conditions_and_stand_ins)"""
    missed = set()
    for cls in E.GELU_CLASSES:
        x = E.gelu_grid(cls, dtype)
        exact, emu32 = E.gelu_ref(x, dtype), RA.gelu32(x)
        lim = E.gate(float(E.row_err(E.gelu_emu(x, dtype), exact).max()), dtype)
        stand_ins = {"rz_store": RA.round_to(emu32, dtype, "rz"), "floor_store": RA.round_to(emu32, dtype, "floor"),
                     "erf_form": RA.gelu_erf64(x).to(dtype).float(), "constant_4th_digit": RA.gelu_off64(x).to(dtype).float()}
        passed = {k for k, v in stand_ins.items() if float(E.row_err(v, exact).max()) <= lim}
        missed = passed if cls == E.GELU_CLASSES[0] else missed & passed
    OLD_GATE_MISSES[TAG[dtype]] = sorted(missed)
    print(f"old gate, {TAG[dtype]}: passes {sorted(missed)} on every GELU grid")
    assert "rz_store" in missed


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_old_gate_lets_a_truncated_operand_through(dtype):
    """attention forward, diffuse class: P truncated toward zero stays inside the old row gate; the slope sees it (test_kind_b_conditions)"""
    c = RA.diffuse_case(2, 32, 0, dtype)
    exact = RA.att_fwd(c)
    lim = E.gate(float(E.row_err(RA.att_fwd(c, RA.Rounder(("p", "o"), dtype)), exact).max()), dtype)
    for fault in ({"p": "rz"}, {"o": "rz"}):
        assert float(E.row_err(RA.att_fwd(c, RA.Rounder(("p", "o"), dtype, fault)), exact).max()) <= lim


# ---------------------------------------------------------------------------------------------------------------------------
# Kind B
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("entry", RA.KIND_B_ENTRY_POINTS)
def test_kind_b_conditions(dtype, entry):
    """three seeds: the nearest-even emulation's slope is at most an eighth of the least visible truncation's, its mean signed error at most an eighth of a floor
    store's; used as the kernel, every faulty emulation fails the gate and the nearest-even one passes"""
    bad = []
    for seed in RA.SEEDS:
        for label, case, args in RA.kind_b_cases(entry, dtype, seed):
            for out, ref, run, switches, final in RA.kind_b_jobs(entry, case, *args):
                st = RA.emulation_stats(ref, run, switches, final, dtype)
                name = f"cpu/{entry}.{out}/{label}/seed{seed}"
                if not RA.condition_ok(st):
                    bad.append(f"{name}: b0 {st['b0']:.2e} b_s {st['b']} mu0 {st['mu0']} mu_floor {st['mu_floor']}")
                if seed:
                    continue
                assert all(b < 0 for b in st["b"].values()), f"{name}: truncation toward zero must shrink"
                assert not RA.gate_kernel(name, run(RA.Rounder(switches, dtype)), ref, st, dtype if final else None)
                for fname, modes in RA.faults(switches, final):
                    assert RA.gate_kernel(name + "/" + fname, run(RA.Rounder(switches, dtype, modes)), ref, st, dtype if final else None), f"{name}: {fname} passes the gate"
    assert not bad, "\n".join(bad)


def test_every_switch_is_covered():
    """every rounding point of a block, and the dS of the attention backward, is truncated in the case of the kernel that owns it; what the whole-block case
    cannot see is listed, and owned"""
    assert set(RA.BLOCK_OBSERVABLE) | set(RA.BLOCK_NOT_OBSERVABLE) == set(RA.BLOCK_POINTS)
    assert set(RA.SWITCH_OWNERS) == set(RA.BLOCK_POINTS) | {"ds"}
    for switch, (entry, local) in RA.SWITCH_OWNERS.items():
        assert entry in RA.KIND_B_ENTRY_POINTS and entry != "uf_lewin_block_fwd"
        label, case, args = RA.kind_b_cases(entry, BF16)[0]
        assert any(local in switches for _, _, _, switches, _ in RA.kind_b_jobs(entry, case, *args)), (switch, entry)


def test_fused_ffn_widths():
    assert any(C <= 128 for C in RA.FFN_CASES) and 256 in RA.FFN_CASES
