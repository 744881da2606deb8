"""CPU twin of tests/test_gpu_crossmod_saturated.py: builds every saturated case of the cross-modulator attention kernel (tests/crossmod_lattice.py
asserts each condition on the float64 reference while it builds one), and shows that the cases see the faults they are built for."""
import pytest
import torch

import crossmod_lattice as XL

IDS = [f"M{M}-C{C}-h{h}" for M, C, h in XL.CASES]


@pytest.mark.parametrize("dtype", XL.MODES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", XL.CASES, ids=IDS)
@pytest.mark.parametrize("kind", XL.KINDS)
def test_case_conditions_hold(kind, case, dtype):
    M, C, heads = case
    c = XL.cross_case(kind, M, C, heads, dtype)
    assert c["out"].shape == (M, C) and torch.equal(c["out"].float().double(), c["out"])
    if kind == "onehot":
        assert c["lead2"] >= XL.LEAD2 and bool((c["n_win"] == 1).all())
        if C // heads == 16:            # 32 signed codes for 64 keys: every code has two holders and the larger amplitude wins
            k = c["k"]
            t = c["target"]
            amp = k.abs()[..., 0]
            for h in range(heads):
                twins = (k[h] / amp[h][:, None]) @ (k[h] / amp[h][:, None]).t() == 16
                assert bool((twins.sum(1) == 2).all())
                assert bool((amp[h][t[h]] == torch.where(twins[t[h]], amp[h][None, :], torch.zeros(1, dtype=torch.float64)).max(1).values).all())
    else:
        assert bool((c["n_win"] == 64).all())
        assert torch.equal(c["o"], c["vt"].mean(2).reshape(1, C).expand(M, C))


def test_the_cases_cover_what_the_kernel_instantiates():
    assert {C // h for _, C, h in XL.CASES} == {16, 32} and {16, 32, 64} <= {C for _, C, _ in XL.CASES} and {256, 512} & {C for _, C, _ in XL.CASES}
    assert all(M % 64 == 0 and M > 64 for M, _, _ in XL.CASES)              # more than one tile


@pytest.mark.parametrize("kind", XL.KINDS)
def test_the_reference_moves_under_the_faults_it_is_built_for(kind):
    for (M, C, heads) in ((128, 64, 4), (128, 32, 1)):
        c = XL.cross_case(kind, M, C, heads, XL.BF16)
        assert torch.equal(XL.faulty_out(c, XL.BF16), c["out"])                                   # no fault: the reference itself
        faults = [dict(v_rowmajor=True), dict(no_residual=True)] + ([dict(head_roll=True)] if heads > 1 and kind == "onehot" else [])
        for f in faults:
            bad = XL.faulty_out(c, XL.BF16, **f)
            assert float((bad != c["out"]).double().mean()) > 0.25, f
