"""GPU: rounding audit of the 2-byte stores of the nonlinear kernels, through the C ABI, bf16 and f16 (tests/rounding_audit.py has the helpers, the case lists and
the references; tests/test_rounding_reference.py asserts the conditions on the CPU and shows what the audit catches; DESIGN.md section 2.3 has the argument).

Kind A: the stored value is the documented function's float64 value rounded once to T, nearest-even, to the bit; either neighbour where that value lies within tau
(the float32 evaluation error, bounded from the reference alone) of a midpoint; one subnormal step below T's smallest normal.  At most 2 % of a case may be near.
Kind B: shrinkage slope and mean signed error of the kernel against the float64 reference, gated at a quarter of what the CPU emulation shows with one rounding point
truncating (slope) or a floor-type final store (mean).  Figures go to $UF_REPORT_DIR/parity_rounding.json.
"""
import pytest
import torch

import rounding_audit as RA
from rounding_audit import HALF, TAG

pytestmark = pytest.mark.gpu
IDS = TAG.get
ENTRY_POINTS = RA.KIND_A_ENTRY_POINTS + RA.KIND_B_ENTRY_POINTS
_RAN = set()             # test functions of this file that have run in this process


@pytest.fixture(autouse=True)
def _ran(request):
    yield
    _RAN.add(request.node.originalname)


@pytest.fixture(scope="module", autouse=True)
def _dump_report(request):
    """the figures go to the report; and if every test function of this file has run, every listed entry point was compared"""
    yield
    RA.dump_report()
    mine = {n for n, f in request.module.__dict__.items() if n.startswith("test_") and callable(f)}
    if mine <= _RAN:
        seen = {k.split("/")[0].split(".")[0] for k in list(RA.RECORDS) + list(RA.STATS)}
        missing = [n for n in ENTRY_POINTS if n not in seen]
        assert not missing, f"every test of this file ran, but these entry points were not compared: {missing}"


def ops():
    from uformer_amd import ops as o
    return o


def dev(t, dtype):
    """a reference-side tensor on the GPU as ``dtype``: the cast must be exact"""
    out = t.to(dtype)
    assert torch.equal(out.double(), t.double()), "the value is not representable in the operand type"
    return out.cuda().contiguous()


def kind_a(name, got, ref, tau, emu32, dtype, flush=None, abs_floor=None):
    """the condition on the bound (the float32 emulation within tau / MARGIN), then the audit (which asserts the cap on the near share itself)"""
    _, _, _, small, _ = RA.classify(ref, tau, dtype, flush, abs_floor)
    ok, worst = RA.emulation_within(emu32, ref, tau, small)
    assert ok, f"{name}: the float32 emulation leaves tau / MARGIN ({worst:.2f} x)"
    torch.cuda.synchronize()
    rec = RA.audit_exact(name, got, ref, tau, dtype, flush, abs_floor)
    print(f"{name}: {rec}")


def assert_bits(name, got, ref64, dtype):
    assert torch.equal(got.cpu().view(torch.int16), ref64.to(dtype).view(torch.int16)), f"{name}: the stored pre-activation is not the exact lattice value"


def set_variant(monkeypatch, v):
    if v is None:
        monkeypatch.delenv("UF_VARIANT", raising=False)
    else:
        monkeypatch.setenv("UF_VARIANT", v)


# ---------------------------------------------------------------------------------------------------------------------------
# Kind A
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_gelu_every_value(dtype):
    """uf_gelu_fwd and uf_gelu_bwd (dy = 1 and a seeded dy) on every T value with |x| in [2^-14, 16), the zeros and the neighbours of -8.4"""
    x = RA.gelu_domain(dtype)
    ref, tau, flush, floor = RA.gelu_doc(x)
    kind_a(f"uf_gelu_fwd/{TAG[dtype]}", ops().gelu(x.cuda()), ref, tau, RA.gelu32(x), dtype, flush, floor)
    for which in ("one", "seeded"):
        dy = RA.gelu_dy(dtype, which)
        ref, tau = RA.gelu_grad_doc(x, dy)
        kind_a(f"uf_gelu_bwd/{which}/{TAG[dtype]}", ops().gelu_bwd(x.cuda(), dy.cuda()), ref, tau, RA.gelu_grad32(x, dy), dtype)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("M,N,K,variant", RA.EPI_GEMM_CASES)
def test_gemm_epilogues(dtype, M, N, K, variant, monkeypatch):
    """uf_linear_fwd (act = 1), uf_linear_pre_gelu_fwd (act_out, from its own stored out) and uf_linear_mul_dgelu on lattices: the accumulator is exact, only
    the epilogue rounds"""
    set_variant(monkeypatch, variant)
    c = RA.epi_gemm_case(M, N, K)
    tag = f"M{M}N{N}K{K}/{variant}/{TAG[dtype]}"
    A, W, b = dev(c["A"], dtype), dev(c["W"], dtype), c["bias"].float().cuda()
    ref, tau, flush, floor = RA.gelu_doc(c["pre"])
    emu = RA.gelu32(c["pre"])
    kind_a(f"uf_linear_fwd/{tag}", ops().linear(A, W, b, act=1), ref, tau, emu, dtype, flush, floor)
    pre, act = ops().linear_pre_gelu(A, W, b)
    assert_bits(f"uf_linear_pre_gelu_fwd/{tag}", pre, c["pre"], dtype)
    kind_a(f"uf_linear_pre_gelu_fwd/{tag}", act, ref, tau, emu, dtype, flush, floor)
    ref, tau = RA.gelu_grad_doc(c["a"], c["g"])
    got = ops().linear_mul_dgelu(A, W, torch.zeros(N, device="cuda"), dev(c["a"], dtype))
    kind_a(f"uf_linear_mul_dgelu/{tag}", got, ref, tau, RA.gelu_grad32(c["a"], c["g"]), dtype)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("B,H,W,C", RA.EPI_DWCONV_CASES)
def test_dwconv_epilogues(dtype, B, H, W, C):
    """uf_dwconv3x3_gelu_fwd, uf_dwconv3x3_fwd (gelu = 1), uf_dwconv3x3_pre_gelu_fwd (act_out), uf_dwconv3x3_mul_dgelu and the da of uf_dwconv3x3_bwd on lattices:
    the walking and the strip kernel, an all-border map and maps with an interior"""
    c = RA.epi_dwconv_case(B, H, W, C)
    tag = f"{B}x{H}x{W}x{C}/{TAG[dtype]}"
    x, w9, bias = dev(c["x"], dtype), c["w9"].float().cuda(), c["bias"].float().cuda()
    ref, tau, flush, floor = RA.gelu_doc(c["pre"])
    emu = RA.gelu32(c["pre"])
    kind_a(f"uf_dwconv3x3_gelu_fwd/{tag}", ops().dwconv3x3_gelu(x, w9, bias), ref, tau, emu, dtype, flush, floor)
    kind_a(f"uf_dwconv3x3_fwd/{tag}", ops().dwconv3x3(x, w9, bias, gelu=True), ref, tau, emu, dtype, flush, floor)
    pre, act = ops().dwconv3x3_pre_gelu(x, w9, bias)
    assert_bits(f"uf_dwconv3x3_pre_gelu_fwd/{tag}", pre, c["pre"], dtype)
    kind_a(f"uf_dwconv3x3_pre_gelu_fwd/{tag}", act, ref, tau, emu, dtype, flush, floor)
    dc, a, w9f = dev(c["dc"], dtype), dev(c["a"], dtype), w9.flip(0).contiguous()
    ref, tau = RA.gelu_grad_doc(c["a"], c["g"])
    emu = RA.gelu_grad32(c["a"], c["g"])
    kind_a(f"uf_dwconv3x3_mul_dgelu/{tag}", ops().dwconv3x3_mul_dgelu(dc, w9f, a), ref, tau, emu, dtype)
    kind_a(f"uf_dwconv3x3_bwd/da/{tag}", ops().dwconv3x3_bwd(dc, w9f, a)[0], ref, tau, emu, dtype)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("C", RA.LN_CS)
def test_layernorm_t_output(dtype, C):
    """uf_layernorm_fwd: 128 integer rows, plain and windowed (shift 0 and 4), with and without modulator"""
    c = RA.ln_case(C)
    B, H, W = RA.LN_MAP
    for name, windowed, shift, mod in RA.LN_MODES:
        m = c["mod"] if mod else None
        ref, tau, emu = RA.ln_doc(c["x"], c["gamma"], c["beta"], m, windowed, shift, C)
        got = ops().layernorm(c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), B=B, H=H, W=W, dtype=dtype, windowed=bool(windowed), shift=shift,
                              modulator=None if m is None else m.cuda())
        kind_a(f"uf_layernorm_fwd/{name}/C{C}/{TAG[dtype]}", got, ref, tau, emu, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# Kind B
# ---------------------------------------------------------------------------------------------------------------------------
def kind_b(entry, dtype, kernel):
    """``kernel(case, *args)`` -> {output label: tensor}; every case of the entry point, every output: condition on the emulation, then the gate on the kernel"""
    bad = []
    for label, case, args in RA.kind_b_cases(entry, dtype):
        got = kernel(case, *args)
        torch.cuda.synchronize()
        for out, ref, run, switches, final in RA.kind_b_jobs(entry, case, *args):
            st = RA.emulation_stats(ref, run, switches, final, dtype)
            name = f"{entry}.{out}/{label}"
            assert RA.condition_ok(st), f"{name}: the emulation does not separate the faults: {st}"
            g = got[out].double().cpu()
            assert torch.isfinite(g).all(), name
            bad += RA.gate_kernel(name, g.reshape(ref.shape), ref, st, dtype if final else None)
            print(f"{name}: {RA.STATS[name]}")
    assert not bad, "\n".join(bad)


def _att_args(c):
    return [c[k].cuda() for k in ("q", "k", "vt", "bias")]


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_window_attention_fwd_statistics(dtype):
    kind_b("uf_window_attention_fwd", dtype, lambda c: {"o": ops().window_attention_core(*_att_args(c), H=RA.ATT_H, W=RA.ATT_W, shift=c["shift"])})


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_window_attention_bwd_statistics(dtype):
    def run(c):
        dq, dk, dvt, _ = ops().window_attention_bwd(*_att_args(c), c["do"].cuda(), RA.ATT_H, RA.ATT_W, shift=c["shift"])
        return {"dq": dq, "dk": dk, "dv": dvt.transpose(-1, -2)}
    kind_b("uf_window_attention_bwd", dtype, run)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_window_attention_bwd_qkv_statistics(dtype):
    def run(c):
        dqkv, _ = ops().window_attention_bwd_qkv(*_att_args(c), c["do"].cuda(), RA.ATT_H, RA.ATT_W, shift=c["shift"])
        C, nW, heads, hd = c["heads"] * c["hd"], c["nW"], c["heads"], c["hd"]
        split = lambda t: t.reshape(nW, 64, heads, hd).permute(0, 2, 1, 3)                     # noqa: E731
        return {"dq": split(dqkv[:, :C]), "dk": split(dqkv[:, C:2 * C]), "dv": split(dqkv[:, 2 * C:])}
    kind_b("uf_window_attention_bwd_qkv", dtype, run)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_window4_attention_statistics(dtype):
    B, H, W = RA.ATT4_MAP
    kind_b("uf_window4_attention_fwd", dtype, lambda c: {"o": ops().window4_attention(c["qkv"].cuda(), c["rpb4"].cuda(), B, H, W, c["heads"])})

    def run(c):
        C = c["heads"] * c["hd"]
        dqkv, _ = ops().window4_attention_bwd(c["qkv"].cuda(), c["rpb4"].cuda(), c["do"].cuda(), B, H, W, c["heads"])
        return {"dq": dqkv[:, :C], "dk": dqkv[:, C:2 * C], "dv": dqkv[:, 2 * C:]}
    kind_b("uf_window4_attention_bwd", dtype, run)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_ln_qkv_statistics(dtype):
    B, H, W = RA.LNG_MAP

    def run(c, heads, shift):
        M, C = c["x"].shape
        q, k, vt = ops().ln_qkv(c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), c["wq"].cuda(), c["bq"].cuda(), heads, B=B, H=H, W=W, shift=shift,
                                modulator=c["mod"].cuda())
        return {"q": q.permute(0, 2, 1, 3).reshape(M, C), "k": k.permute(0, 2, 1, 3).reshape(M, C), "v": vt.permute(0, 3, 1, 2).reshape(M, C)}
    kind_b("uf_ln_qkv_fwd", dtype, run)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_ln_linear_gelu_statistics(dtype):
    kind_b("uf_ln_linear_gelu_fwd", dtype,
           lambda c: {"h1": ops().ln_linear_gelu(c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), c["w1"].cuda(), c["b1"].cuda())})


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_dwconv_linear2_statistics(dtype):
    B, H, W = RA.LNG_MAP

    def run(c):
        x = c["x"].cuda()
        out = ops().dwconv_linear2(c["h1"].cuda().reshape(B, H, W, -1), c["w9"].cuda(), c["bdw"].cuda(), c["w2"].cuda(), c["b2"].cuda(), x)
        return {"dx": out.double() - x.double()}
    kind_b("uf_dwconv_linear2_fwd", dtype, run)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_ffn_statistics(dtype):
    B = RA.LNG_MAP[0]

    def run(c):
        x = c["x"].cuda()
        out = ops().ffn(x.clone(), c["gamma"].cuda(), c["beta"].cuda(), c["w1"].cuda(), c["b1"].cuda(), c["w2"].cuda(), c["b2"].cuda(), None, B=B)
        return {"dx": out.double() - x.double()}
    kind_b("uf_ffn_fwd", dtype, run)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_lewin_block_statistics(dtype):
    def run(case, heads, shift):
        x, _, blk = case
        with torch.no_grad():
            out = blk.cuda()(x.cuda(), None, dtype)
        return {"dx": out.double() - x.cuda().double()}
    kind_b("uf_lewin_block_fwd", dtype, run)
