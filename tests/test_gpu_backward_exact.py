"""GPU: the nonlinear BACKWARD kernels against their float64 reference TO THE BIT, on lattice inputs (tests/backward_lattice.py has the argument, the
constructions, the conditions and the references; tests/test_backward_lattice_reference.py checks them on the CPU).

Through the C ABI.  Sources and destinations are strided views in poisoned allocations wherever the entry point takes a leading dimension, dense
outputs lie between poisoned guard rows and start as NaN (every output here is documented as OVERWRITTEN), workspaces are 0xFF bytes with a guard
behind them.  Every call runs twice and must reproduce its bits.  The gate is assert_exact -- zero differing elements -- with TWO stated exceptions.
(a) the q rows of wqkv / bqkv of uf_lewin_attn_bwd where dq is live sum T-rounded multiples of float32(32^-0.5): held to the float32 summation bound
(M - 1) 2^-24 sum |terms|, from the reference.  (b) behind a GELU' of the sigmoid form at a <= -15, bf16 keeps the 2^-80 residue of the clamp; such an
element is held to backward_lattice.gelu_residue_bound (below 2^-24 of the lattice step, asserted), at most 40 % of any output; a tap gradient of
uf_dwconv3x3_bwd whose reference is 0 is held to backward_lattice.dw9_residue_bound in bf16 (what h = T(GELU(pre)) keeps of that residue).  Per-entry-point counts go to
$UF_REPORT_DIR/parity_backward_exact.json.
"""
import json
import os

import pytest
import torch

import backward_lattice as L
import edge_cases as E
import exact_lattice as X
from edge_cases import PoisonedView
from exact_lattice import BF16, F32, MODES, TAG, assert_exact

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ["uf_window_attention_bwd", "uf_window_attention_bwd_qkv", "uf_rpb_table_grad", "uf_window4_attention_bwd", "uf_rpb4_table_grad", "uf_layernorm_bwd",
                "uf_layernorm_bwd_fused", "uf_layernorm_bwd_cast", "uf_gelu_bwd", "uf_linear_mul_dgelu", "uf_dwconv3x3_mul_dgelu", "uf_dwconv3x3_bwd", "uf_leff_bwd", "uf_lewin_attn_bwd"]
_RAN = set()
RULE_B = {}             # entry point -> elements compared under rule (b)
RULE_A = {}             # entry point -> elements compared under the float32 summation bound


@pytest.fixture(autouse=True)
def _ran(request):
    yield
    _RAN.add(request.node.originalname)


@pytest.fixture(scope="module", autouse=True)
def _dump_report(request):
    yield
    rep = {k: dict(v, under_rule_b=RULE_B.get(k, 0), under_summation_bound=RULE_A.get(k, 0)) for k, v in X.report().items() if k in ENTRY_POINTS}
    out = os.environ.get("UF_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_backward_exact.json"), "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)
    assert all(e["differing"] == 0 for e in rep.values()), {k: v for k, v in rep.items() if v["differing"]}
    mine = {n for n, f in request.module.__dict__.items() if n.startswith("test_") and callable(f)}
    if mine <= _RAN:
        missing = [n for n in ENTRY_POINTS if n not in rep]
        assert not missing, f"every test of this file ran, but these entry points were not compared: {missing}"


class variant:
    """UF_VARIANT for the calls inside the block (None: the key is absent, the shape picks); the selector is read on every call"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("UF_VARIANT")
        if self.value is None:
            os.environ.pop("UF_VARIANT", None)
        else:
            os.environ["UF_VARIANT"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("UF_VARIANT", None)
        else:
            os.environ["UF_VARIANT"] = self.old


def lib():
    from uformer_amd import _lib
    return _lib.load()


def call(name, *args):
    from uformer_amd import _lib
    _lib.check(getattr(_lib.load(), name)(*args), name)
    torch.cuda.synchronize()


def st():
    return torch.cuda.current_stream().cuda_stream


def dt(dtype):
    from uformer_amd import ops
    return ops.uf_dtype(dtype)


def dev(t, dtype=F32):
    """a lattice tensor on the GPU as ``dtype``: the cast must be exact"""
    out = t.to(dtype)
    assert torch.equal(out.double(), t.double()), "lattice value is not representable in the operand type"
    return out.cuda().contiguous()


def view(rows, C, dtype, mode, src=None):
    v = PoisonedView(rows, C, dtype, mode, "cuda")
    return v if src is None else v.fill(dev(src.reshape(rows, C), dtype))


def dense(rows, C, dtype, src=None):
    return view(rows, C, dtype, "guard", src)


class Workspace:
    """0xFF bytes (NaN patterns in every type) with a guard behind them"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf, self.guard = E.poisoned_bytes(self.nbytes, 4096, 0xFF, "cuda")

    def ptr(self):
        return self.buf.data_ptr()

    def guard_intact(self):
        return bool((self.guard == 0xA5).all())


def twice(name, run, refs, dtypes, rule_b=None, rule_a=None):
    """``run`` -> ({key: PoisonedView}, [further views and workspaces]), fresh buffers per call.  Both runs: guards intact; the first against the
    reference, the second against the first.  ``rule_b``: {key: (mask, bound)} -- elements held to a bound instead (rule (b) of the header); ``rule_a``: {key:
    bound} -- the elements with a non-zero bound are held to it (the float32 summation bound of the q rows of wqkv / bqkv, see test_lewin_attn_bwd)"""
    first = None
    for _ in range(2):
        outs, views = run()
        torch.cuda.synchronize()
        for v in list(outs.values()) + views:
            assert v.guard_intact(), f"{name}: wrote outside a view or behind a workspace"
        bits = {k: v.live_bits().cpu() for k, v in outs.items()}
        if first is None:
            first = bits
            for k, v in outs.items():
                got = v.live().reshape(refs[k].shape).cpu()
                if rule_b and k in rule_b:
                    mask, bound = rule_b[k]
                    share = float(mask.double().mean())
                    assert share <= L.RULE_B_CAP, f"{name}/{k}: {share:.2f} of the elements under rule (b)"
                    err = (got.double() - refs[k]).abs()
                    assert bool((err[mask] <= bound[mask]).all()), f"{name}/{k}: a residue of {float(err[mask].max())} exceeds the bound of rule (b)"
                    RULE_B[name.split("/")[0]] = RULE_B.get(name.split("/")[0], 0) + int(mask.sum())
                    got = torch.where(mask, refs[k].to(dtypes[k]), got)
                if rule_a and k in rule_a:
                    bound = rule_a[k].reshape(refs[k].shape)
                    mask = bound > 0
                    err = (got.double() - refs[k]).abs()
                    assert bool((err[mask] <= bound[mask]).all()), f"{name}/{k}: {float((err[mask] / bound[mask]).max())} times the float32 summation bound"
                    RULE_A[name.split("/")[0]] = RULE_A.get(name.split("/")[0], 0) + int(mask.sum())
                    got = torch.where(mask, refs[k].to(dtypes[k]), got)
                assert_exact(f"{name}/{k}", got, refs[k], dtypes[k])
        else:
            for k in bits:
                assert torch.equal(bits[k], first[k]), f"{name}: {k} differs between two runs on the same inputs"


# ---------------------------------------------------------------------------------------------------------------------------
# window attention backward
# ---------------------------------------------------------------------------------------------------------------------------
def attn_id(case):
    B, H, W, heads, hd, shift, kind, masked = case
    return f"{B}x{H}x{W}-h{heads}-hd{hd}-s{shift}-{kind}" + ("-mask" if masked else "")


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("case", L.ATTN_BWD_CASES, ids=attn_id)
def test_window_attention_bwd(dtype, case):
    """uf_window_attention_bwd (dq, dk, dvt, dbias) and uf_window_attention_bwd_qkv (dqkv with the scaled q third, dbias), then uf_rpb_table_grad on the dbias
    the kernel wrote.  The second kernel serves the 2-byte types at head_dim 16 / 32 (its MK = true instantiation with the caller mask), the first one f32
    and every type at head_dim 64."""
    B, H, W, heads, hd, shift, kind, masked = case
    c = L.attn_bwd_case(*case)
    n, C, r = c["n"], heads * hd, c["ref"]
    bias = dev(c["bias"])
    mask = dev(c["caller"]) if masked else None
    nbytes = lib().uf_window_attention_bwd_workspace_bytes(n, heads)
    tag = f"{TAG[dtype]} {attn_id(case)}"

    def operands():
        q, k, vt = (dense(n * 64, C, dtype, c[key]) for key in ("q", "k", "vt"))
        dO = view(n * 64, C, dtype, "strided", c["dO_rows"])
        return q, k, vt, dO, dense(heads * 64, 64, F32), dense(225, heads, F32), Workspace(nbytes)

    def run():
        q, k, vt, dO, dbias, dtab, ws = operands()
        dq, dk, dvt = (dense(n * 64, C, dtype) for _ in range(3))
        call("uf_window_attention_bwd", q.ptr(), k.ptr(), vt.ptr(), bias.data_ptr(), None if mask is None else mask.data_ptr(), 2 if masked else 0, dO.ptr(), dO.ld,
             dq.ptr(), dk.ptr(), dvt.ptr(), dbias.ptr(), n, heads, hd, H, W, shift, dt(dtype), ws.ptr(), nbytes, st())
        call("uf_rpb_table_grad", dbias.ptr(), dtab.ptr(), heads, st())
        return {"dq": dq, "dk": dk, "dvt": dvt, "dbias": dbias, "dtable": dtab}, [q, k, vt, dO, ws]
    twice(f"uf_window_attention_bwd/{tag}", run, {"dq": r["dq"], "dk": r["dk"], "dvt": r["dvt"], "dbias": r["dbias"], "dtable": c["dtable"]},
          {"dq": dtype, "dk": dtype, "dvt": dtype, "dbias": F32, "dtable": F32})
    X.RECORDS[f"uf_rpb_table_grad/{tag}"] = X.RECORDS.pop(f"uf_window_attention_bwd/{tag}/dtable")

    def run_qkv():
        q, k, vt, dO, dbias, dtab, ws = operands()
        dqkv = dense(n * 64, 3 * C, dtype)
        call("uf_window_attention_bwd_qkv", q.ptr(), k.ptr(), vt.ptr(), bias.data_ptr(), None if mask is None else mask.data_ptr(), 2 if masked else 0, dO.ptr(), dO.ld,
             dqkv.ptr(), dbias.ptr(), n, heads, hd, H, W, shift, dt(dtype), ws.ptr(), nbytes, st())
        return {"dqkv": dqkv, "dbias": dbias}, [q, k, vt, dO, ws]
    twice(f"uf_window_attention_bwd_qkv/{tag}", run_qkv, {"dqkv": c["dqkv"], "dbias": r["dbias"]}, {"dqkv": dtype, "dbias": F32})


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,heads,hd,kind", L.ATTN4_BWD_CASES)
def test_window4_attention_bwd(dtype, B, H, W, heads, hd, kind):
    """the 4 x 4-window backward on raster q | k | v rows at row stride 3C + 16, dout and dqkv strided as well; dscore, then uf_rpb4_table_grad on it"""
    c = L.attn4_bwd_case(B, H, W, heads, hd, kind)
    M, C, n = B * H * W, c["C"], c["n"]
    tab = dev(c["tab"])
    tag = f"{TAG[dtype]} {B}x{H}x{W} heads={heads} hd={hd} {kind}"

    def run():
        qkv, dout = view(M, 3 * C, dtype, "strided", c["qkv"]), view(M, C, dtype, "strided", c["dO_rows"])
        dqkv, dscore, dtab = view(M, 3 * C, dtype, "strided"), dense(n * heads * 16, 16, F32), dense(49, heads, F32)
        call("uf_window4_attention_bwd", qkv.ptr(), qkv.ld, tab.data_ptr(), dout.ptr(), dout.ld, dqkv.ptr(), dqkv.ld, dscore.ptr(), B, H, W, C, heads, dt(dtype), st())
        call("uf_rpb4_table_grad", dscore.ptr(), dtab.ptr(), n, heads, st())
        return {"dqkv": dqkv, "dscore": dscore, "dtable": dtab}, [qkv, dout]
    twice(f"uf_window4_attention_bwd/{tag}", run, {"dqkv": c["dqkv"], "dscore": c["dscore"], "dtable": c["dtable"]}, {"dqkv": dtype, "dscore": F32, "dtable": F32})
    X.RECORDS[f"uf_rpb4_table_grad/{tag}"] = X.RECORDS.pop(f"uf_window4_attention_bwd/{tag}/dtable")


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,rows", L.LN_PLAIN_CASES)
def test_layernorm_bwd(C, rows):
    """uf_layernorm_bwd: x and dx in the right half of a concat buffer, dy strided; ragged row counts, and three that exceed the grid (a second trip of the
    grid-stride loop, whose dgamma / dbeta partials the workgroup keeps adding)"""
    c = L.ln_bwd_case(C, rows)
    r = L.ln_bwd_eval(c)
    gm = dev(c["gamma"])
    nbytes = lib().uf_layernorm_bwd_workspace_bytes(rows, C)

    def run():
        x, dy, dx = view(rows, C, F32, "cat", c["x"]), view(rows, C, F32, "strided", c["dy"]), view(rows, C, F32, "cat")
        dg, db, ws = dense(1, C, F32), dense(1, C, F32), Workspace(nbytes)
        call("uf_layernorm_bwd", x.ptr(), x.ld, gm.data_ptr(), dy.ptr(), dy.ld, dx.ptr(), dx.ld, dg.ptr(), db.ptr(), rows, C, ws.ptr(), nbytes, st())
        return {"dx": dx, "dgamma": dg, "dbeta": db}, [x, dy, ws]
    twice(f"uf_layernorm_bwd/C={C} rows={rows}", run, {"dx": r["dx"], "dgamma": r["dgamma"].reshape(1, C), "dbeta": r["dbeta"].reshape(1, C)}, {"dx": F32, "dgamma": F32, "dbeta": F32})


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("C", L.LN_WIDTHS)
def test_layernorm_bwd_fused_and_cast(dtype, C):
    """uf_layernorm_bwd_fused and uf_layernorm_bwd_cast in the forms the block backward uses: dy as T and as f32, in token and in window order (shift 0 / 4),
    the residual gradient ``add`` present and absent, the cast output at the token row and at the window row, DropPath scales absent and (0, 2, 1)"""
    for ci, config in enumerate(L.LN_FUSED_CONFIGS):
        run_ln_config(dtype, C, ci, config)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
def test_layernorm_bwd_cast_second_trip(dtype):
    """more rows than the grid covers in one trip, in the windowed form with T dy, the residual gradient and the window-order cast output with scales"""
    run_ln_config(dtype, L.LN_FUSED_BIG[0], 100, L.LN_FUSED_BIG[1])


def run_ln_config(dtype, C, ci, config):
    """one configuration of uf_layernorm_bwd_fused / uf_layernorm_bwd_cast against backward_lattice.ln_bwd_eval"""
    B, H, W, windowed, shift, add, dy_f32, cast, cast_shift, scaled = config
    M = B * H * W
    c = L.ln_bwd_case(C, M, seed=ci)
    tok = X.window_tokens(B, H, W, shift) if windowed else None
    scales = L.drops(B) if scaled else None
    r = L.ln_bwd_eval(c, tok, add, None if cast is None else (L.cast_rows(B, H, W, cast == "window", cast_shift), scales, H * W), dtype)
    gm = dev(c["gamma"])
    sc = None if scales is None else torch.tensor(scales, dtype=F32, device="cuda")
    dyt = F32 if dy_f32 else dtype
    nbytes = lib().uf_layernorm_bwd_workspace_bytes(M, C)

    def run():
        x, dy, dx = view(M, C, F32, "cat", c["x"]), view(M, C, dyt, "strided", c["dy"]), view(M, C, F32, "cat")
        ad = view(M, C, F32, "cat", c["add"]) if add else None
        dg, db, ws = dense(1, C, F32), dense(1, C, F32), Workspace(nbytes)
        outs = {"dx": dx, "dgamma": dg, "dbeta": db}
        head = (x.ptr(), x.ld, gm.data_ptr(), dy.ptr(), dy.ld, int(dy_f32), None if ad is None else ad.ptr(), dx.ptr(), dx.ld, dg.ptr(), db.ptr(), B, H, W, C, int(windowed), shift, dt(dtype))
        if cast is None:
            call("uf_layernorm_bwd_fused", *head, ws.ptr(), nbytes, st())
        else:
            outs["cast"] = dense(M, C, dtype)
            call("uf_layernorm_bwd_cast", *head, outs["cast"].ptr(), None if sc is None else sc.data_ptr(), int(cast == "window"), cast_shift, ws.ptr(), nbytes, st())
        return outs, [x, dy, ws] + ([ad] if add else [])
    refs = {"dx": r["dx"], "dgamma": r["dgamma"].reshape(1, C), "dbeta": r["dbeta"].reshape(1, C)}
    types = {"dx": F32, "dgamma": F32, "dbeta": F32}
    if cast is not None:
        refs["cast"], types["cast"] = r["cast"], dtype
        assert bool(r["cast"].any())
    name = "uf_layernorm_bwd_fused" if cast is None else "uf_layernorm_bwd_cast"
    twice(f"{name}/{TAG[dtype]} C={C} {B}x{H}x{W} win={int(windowed)} shift={shift} add={int(add)} dyf32={int(dy_f32)} cast={cast}:{cast_shift} scaled={int(scaled)}", run, refs, types)


# ---------------------------------------------------------------------------------------------------------------------------
# GELU'
# ---------------------------------------------------------------------------------------------------------------------------
def rule_b(dtype, pre64, dc64):
    """the elements of a bf16 output behind a GELU' at a <= -15 and their bound; None for the other types (f16 flushes the residue, f32 runs the erf form)"""
    if dtype != BF16:
        return None
    return pre64 <= L.NEG_MAX, L.gelu_residue_bound(dc64, pre64)


def canonical(v, pre64):
    """-0 -> +0 in the live elements of a view that lie behind a GELU' of exactly 0 (pre <= -15, see backward_lattice.nz); every other element and the poison
    around them are left alone"""
    neg = (pre64 <= L.NEG_MAX).reshape(v.view.shape).to(v.view.device)
    v.view.copy_(torch.where(neg, L.nz(v.view), v.view))
    return v


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("n", L.GELU_BWD_N)
def test_gelu_bwd(dtype, n):
    c = L.gelu_bwd_case(n, dtype)

    def run():
        a, dy, dx = dense(n // 8, 8, dtype, c["pre"]), dense(n // 8, 8, dtype, c["dy"]), dense(n // 8, 8, dtype)
        call("uf_gelu_bwd", a.ptr(), dy.ptr(), dx.ptr(), n, dt(dtype), st())
        return {"dx": canonical(dx, c["pre"])}, [a, dy]
    rb = rule_b(dtype, c["pre"], c["dy"])
    twice(f"uf_gelu_bwd/{TAG[dtype]} n={n}", run, {"dx": c["dx"]}, {"dx": dtype}, None if rb is None else {"dx": rb})


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("M,N,K,var", L.LINEAR_DGELU_CASES)
def test_linear_mul_dgelu(dtype, M, N, K, var):
    c = L.linear_dgelu_case(M, N, K, dtype)
    bias = dev(c["bias"])

    def run():
        a, w, pre, out = dense(M, K, dtype, c["A"]), dense(N, K, dtype, c["W"]), dense(M, N, dtype, c["pre"]), dense(M, N, dtype)
        with variant(var):
            call("uf_linear_mul_dgelu", a.ptr(), w.ptr(), bias.data_ptr(), pre.ptr(), out.ptr(), M, N, K, dt(dtype), st())
        return {"out": canonical(out, c["pre"])}, [a, w, pre]
    rb = rule_b(dtype, c["pre"], c["P"])
    twice(f"uf_linear_mul_dgelu/{TAG[dtype]} M={M} N={N} K={K} {var}", run, {"out": c["out"]}, {"out": dtype}, None if rb is None else {"out": rb})


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C", L.DW_BWD_CASES)
def test_dwconv3x3_mul_dgelu(dtype, B, H, W, C):
    c = L.dw_bwd_case(B, H, W, C, dtype)
    M = B * H * W
    w9f = dev(c["w9_flipped"])

    def run():
        dc, pre, out = dense(M, C, dtype, c["dc"]), dense(M, C, dtype, c["pre"]), dense(M, C, dtype)
        call("uf_dwconv3x3_mul_dgelu", dc.ptr(), w9f.data_ptr(), pre.ptr(), out.ptr(), B, H, W, C, dt(dtype), st())
        return {"da": canonical(out, c["pre"])}, [dc, pre]
    rb = rule_b(dtype, c["pre"].reshape(M, C), c["stencil"].reshape(M, C))
    twice(f"uf_dwconv3x3_mul_dgelu/{TAG[dtype]} {B}x{H}x{W} C={C}", run, {"da": c["da"].reshape(M, C)}, {"da": dtype}, None if rb is None else {"da": rb})


def run_dw_bwd(dtype, B, H, W, C, label=""):
    """uf_dwconv3x3_bwd on one lattice case: da (bf16: rule (b) behind a <= -15), dbias at zero, dw9 at zero wherever the reference is non-zero -- the 2^-80 that
    bf16 keeps in h = T(GELU(pre)) at a <= -15 disappears in a float32 sum whose exact part is non-zero -- and held to backward_lattice.dw9_residue_bound where
    the reference is 0"""
    c = L.dw_bwd_case(B, H, W, C, dtype)
    M = B * H * W
    w9f = dev(c["w9_flipped"])
    nbytes = lib().uf_dwconv3x3_bwd_workspace_bytes(C, dt(dtype))

    def run():
        dc, pre, da = dense(M, C, dtype, c["dc"]), dense(M, C, dtype, c["pre"]), dense(M, C, dtype)
        dw9, db, ws = dense(9, C, F32), dense(1, C, F32), Workspace(nbytes)
        call("uf_dwconv3x3_bwd", dc.ptr(), w9f.data_ptr(), pre.ptr(), da.ptr(), dw9.ptr(), db.ptr(), B, H, W, C, dt(dtype), ws.ptr(), nbytes, st())
        return {"da": canonical(da, c["pre"]), "dw9": dw9, "dbias": db}, [dc, pre, ws]
    rb = rule_b(dtype, c["pre"].reshape(M, C), c["stencil"].reshape(M, C))
    rules = None if rb is None else {"da": rb, "dw9": (c["dw9"] == 0, L.dw9_residue_bound(c))}
    twice(f"uf_dwconv3x3_bwd/{TAG[dtype]} {B}x{H}x{W} C={C}{label}", run, {"da": c["da"].reshape(M, C), "dw9": c["dw9"], "dbias": c["dbias"].reshape(1, C)},
          {"da": dtype, "dw9": F32, "dbias": F32}, rules)


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C", L.DW_BWD_CASES)
def test_dwconv3x3_bwd(dtype, B, H, W, C):
    """the one-pass depthwise backward with all three classes in every type: da, and the tap / bias gradients from h = T(GELU(pre)) recomputed in the kernel"""
    run_dw_bwd(dtype, B, H, W, C)


CHUNKED_CASE = (5, 8, 8, 32)
CHUNKED_LIMIT = 2 * 8 * 8 * 32 * 4 + 1          # bytes: two f32 images (chunks of 2, 2, 1), four 2-byte images (4, 1)


def chunked_child():
    """runs in a fresh process whose environment lowers the library's 4 GiB limit (it is read once): the chunks' tap / bias gradients are added in chunk order"""
    assert os.environ.get("UF_DWBWD_MAX_BYTES") == str(CHUNKED_LIMIT)
    for dtype in MODES:
        run_dw_bwd(dtype, *CHUNKED_CASE, label=" chunked")
    rep = X.report()["uf_dwconv3x3_bwd"]
    assert rep["differing"] == 0
    print("chunked ok", rep["cases"], rep["elements"])


def test_dwconv3x3_bwd_chunked():
    """the chunked form of uf_dwconv3x3_bwd (tensors of 4 GiB and more; here the limit is lowered, which only a fresh process can do) on the lattice case, all types"""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_backward_exact as T; T.chunked_child()"
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UF_DWBWD_MAX_BYTES=str(CHUNKED_LIMIT)), capture_output=True, text=True)
    assert out.returncode == 0 and "chunked ok 9 " in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    _, cases, elements = out.stdout.strip().splitlines()[-1].rsplit(" ", 2)
    X.RECORDS["uf_dwconv3x3_bwd/chunked (child process)"] = {"elements": int(elements), "differing": 0}


# ---------------------------------------------------------------------------------------------------------------------------
# the LeFF half of a block
# ---------------------------------------------------------------------------------------------------------------------------
LEFF_GRADS = {"norm2_w": lambda C: (1, C), "norm2_b": lambda C: (1, C), "w1": lambda C: (4 * C, C), "b1": lambda C: (1, 4 * C), "wdw": lambda C: (4 * C, 9),
              "bdw": lambda C: (1, 4 * C), "w2": lambda C: (C, 4 * C), "b2": lambda C: (1, C)}


@pytest.mark.parametrize("dtype", MODES, ids=TAG.get)
@pytest.mark.parametrize("B,H,W,C", L.LEFF_BWD_CASES)
def test_leff_bwd(dtype, B, H, W, C):
    """uf_leff_bwd: the recomputation (LN2, linear1, stencil with the GELU in front of it) and the whole backward chain -- dyT, linear2's gradients, GELU', the one-pass
    depthwise backward, linear1's gradients, LN2's backward with the residual path -- on a construction whose every intermediate is a lattice value: dx1 and all
    eight gradient tensors to the bit, without DropPath scales and with (0, 2, 1)"""
    from uformer_amd import _lib, train
    import ctypes
    M, heads = B * H * W, C // 32
    nbytes = lib().uf_lewin_block_bwd_workspace_bytes(B, H, W, C, heads, dt(dtype))
    for dropped in (False, True):
        c = L.leff_bwd_case(B, H, W, C, dtype, dropped)
        sd = {k: dev(v) for k, v in c["sd"].items()}
        for k in ("mlp.linear1.0.weight", "mlp.linear2.0.weight", "mlp.dwconv.0.weight"):
            assert torch.equal(sd[k].to(dtype).double().cpu(), c["sd"][k]), k
        sd["attn.relative_position_index"] = X.rpb_index(8).cuda()
        pk = train.BlockPack(sd, "", heads, 0, dtype, fused=False)
        tp = pk.train_params
        drop = None if c["drop"] is None else dev(c["drop"])

        def run():
            x1, dy, dx1, ws = dense(M, C, F32, c["x1"]), dense(M, C, F32, c["dy"]), dense(M, C, F32), Workspace(nbytes)
            outs = {k: dense(*shape(C), F32) for k, shape in LEFF_GRADS.items()}
            g = _lib.BlockGrads()
            for k, v in outs.items():
                setattr(g, k, v.ptr())
            outs["dx1"] = dx1
            call("uf_leff_bwd", ctypes.byref(tp), x1.ptr(), dy.ptr(), dx1.ptr(), None if drop is None else drop.data_ptr(), ctypes.byref(g), B, H, W, C, dt(dtype),
                 ws.ptr(), nbytes, st())
            return outs, [x1, dy, ws]
        refs = {k: v.reshape(LEFF_GRADS[k](C)) if k in LEFF_GRADS else v for k, v in c["refs"].items()}
        twice(f"uf_leff_bwd/{TAG[dtype]} {B}x{H}x{W} C={C} drop={dropped}", run, refs, {k: F32 for k in refs})


# ---------------------------------------------------------------------------------------------------------------------------
# the attention half of a block
# ---------------------------------------------------------------------------------------------------------------------------
ATTN_GRADS = {"norm1_w": lambda C, h: (1, C), "norm1_b": lambda C, h: (1, C), "modulator": lambda C, h: (64, C), "rpb_table": lambda C, h: (225, h),
              "wqkv": lambda C, h: (3 * C, C), "bqkv": lambda C, h: (1, 3 * C), "wproj": lambda C, h: (C, C), "bproj": lambda C, h: (1, C)}


def attn_half_tests():
    return [(dtype, case) for dtype in MODES for case in L.attn_half_cases(dtype)]


@pytest.mark.parametrize("dtype,case", attn_half_tests(), ids=[f"{TAG[d]}-{B}x{H}x{W}-C{C}-s{s_}-{kind}-mod{int(m)}" for d, (B, H, W, C, s_, kind, m) in attn_half_tests()])
def test_lewin_attn_bwd(dtype, case):
    """uf_lewin_attn_bwd on the saturated block constructions: the recomputation (LN1 + modulator, q | k | v, the window attention) and the backward chain -- dyw, the
    projection's gradients, dO, the attention backward with its merged output, the bias-table gradient, the q | k | v projection's gradients, dxn, the modulator
    gradient, LN1's backward in window order with the residual path.  Everything to the bit, except the q rows of wqkv / bqkv where dq is live: they sum T-rounded
    multiples of float32(32^-0.5), which no summation order makes exact, and are held to (M - 1) 2^-24 sum |terms| from the reference."""
    from uformer_amd import _lib, train
    import ctypes
    B, H, W, C, shift, kind, use_mod = case
    M, heads = B * H * W, C // 32
    nbytes = lib().uf_lewin_block_bwd_workspace_bytes(B, H, W, C, heads, dt(dtype))
    for dropped in (False, True):
        c = L.attn_half_bwd_case(*case, dtype, dropped)
        sd = {k: dev(v) for k, v in c["sd"].items()}
        for k, v in sd.items():
            if v.dim() == 2 and "table" not in k and "modulator" not in k:
                assert torch.equal(v.to(dtype).double().cpu(), c["sd"][k]), k
        sd["attn.relative_position_index"] = X.rpb_index(8).cuda()
        pk = train.BlockPack(sd, "", heads, shift, dtype, fused=False)
        tp = pk.train_params
        drop = None if c["drop"] is None else dev(c["drop"])
        names = [k for k in ATTN_GRADS if k != "modulator" or use_mod]

        def run():
            x, dx1, dx, ws = dense(M, C, F32, c["x"]), dense(M, C, F32, c["dx1"]), dense(M, C, F32), Workspace(nbytes)
            outs = {k: dense(*ATTN_GRADS[k](C, heads), F32) for k in names}
            g = _lib.BlockGrads()
            for k, v in outs.items():
                setattr(g, k, v.ptr())
            outs["dx"] = dx
            call("uf_lewin_attn_bwd", ctypes.byref(tp), x.ptr(), dx1.ptr(), dx.ptr(), None if drop is None else drop.data_ptr(), ctypes.byref(g), B, H, W, C, dt(dtype),
                 ws.ptr(), nbytes, st())
            return outs, [x, dx1, ws]
        refs = {k: v.reshape(ATTN_GRADS[k](C, heads)) if k in ATTN_GRADS else v for k, v in c["refs"].items()}
        twice(f"uf_lewin_attn_bwd/{TAG[dtype]} {B}x{H}x{W} C={C} shift={shift} {kind} mod={int(use_mod)} drop={dropped}", run, refs, {k: F32 for k in refs}, rule_a=c["bounds"])
