"""GPU: every buildable combination of the model switches against ONE float64 reference.

The rows, the reference and the gates are tests/switch_matrix.py's (tests/test_switch_matrix_reference.py holds them on the CPU: coverage by
enumeration, the reference against every fixture, the gates against stand-in wiring faults, the inputs against bf16 rounding).  Here:

* inference rows: the model in float32 and in the row's 2-byte type, under ``no_grad`` in the row's execution mode, against the reference by the
  whole-model gate of tests/test_gpu_model.py; graph replay / pipelined runs bit-equal to the eager forward; repeated images of a batch bit-equal,
  and the batch bit-equal to the per-image calls; a mask row also runs an all-zero mask against no mask (bit-equal for 'conv', whose window
  attention takes one route; the gate otherwise: the rule of tests/test_gpu_crossmod.py::test_crossmod_model_paths_are_bit_equal);
* training rows: train()-mode forward with drop_path_rate 0 and the backward from the Charbonnier gradient at the reference output; y by the output
  gate, dx and EVERY parameter gradient by tests/test_gpu_bwd.py's gate on the full tensor; a use_checkpoint row against its kept twin in f32;
* UF_BWD_STREAMS = 1 and 3 in fresh child processes against this process's default: sha256 of every gradient tensor identical.

The float64 references are computed once per (form, seed, geometry) at module scope; a JSON report goes under pytest's tmp path."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import switch_matrix as SM
from uformer_amd import infer, model, spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
_REF, _TRAIN_REF, _KEPT_F32, REPORT = {}, {}, {}, {}


def build(form, dtype, sd, **kw):
    m = model.Uformer(compute_dtype=dtype, **form.ctor_kwargs(), **kw)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def gate(name, y, ref, dtype):
    ok, err, ps = SM.output_gate(y, ref, dtype)
    tol = SM.F32_TOL if dtype in (torch.float32, torch.float16) else SM.BF16_TOL
    print(f"{name}: err {err:.3e} (gate {tol:.0e}) psnr {ps:.1f} dB")
    assert ok, (name, err, ps)
    return err


@pytest.fixture(scope="module", autouse=True)
def report(tmp_path_factory):
    yield REPORT
    path = tmp_path_factory.mktemp("switch_matrix") / "report.json"
    path.write_text(json.dumps(REPORT, indent=1, sort_keys=True))
    print(f"\nswitch matrix report: {path}")
    for name, r in REPORT.items():
        print(name, " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in sorted(r.items())))


# ---- inference -----------------------------------------------------------------------------------------------------------------------------------
def infer_reference(name):
    """(row, form, state dict, inputs, float64 reference of the row's distinct images, |float32 reference - float64 reference| of the first)"""
    if name not in _REF:
        row = SM.parse_infer(name)
        form = SM.form_of(row)
        sd, x2, mask, _ = SM.row_inputs(name, row)
        n = 1 if row["B"] == 1 else 2
        with torch.no_grad():
            ref = SM.reference_forward(form, sd, x2[:n], mask)
            r32 = SM.reference_forward(form, sd, x2[:1], mask, dtype=torch.float32)
        _REF[name] = (row, form, sd, x2, mask, ref, (r32.double() - ref[:1]).abs().max().item())
    return _REF[name]


@pytest.mark.parametrize("name", SM.INFER_ROWS)
def test_inference_row(name):
    row, form, sd, x2, mask, ref, dev32 = infer_reference(name)
    B, pattern = row["B"], SM.IMAGE_PATTERN[row["B"]]
    H, W = SM.geometry(row)
    xb = SM.batch_of(x2, B).cuda()
    other = torch.roll(xb, 1, 0) if B > 1 else SM.batch_of(x2[1:], 1).cuda()       # a second batch for the graph / pipelined runs
    refb = ref[list(pattern)]
    mk = mask.cuda() if mask is not None else None
    rec = REPORT.setdefault(name, dict(levels=name, ref_f32_vs_f64=dev32))

    def run(m, x):
        return (m(x, mk) if mk is not None else m(x)).clone()

    for dtype in (F32, SM.DTYPES[row["dt"]]):
        tag = "f32" if dtype is F32 else row["dt"]
        m = build(form, dtype, sd).eval()
        with torch.no_grad():
            y = run(m, xb)
            assert tuple(y.shape) == (B, form.in_chans, H, W)
            rec["err_" + tag] = gate(f"{name}[{tag}]", y, refb, dtype)
            rec["gate_" + tag] = SM.F32_TOL if dtype in (F32, torch.float16) else SM.BF16_TOL
            y_other = run(m, other)
            if row["ex"] == "graph":
                gf = infer.GraphedForward(m, xb)
                assert torch.equal(gf(xb), y), "graph replay differs from the eager forward"
                assert torch.equal(gf(other), y_other) and torch.equal(gf(xb), y)
            elif row["ex"] == "pipe":
                pf = infer.PipelinedForward(m, depth=2)
                outs = list(pf.map([xb, other, xb]))
                assert torch.equal(outs[0], y) and torch.equal(outs[1], y_other) and torch.equal(outs[2], y), "pipelined run differs from the eager forward"
            if B > 1:
                assert not torch.equal(y[0], y[1])
                for i, k in enumerate(pattern):                                      # equal images give equal outputs, wherever they stand in the batch
                    assert torch.equal(y[i], y[pattern.index(k)]), (i, k)
                for i in (0, 1):                                                     # and the batch is the per-image calls, bit for bit
                    assert torch.equal(run(m, xb[i:i + 1]), y[i:i + 1]), i
            if mk is not None:
                plain = m(xb)
                zero = m(xb, torch.zeros_like(mk))
                assert not torch.equal(plain, y), "the mask changed nothing"
                if form.proj == "conv":
                    assert torch.equal(zero, plain), "an all-zero mask changed the output of a 'conv' model"
                else:
                    gate(f"{name}[{tag}] zero mask", zero, plain.cpu(), dtype)
        del m


# ---- training ------------------------------------------------------------------------------------------------------------------------------------
def base_of(name):
    return name.rsplit("-", 1)[0]


def train_reference(name):
    key = base_of(name)
    if key not in _TRAIN_REF:
        _TRAIN_REF.clear()                                                           # one configuration at a time: kept then ckpt follow each other
        row = SM.parse_train(name)
        form = SM.form_of(row)
        sd, x2, _, t2 = SM.row_inputs(name, row)
        x, target = SM.batch_of(x2, row["B"]), SM.batch_of(t2, row["B"])
        y, loss, dx, grads = SM.reference_grads(form, sd, x, target)
        with torch.no_grad():
            r32 = SM.reference_forward(form, sd, x[:1], dtype=torch.float32)
        _TRAIN_REF[key] = (row, (form, sd), x, target, y, dx, grads, (r32.double() - y[:1]).abs().max().item())
    return _TRAIN_REF[key]


def run_training(name, dtype, inputs=None):
    """(y, dx, {name: gradient}) of the train()-mode forward and the backward from d loss / d y at the REFERENCE output, loss scale undone"""
    (form, sd), x, target, y_ref = inputs if inputs is not None else train_reference(name)[1:5]
    m = build(form, dtype, sd, drop_path_rate=0.0, use_checkpoint=SM.parse_train(name)["ckpt"] == "ckpt").train()
    xg = x.cuda().requires_grad_(True)
    y = m(xg)
    assert y.grad_fn is not None
    ls = SM.F16_LOSS_SCALE if dtype == torch.float16 else 1.0
    y.backward(SM.charbonnier_dy(y_ref, target).cuda() * ls)
    torch.cuda.synchronize()
    grads = {}
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        grads[n] = (p.grad / ls).float().cpu()
    return y.detach().float().cpu(), (xg.grad / ls).float().cpu(), grads


def worst_grad(dx, grads, dx_ref, grads_ref):
    worst = (SM.grad_rel(dx, dx_ref), "dx")
    for n in grads_ref:
        worst = max(worst, (SM.grad_rel(grads[n], grads_ref[n]), n))
    return worst


@pytest.mark.parametrize("name", SM.TRAIN_ROWS)
def test_training_row(name):
    row, _, x, target, y_ref, dx_ref, g_ref, dev32 = train_reference(name)
    rec = REPORT.setdefault(name, dict(levels=name, ref_f32_vs_f64=dev32))
    for dtype in (F32, SM.DTYPES[row["dt"]]):
        tag = "f32" if dtype is F32 else row["dt"]
        y, dx, grads = run_training(name, dtype)
        rec["err_" + tag] = gate(f"{name}[{tag}] y", y, y_ref, dtype)
        assert sorted(grads) == sorted(g_ref), sorted(set(grads) ^ set(g_ref))
        worst = worst_grad(dx, grads, dx_ref, g_ref)
        rec["grad_" + tag], rec["grad_gate_" + tag], rec["grad_worst_" + tag] = worst[0], SM.GRAD_RTOL[dtype], worst[1]
        print(f"{name}[{tag}]: worst gradient {worst[0]:.3e} x max|g_ref| at {worst[1]} (gate {SM.GRAD_RTOL[dtype]:.0e})")
        assert worst[0] <= SM.GRAD_RTOL[dtype], worst
        if dtype is F32:
            if name.endswith("-kept"):
                _KEPT_F32.clear()
                _KEPT_F32[base_of(name)] = (dx, grads)
            else:
                if base_of(name) not in _KEPT_F32:                                   # the ckpt row run on its own
                    _, kdx, kgr = run_training(base_of(name) + "-kept", F32)
                    _KEPT_F32[base_of(name)] = (kdx, kgr)
                kdx, kgr = _KEPT_F32.pop(base_of(name))
                twin = worst_grad(dx, grads, kdx, kgr)
                rec["grad_f32_vs_kept"] = twin[0]
                print(f"{name}[f32]: against the kept form {twin[0]:.3e} at {twin[1]}")
                assert twin[0] <= SM.GRAD_RTOL[F32], twin


# ---- backward stream counts ----------------------------------------------------------------------------------------------------------------------
STREAM_ROWS = ["e32-128x128-leff-lin-nox-d4c4-nomod-B3-bf16-kept",        # LeFF, every intermediate kept: train.py's _Side
               "e32-128x128-leff-lin-nox-d4c4-nomod-B3-bf16-ckpt"]        # recompute_fused (head_dim 32, LeFF, 2-byte operands): uf_lewin_block_bwd's Queues


def grad_hashes(name):
    """sha256 of y, dx and every parameter gradient (the raw bytes of the float32 tensors) of the row in its 2-byte type"""
    row = SM.parse_train(name)
    form = SM.form_of(row)
    sd, x2, _, t2 = SM.row_inputs(name, row)
    with torch.no_grad():                                                            # the forward alone: all the backward needs is d loss / d y
        y_ref = SM.reference_forward(form, sd, x2)[list(SM.IMAGE_PATTERN[row["B"]])]
    y, dx, grads = run_training(name, SM.DTYPES[row["dt"]], ((form, sd), SM.batch_of(x2, row["B"]), SM.batch_of(t2, row["B"]), y_ref))
    out = {"y": y, "dx": dx, **grads}
    return {k: hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() for k, v in out.items()}


def print_grad_hashes(name):
    for k, v in grad_hashes(name).items():
        print(f"HASH {k} {v}")


@pytest.mark.parametrize("name", STREAM_ROWS)
def test_backward_stream_counts_give_identical_gradients(name):
    """The kernels hold no atomics and UF_BWD_STREAMS only chooses the stream a weight-gradient job is enqueued on, so 1 (none), the default (one
    side stream) and 3 (jobs alternate over two) must give the same bits; a difference is a missing ordering edge in _Side / Queues."""
    assert name in SM.TRAIN_ROWS
    assert os.environ.get("UF_BWD_STREAMS") in (None, "2"), "this process must run the default"
    want = grad_hashes(name)
    assert len(want) > 100
    code = (f"import sys; sys.path[:0] = [{REPO!r}, {os.path.join(REPO, 'tests')!r}]; import test_gpu_switch_matrix as T; T.print_grad_hashes({name!r})")
    for n in ("1", "3"):
        env = dict(os.environ, UF_BWD_STREAMS=n)
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("HASH "))
        assert sorted(got) == sorted(want)
        diff = [k for k in want if got[k] != want[k]]
        assert not diff, (f"UF_BWD_STREAMS={n}", diff[:8])
