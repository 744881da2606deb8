"""GPU: the launchers at their real size limits -- tensors of 4 GiB / 2^31 elements and more -- through the C ABI (tests/large_tensor.py
has the inventory of the predicates, the planner and the two comparisons, tests/test_large_tensor_reference.py checks them on the CPU).

Every `form` / `chunk` predicate runs just under it, at it (the first shape for which it is false) and one image beyond it; the entry points without
a predicate run once past 2^32 bytes.  Operations local to an image are compared, over the whole tensor and bit for bit, with the same entry point
run on chunks of whole images through offset pointers; reductions over the rows run on the sparse lattice against a float64 sum over the
planner's blocks.  No tolerance appears in this file.  Batches are built from images of 2^25 / 2^26 bytes, so that chunk seams and boundaries fall
between images of one batch.

No test holds more than 24 GiB of device memory (asserted from the allocator's peak); a test that needs more than is free at its start skips with
both numbers.  Inputs are filled in place on the GPU, nothing large moves to the host.  Figures go to $UF_REPORT_DIR/parity_large.json.
"""
import gc
import json
import os
import time

import pytest
import torch

import exact_lattice as X
import large_tensor as LT
from exact_lattice import BF16, F32, TAG
from large_tensor import B32

pytestmark = pytest.mark.gpu

CASES = []               # the report: one entry per test
_RAN = set()


def L():
    from uformer_amd import _lib
    return _lib.load()


def call(name, *args):
    from uformer_amd import _lib
    _lib.check(getattr(L(), name)(*args), name)
    torch.cuda.synchronize()


def status(name, *args):
    rc = getattr(L(), name)(*args)
    torch.cuda.synchronize()
    return rc


def st():
    return torch.cuda.current_stream().cuda_stream


def dt(dtype):
    from uformer_amd import _lib
    return {F32: _lib.UF_F32, BF16: _lib.UF_BF16}[dtype]


def esz(dtype):
    return 4 if dtype == F32 else 2


def at(t, elems=0):
    """device address of element ``elems`` of t"""
    return t.data_ptr() + elems * t.element_size()


def empty(n, dtype):
    return torch.empty(n, dtype=dtype, device="cuda")


def out_buf(n, dtype):
    return LT.guarded(n, dtype, "cuda")


def small(values, dtype=F32):
    return torch.as_tensor(values, dtype=torch.float64).to(dtype).cuda().contiguous()


@pytest.fixture(autouse=True)
def case(request):
    """case(entry_points, predicate, shape, need_bytes): declares what the test holds, skips when the device has less free; afterwards everything is
    freed, the cache emptied and the allocator's peak held to the 24 GiB cap.  The test's figures go to the report."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    torch.manual_seed(20260)
    free = torch.cuda.mem_get_info()[0]
    entry = {"test": request.node.name, "status": "ran", "free_bytes": free}
    CASES.append(entry)
    first_record = set(X.RECORDS)
    t0 = time.time()

    def declare(entry_points, predicate, shape, need_bytes):
        entry.update(entry_points=list(entry_points), predicate=predicate, shape=shape, bytes=int(need_bytes))
        assert need_bytes <= LT.MEMORY_CAP, f"the case needs {need_bytes} bytes, over the cap: reshape it or list it as not run"
        if need_bytes > free:
            entry["status"] = "skipped"
            pytest.skip(f"needs {need_bytes} bytes of device memory, {free} are free")
    yield declare
    torch.cuda.synchronize()
    entry["seconds"] = round(time.time() - t0, 3)
    mine = {k: v for k, v in X.RECORDS.items() if k not in first_record}
    entry["elements"] = sum(v["elements"] for v in mine.values())
    entry["differing"] = sum(v["differing"] for v in mine.values())
    entry["peak_bytes"] = torch.cuda.max_memory_allocated()
    gc.collect()
    torch.cuda.empty_cache()
    if entry["status"] == "ran":                    # a case that skipped on free memory has run nothing: it counts neither as run nor as covering its entry points
        _RAN.add(request.node.originalname)
    assert entry["peak_bytes"] <= LT.MEMORY_CAP, f"held {entry['peak_bytes']} bytes of device memory, the cap is {LT.MEMORY_CAP}"


@pytest.fixture(scope="module", autouse=True)
def _report(request):
    yield
    ran = [c for c in CASES if c["status"] == "ran"]
    rep = {"cases": CASES, "ran": len(ran), "skipped": len(CASES) - len(ran), "differing": sum(c.get("differing", 0) for c in ran),
           "wall_seconds": round(sum(c.get("seconds", 0) for c in CASES), 2), "slowest": max(CASES, key=lambda c: c.get("seconds", 0))["test"] if CASES else None,
           "not_run": [{"entry_points": r["entry_points"], "predicate": r["predicate"], "reason": r["run"]} for r in LT.INVENTORY if r["run"] is not True]}
    out = os.environ.get("UF_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_large.json"), "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)
    assert rep["differing"] == 0, [c for c in ran if c.get("differing")]
    # when every test function of this file was selected and has run, every entry point the inventory marks as run is in the report
    mine = {n for n, f in request.module.__dict__.items() if n.startswith("test_") and callable(f)}
    if mine <= _RAN:
        seen = {e for c in ran for e in c.get("entry_points", [])}
        missing = [e for e in LT.entry_points(True) if e not in seen]
        assert not missing, f"every test of this file ran, but these entry points of the inventory were not: {missing}"


# ---------------------------------------------------------------------------------------------------------------------------
# the depthwise 3x3 family: launch_dwconv's walking / one-column forms, and uf_dwconv3x3_mul_dgelu
# ---------------------------------------------------------------------------------------------------------------------------
DW_H, DW_W, DW_C = 256, 256, 256                       # the LeFF hidden tensor of the last decoder stage of Uformer-B (C = 64): 2^26 bytes per image in f32
DW_PER = DW_H * DW_W * DW_C
# (type, images): under the predicate, at it (exactly 2^32 bytes), one image beyond it
DW_SIZES = [(F32, 63), (F32, 64), (F32, 65), (BF16, 127), (BF16, 128), (BF16, 129)]
DW_IDS = [f"{TAG[d]}-{b}" for d, b in DW_SIZES]
DW_PREDICATE = "launch_dwconv: B*H*W*C*sizeof(T) < 0xffffffff"
# entry point -> (number of M-sized inputs, number of M-sized outputs)
DW_ENTRIES = {"uf_dwconv3x3_fwd": (1, 1), "uf_dwconv3x3_gelu_fwd": (1, 1), "uf_dwconv3x3_pre_gelu_fwd": (1, 2), "uf_dwconv3x3_gelu_in_pre_gelu_fwd": (1, 2), "uf_dwconv3x3_mul_dgelu": (2, 1)}


def dw_taps():
    g = torch.Generator().manual_seed(11)
    w9 = torch.randint(-2, 3, (9, DW_C), generator=g).double()
    w9[w9 == 0] = 1.0
    bias = torch.randint(-2, 3, (DW_C,), generator=g).double()
    return w9, bias


def dw_call(entry, ins, outs, w9, bias, nb, dtype):
    a = (nb, DW_H, DW_W, DW_C)
    if entry == "uf_dwconv3x3_fwd":
        call(entry, ins[0], w9.data_ptr(), bias.data_ptr(), outs[0], *a, 0, dt(dtype), st())
    elif entry == "uf_dwconv3x3_gelu_fwd":
        call(entry, ins[0], w9.data_ptr(), bias.data_ptr(), outs[0], *a, dt(dtype), st())
    elif entry == "uf_dwconv3x3_mul_dgelu":
        call(entry, ins[0], w9.data_ptr(), ins[1], outs[0], *a, dt(dtype), st())
    else:
        call(entry, ins[0], w9.data_ptr(), bias.data_ptr(), outs[0], outs[1], *a, dt(dtype), st())


@pytest.mark.parametrize("dtype,B", DW_SIZES, ids=DW_IDS)
@pytest.mark.parametrize("entry", list(DW_ENTRIES))
def test_dwconv_forms(case, entry, dtype, B):
    """B x 256 x 256 x 256 through one entry point of the depthwise family against the same entry point on chunks of 2^29 bytes; the bare stencil
    (uf_dwconv3x3_fwd, linear) also against float64 on the planner's images"""
    n_in, n_out = DW_ENTRIES[entry]
    n = B * DW_PER
    chunk = LT.chunk_images([DW_PER * esz(dtype)])
    case([entry], DW_PREDICATE if entry != "uf_dwconv3x3_mul_dgelu" else "none (always the one-column form)", f"{B}x{DW_H}x{DW_W}x{DW_C} {TAG[dtype]}",
         (n_in + n_out) * n * esz(dtype) + n_out * chunk * DW_PER * esz(dtype) + (1 << 28))
    w9_64, bias_64 = dw_taps()
    w9, bias = small(w9_64), small(bias_64)
    ins = [LT.fill_odd(empty(n, dtype), 3)]
    if n_in == 2:
        ins.append(LT.fill_range(empty(n, dtype), -4, 4))                    # the pre-activation GELU' is taken of
    outs = [out_buf(n, dtype) for _ in range(n_out)]
    dw_call(entry, [at(t) for t in ins], [at(t) for t in outs], w9, bias, B, dtype)
    assert all(LT.tail_intact(o, n) for o in outs), "the large call wrote behind its output"
    scratch = [out_buf(chunk * DW_PER, dtype) for _ in range(n_out)]

    def run_chunk(b0, nb):
        dw_call(entry, [at(t, b0 * DW_PER) for t in ins], [at(s) for s in scratch], w9, bias, nb, dtype)
        assert all(LT.tail_intact(s, chunk * DW_PER) for s in scratch)
        return [s[:nb * DW_PER] for s in scratch]
    tag = f"{entry}/{TAG[dtype]}/B{B}"
    LT.compare_chunks(tag + "/chunks", [o[:n] for o in outs], DW_PER, B, chunk, run_chunk)
    if entry == "uf_dwconv3x3_fwd":
        p = LT.plan(B * DW_H * DW_W, DW_C, esz(dtype), DW_H * DW_W)
        for b in p["blocks"]:
            ref = LT.dwconv64(ins[0][b * DW_PER:(b + 1) * DW_PER].view(1, DW_H, DW_W, DW_C), w9_64.cuda(), bias_64.cuda())
            LT.assert_exact_device(f"{tag}/float64 image {b}", outs[0][b * DW_PER:(b + 1) * DW_PER], ref.reshape(-1), dtype)


def dw_sparse(B, dtype, seams=()):
    """dc in {-1, 1} and pre-activations in 8..15 (T(GELU(a)) = a, GELU'(a) = 1 there: backward_lattice) on the planner's images, zero elsewhere;
    the float64 tap / bias gradients of those images"""
    n = B * DW_PER
    p = LT.plan(B * DW_H * DW_W, DW_C, esz(dtype), DW_H * DW_W, extra=seams)
    dc = LT.fill_sparse(empty(n, dtype), DW_PER, p["blocks"], lambda v: LT.fill_odd(v, 1))
    pre = LT.fill_sparse(empty(n, dtype), DW_PER, p["blocks"], lambda v: LT.fill_range(v, 8, 15))
    LT.check_sparse_sum(len(p["blocks"]) * DW_H * DW_W, 15, 1)
    dw9 = torch.zeros(9, DW_C, dtype=torch.float64, device="cuda")
    db = torch.zeros(DW_C, dtype=torch.float64, device="cuda")
    for b in p["blocks"]:
        v = slice(b * DW_PER, (b + 1) * DW_PER)
        g, s = LT.dw_grads64(dc[v].view(1, DW_H, DW_W, DW_C), pre[v].view(1, DW_H, DW_W, DW_C))
        dw9 += g
        db += s
    assert bool(dw9.any(1).all()) and bool(db.any())
    return p, dc, pre, dw9, db


@pytest.mark.parametrize("dtype,B", DW_SIZES, ids=DW_IDS)
def test_dwconv3x3_bwd_chunked_walk(case, dtype, B):
    """uf_dwconv3x3_bwd at its real limit (chunks of at most 63 f32 / 127 bf16 images): da against the entry point on chunks of 2^29 bytes; dw9 / dbias on
    the sparse lattice with non-zero images in the first chunk, in the last one and on both sides of the seam"""
    n = B * DW_PER
    chunk = LT.chunk_images([DW_PER * esz(dtype)])
    case(["uf_dwconv3x3_bwd"], "chunks of whole images under 0xffffffff bytes", f"{B}x{DW_H}x{DW_W}x{DW_C} {TAG[dtype]}", 3 * n * esz(dtype) + chunk * DW_PER * esz(dtype) + (1 << 28))
    w9_64, _ = dw_taps()
    w9f = small(w9_64.flip(0))
    nbytes = L().uf_dwconv3x3_bwd_workspace_bytes(DW_C, dt(dtype))
    ws = out_buf(nbytes // 4, F32)
    dw9, db = out_buf(9 * DW_C, F32), out_buf(DW_C, F32)

    def run(dc_p, pre_p, da_p, nb):
        call("uf_dwconv3x3_bwd", dc_p, w9f.data_ptr(), pre_p, da_p, dw9.data_ptr(), db.data_ptr(), nb, DW_H, DW_W, DW_C, dt(dtype), ws.data_ptr(), nbytes, st())
        assert LT.tail_intact(ws, nbytes // 4) and LT.tail_intact(dw9, 9 * DW_C) and LT.tail_intact(db, DW_C)
    tag = f"uf_dwconv3x3_bwd/{TAG[dtype]}/B{B}"
    dc, pre, da = LT.fill_odd(empty(n, dtype), 1), LT.fill_range(empty(n, dtype), -4, 4), out_buf(n, dtype)
    run(at(dc), at(pre), at(da), B)
    assert LT.tail_intact(da, n)
    scratch = out_buf(chunk * DW_PER, dtype)

    def run_chunk(b0, nb):
        run(at(dc, b0 * DW_PER), at(pre, b0 * DW_PER), at(scratch), nb)
        assert LT.tail_intact(scratch, chunk * DW_PER)
        return scratch[:nb * DW_PER]
    LT.compare_chunks(tag + "/da chunks", da[:n], DW_PER, B, chunk, run_chunk)
    del dc, pre
    # the launcher's own chunks: (0xffffffff - 1) // per-image bytes images each
    own = (0xffffffff - 1) // (DW_PER * esz(dtype))
    seams = [s for b0 in range(own, B, own) for s in (b0 - 1, b0)]
    p, dc, pre, dw9_ref, db_ref = dw_sparse(B, dtype, seams)
    assert B <= own or {own - 1, own} <= set(p["blocks"])
    run(at(dc), at(pre), at(da), B)
    LT.assert_exact_device(tag + "/dw9 sparse", dw9[:9 * DW_C], dw9_ref.reshape(-1), F32)
    LT.assert_exact_device(tag + "/dbias sparse", db[:DW_C], db_ref, F32)


def test_dwconv3x3_wgrad_under_its_refusal(case):
    """uf_dwconv3x3_wgrad at 127 x 256 x 256 x 256 bf16, the largest whole-image shape under 2^31 - 1 elements, on the sparse lattice; 128 images are refused"""
    dtype, B = BF16, 128
    n = B * DW_PER
    case(["uf_dwconv3x3_wgrad"], "refuses B*H*W*C >= 2^31 - 1", f"127 and 128 x {DW_H}x{DW_W}x{DW_C} bf16", 2 * n * 2 + (1 << 28))
    nbytes = L().uf_dwconv3x3_wgrad_workspace_bytes(DW_C, dt(dtype))
    ws = out_buf(nbytes // 4, F32)
    dw9, db = out_buf(9 * DW_C, F32), out_buf(DW_C, F32)
    p, dc, h, dw9_ref, db_ref = dw_sparse(B - 1, dtype)
    call("uf_dwconv3x3_wgrad", at(h), at(dc), dw9.data_ptr(), db.data_ptr(), B - 1, DW_H, DW_W, DW_C, dt(dtype), ws.data_ptr(), nbytes, st())
    assert LT.tail_intact(ws, nbytes // 4) and LT.tail_intact(dw9, 9 * DW_C) and LT.tail_intact(db, DW_C)
    LT.assert_exact_device("uf_dwconv3x3_wgrad/bf16/B127/dw9 sparse", dw9[:9 * DW_C], dw9_ref.reshape(-1), F32)
    LT.assert_exact_device("uf_dwconv3x3_wgrad/bf16/B127/dbias sparse", db[:DW_C], db_ref, F32)
    del dc, h
    dc, h = empty(n, dtype).zero_(), empty(n, dtype).zero_()           # real allocations of the refused size behind every pointer
    assert status("uf_dwconv3x3_wgrad", at(h), at(dc), dw9.data_ptr(), db.data_ptr(), B, DW_H, DW_W, DW_C, dt(dtype), ws.data_ptr(), nbytes, st()) == X.UF_ERR_SHAPE


# ---------------------------------------------------------------------------------------------------------------------------
# uf_output_proj_fwd: the LDS-DMA form, the first form, the refusal
# ---------------------------------------------------------------------------------------------------------------------------
OP_H, OP_W, OP_C2 = 512, 512, 32                       # 2^25 bytes of token rows per image


def output_proj_setup(B):
    per_x, per_o = OP_H * OP_W * OP_C2, 3 * OP_H * OP_W
    g = torch.Generator().manual_seed(13)
    w = small(torch.randint(-2, 3, (3 * 9 * OP_C2,), generator=g).double())
    bias = small([1.0, -2.0, 3.0])
    x = LT.fill_odd(empty(B * per_x, F32), 3)
    img = LT.fill_range(empty(B * per_o, F32), -8, 8)
    return per_x, per_o, w, bias, x, img


@pytest.mark.parametrize("B", [127, 128, 129, 511])
def test_output_proj_forms(case, B):
    """uf_output_proj_fwd (f32) around B*H*W*ld_x*4 = 0xffffff00 -- 127 images take the LDS-DMA form, 128 (2^32 bytes) and 129 the first form -- and at 511
    images, the largest whole-image batch under the refusal at 2^32 - 1 elements; against the entry point on chunks of 16 images (the two forms are
    documented bit-identical)"""
    per_x, per_o = OP_H * OP_W * OP_C2, 3 * OP_H * OP_W
    chunk = LT.chunk_images([per_x * 4])
    case(["uf_output_proj_fwd"], "LDS-DMA form iff B*H*W*ld_x*4 < 0xffffff00; refuses B*H*W*ld_x >= 2^32 - 1", f"{B}x{OP_H}x{OP_W}x{OP_C2} f32", B * (per_x + 2 * per_o) * 4 + chunk * per_o * 4 + (1 << 28))
    per_x, per_o, w, bias, x, img = output_proj_setup(B)
    out = out_buf(B * per_o, F32)
    call("uf_output_proj_fwd", at(x), OP_C2, w.data_ptr(), bias.data_ptr(), at(img), at(out), B, OP_H, OP_W, OP_C2, 1, st())
    assert LT.tail_intact(out, B * per_o)
    scratch = out_buf(chunk * per_o, F32)

    def run_chunk(b0, nb):
        call("uf_output_proj_fwd", at(x, b0 * per_x), OP_C2, w.data_ptr(), bias.data_ptr(), at(img, b0 * per_o), at(scratch), nb, OP_H, OP_W, OP_C2, 1, st())
        assert LT.tail_intact(scratch, chunk * per_o)
        return scratch[:nb * per_o]
    LT.compare_chunks(f"uf_output_proj_fwd/f32/B{B}/chunks", out[:B * per_o], per_o, B, chunk, run_chunk)


def test_output_proj_refuses_two_to_the_32_elements(case):
    """512 x 512 x 512 rows of 32 floats are 2^32 elements: UF_ERR_SHAPE, with allocations of that size behind every pointer"""
    B = 512
    per_x, per_o = OP_H * OP_W * OP_C2, 3 * OP_H * OP_W
    case(["uf_output_proj_fwd"], "refuses B*H*W*ld_x >= 2^32 - 1", f"{B}x{OP_H}x{OP_W}x{OP_C2} f32", B * (per_x + 2 * per_o) * 4 + (1 << 28))
    x, img, out = empty(B * per_x, F32), empty(B * per_o, F32), out_buf(B * per_o, F32)
    w, bias = small([1.0] * (27 * OP_C2)), small([0.0] * 3)
    assert status("uf_output_proj_fwd", at(x), OP_C2, w.data_ptr(), bias.data_ptr(), at(img), at(out), B, OP_H, OP_W, OP_C2, 1, st()) == X.UF_ERR_SHAPE
    X.RECORDS["uf_output_proj_fwd/refusal"] = {"elements": 0, "differing": 0}


# ---------------------------------------------------------------------------------------------------------------------------
# uf_linear_fwd: LDS-DMA staging iff M * lda * 2 < 0xffffff00
# ---------------------------------------------------------------------------------------------------------------------------
LIN_N, LIN_K, LIN_BLOCK = 64, 512, 32768               # a row block of the activation is 2^25 bytes
LIN_AT = 4194304                                       # M * 512 * 2 = 2^32: the first M for which the predicate is false


@pytest.mark.parametrize("M", [LIN_AT - 1, LIN_AT, LIN_AT + LIN_BLOCK], ids=["under", "at", "beyond"])
def test_linear_fwd_dma_limit(case, M):
    """bf16 A[M][512] W[64][512]^T: M = 4194303 takes the LDS-DMA staging (4 GiB - 1 KiB of activations), 4194304 and more the register staging.  Odd
    integers in [-3, 3] against +-1 weights: every sum is exact in float32, so both stagings return float64 rounded once -- checked on the planner's row
    blocks -- and the large call equals the entry point on chunks of 16 row blocks bit for bit"""
    dtype = BF16
    assert ((LIN_AT - 1) * LIN_K * 2 < 0xffffff00) and not (LIN_AT * LIN_K * 2 < 0xffffff00)
    B = (M + LIN_BLOCK - 1) // LIN_BLOCK
    chunk = LT.chunk_images([LIN_BLOCK * LIN_K * 2])
    case(["uf_linear_fwd"], "LDS-DMA staging iff M*lda*2 < 0xffffff00", f"M={M} N={LIN_N} K={LIN_K} bf16", M * (LIN_K + LIN_N) * 2 + chunk * LIN_BLOCK * LIN_N * 2 + (1 << 28))
    g = torch.Generator().manual_seed(17)
    W64 = (torch.randint(0, 2, (LIN_N, LIN_K), generator=g) * 2 - 1).double()
    b64 = torch.randint(-3, 4, (LIN_N,), generator=g).double()
    W, bias = small(W64, dtype), small(b64)
    A = LT.fill_odd(empty(M * LIN_K, dtype), 3)
    X.check_accumulation(LIN_K, (3,), addend_steps=3)
    out = out_buf(M * LIN_N, dtype)
    call("uf_linear_fwd", at(A), W.data_ptr(), bias.data_ptr(), at(out), M, LIN_N, LIN_K, 0, dt(dtype), st())
    assert LT.tail_intact(out, M * LIN_N)
    scratch = out_buf(chunk * LIN_BLOCK * LIN_N, dtype)

    def run_chunk(b0, nb):
        rows = min(nb * LIN_BLOCK, M - b0 * LIN_BLOCK)
        call("uf_linear_fwd", at(A, b0 * LIN_BLOCK * LIN_K), W.data_ptr(), bias.data_ptr(), at(scratch), rows, LIN_N, LIN_K, 0, dt(dtype), st())
        assert LT.tail_intact(scratch, chunk * LIN_BLOCK * LIN_N)
        return scratch[:rows * LIN_N]
    tag = f"uf_linear_fwd/bf16/M{M}"
    LT.compare_chunks(tag + "/chunks", out[:M * LIN_N], LIN_BLOCK * LIN_N, B, chunk, run_chunk, total=M * LIN_N)
    p = LT.plan(M, LIN_K, 2, LIN_BLOCK)
    for b in p["blocks"]:
        a = LT.block_rows_of(A, LIN_K, LIN_BLOCK, b, M)
        ref = a.double() @ W64.cuda().t() + b64.cuda()
        LT.assert_exact_device(f"{tag}/float64 block {b}", LT.block_rows_of(out, LIN_N, LIN_BLOCK, b, M), ref, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# uf_linear_wgrad: the DMA versions iff (M + 64) * ldy * 2 and (M + 64) * ldx * 2 are both under 0xffffff00
# ---------------------------------------------------------------------------------------------------------------------------
WG_BLOCK = 65536
# name: (N, K, ldy, ldx, first M for which the predicate is false)
WG_CONFIGS = {"v3 both": (128, 128, 128, 128, 16777151), "v3 ldy": (128, 128, 256, 128, 8388544), "v3 ldx": (128, 128, 128, 256, 8388544), "v4 both": (512, 512, 512, 512, 4194240)}


@pytest.mark.parametrize("where", ["under", "at", "beyond"])
@pytest.mark.parametrize("cfg", list(WG_CONFIGS))
def test_linear_wgrad_dma_limit(case, cfg, where):
    """bf16 dW = dY^T X, db = sum dY across the limit of the LDS-DMA versions (third: 128-wide tiles; fourth: N, K multiples of 256) in both operands, in
    dY alone (ldy = 2 N) and in X alone, on the sparse lattice: non-zero row blocks of 65536 rows where the planner puts them for EITHER operand (pad
    columns included: nothing may read them), float64 reference over those blocks"""
    dtype = BF16
    N, K, ldy, ldx, at_m = WG_CONFIGS[cfg]
    assert (at_m - 1 + 64) * max(ldy, ldx) * 2 < 0xffffff00 <= (at_m + 64) * max(ldy, ldx) * 2
    M = {"under": at_m - 1, "at": at_m, "beyond": at_m + WG_BLOCK}[where]
    nbytes = L().uf_linear_wgrad_workspace_bytes(M, N, K)
    case(["uf_linear_wgrad"], "DMA versions iff (M+64)*ldy*2 and (M+64)*ldx*2 < 0xffffff00", f"{cfg}: M={M} N={N} K={K} ldy={ldy} ldx={ldx} bf16", M * (ldy + ldx) * 2 + nbytes + (1 << 28))
    py, px = LT.plan(M, ldy, 2, WG_BLOCK), LT.plan(M, ldx, 2, WG_BLOCK)
    blocks = sorted(set(py["blocks"]) | set(px["blocks"]))
    assert where != "beyond" or ("byte", B32) in (py["marks"] if ldy >= ldx else px["marks"])       # under / at: the operand ends (M + 64 rows) short of 2^32 bytes
    dY = LT.fill_sparse(empty(M * ldy, dtype), WG_BLOCK * ldy, blocks, lambda v: LT.fill_odd(v, 1))
    Xa = LT.fill_sparse(empty(M * ldx, dtype), WG_BLOCK * ldx, blocks, lambda v: LT.fill_odd(v, 3))
    LT.check_sparse_sum(len(blocks) * WG_BLOCK, 1, 3)
    dW_ref = torch.zeros(N, K, dtype=torch.float64, device="cuda")
    db_ref = torch.zeros(N, dtype=torch.float64, device="cuda")
    for b in blocks:
        y = LT.block_rows_of(dY, ldy, WG_BLOCK, b, M)[:, :N].double()
        dW_ref += y.t() @ LT.block_rows_of(Xa, ldx, WG_BLOCK, b, M)[:, :K].double()
        db_ref += y.sum(0)
    assert bool(dW_ref.any()) and bool(db_ref.any())
    ws = out_buf(nbytes // 4, F32)
    dW, db = out_buf(N * K, F32), out_buf(N, F32)
    call("uf_linear_wgrad", at(dY), ldy, at(Xa), ldx, dW.data_ptr(), db.data_ptr(), M, N, K, dt(dtype), ws.data_ptr(), nbytes, st())
    assert LT.tail_intact(ws, nbytes // 4) and LT.tail_intact(dW, N * K) and LT.tail_intact(db, N)
    LT.assert_exact_device(f"uf_linear_wgrad/{cfg}/{where}/dW sparse", dW[:N * K], dW_ref.reshape(-1), F32)
    LT.assert_exact_device(f"uf_linear_wgrad/{cfg}/{where}/db sparse", db[:N], db_ref, F32)


# ---------------------------------------------------------------------------------------------------------------------------
# entry points without a size predicate, once past 2^32 bytes
# ---------------------------------------------------------------------------------------------------------------------------
LN_H, LN_W, LN_C = 64, 64, 256                         # 2^22 bytes of f32 rows per image
LN_PER = LN_H * LN_W * LN_C


@pytest.mark.parametrize("dtype,B,windowed", [(F32, 1025, 0), (BF16, 2049, 1)], ids=["f32-plain", "bf16-windowed"])
def test_layernorm_fwd_past_4gib(case, dtype, B, windowed):
    """uf_layernorm_fwd with the f32 input past 2^32 bytes (f32 out, plain) and with the bf16 output past 2^32 bytes too (roll 4 + partition + modulator)"""
    n = B * LN_PER
    chunk = LT.chunk_images([LN_PER * 4])
    case(["uf_layernorm_fwd"], "none", f"{B}x{LN_H}x{LN_W}x{LN_C} f32 -> {TAG[dtype]}", n * (4 + esz(dtype)) + chunk * LN_PER * esz(dtype) + (1 << 28))
    g = torch.Generator().manual_seed(19)
    gamma, beta = small(torch.randint(1, 4, (LN_C,), generator=g).double()), small(torch.randint(-2, 3, (LN_C,), generator=g).double())
    mod = small(torch.randint(-2, 3, (64 * LN_C,), generator=g).double()) if windowed else None
    x = LT.fill_odd(empty(n, F32), 7)
    out = out_buf(n, dtype)

    def run(x_p, out_p, nb):
        call("uf_layernorm_fwd", x_p, LN_C, gamma.data_ptr(), beta.data_ptr(), mod.data_ptr() if windowed else None, out_p, nb, LN_H, LN_W, LN_C, windowed, 4 if windowed else 0, dt(dtype), st())
    run(at(x), at(out), B)
    assert LT.tail_intact(out, n)
    scratch = out_buf(chunk * LN_PER, dtype)

    def run_chunk(b0, nb):
        run(at(x, b0 * LN_PER), at(scratch), nb)
        assert LT.tail_intact(scratch, chunk * LN_PER)
        return scratch[:nb * LN_PER]
    LT.compare_chunks(f"uf_layernorm_fwd/{TAG[dtype]}/B{B}/chunks", out[:n], LN_PER, B, chunk, run_chunk)


def test_layernorm_bwd_past_4gib(case):
    """uf_layernorm_bwd (f32) with x, dy and dx past 2^32 bytes each: dx against the entry point on chunks; dgamma / dbeta on the sparse lattice -- rows
    x = 32 s (-1)^c with a sign s per row (mean 0, rstd = 1 / 32, xhat = +-1 exactly: eps disappears in float32(1024 + 1e-5)), dy in {-1, 1}, zero rows
    elsewhere (xhat = 0, dy = 0)"""
    B = 1025
    n = B * LN_PER
    rows_img = LN_H * LN_W
    chunk = LT.chunk_images([LN_PER * 4])
    nbytes = L().uf_layernorm_bwd_workspace_bytes(B * rows_img, LN_C)
    case(["uf_layernorm_bwd"], "none", f"{B * rows_img} rows of {LN_C} f32", 3 * n * 4 + chunk * LN_PER * 4 + nbytes + (1 << 28))
    g = torch.Generator().manual_seed(23)
    gamma = small(torch.randint(1, 4, (LN_C,), generator=g).double())
    ws = out_buf(nbytes // 4, F32)
    dg, dbt = out_buf(LN_C, F32), out_buf(LN_C, F32)

    def run(x_p, dy_p, dx_p, rows):
        call("uf_layernorm_bwd", x_p, LN_C, gamma.data_ptr(), dy_p, LN_C, dx_p, LN_C, dg.data_ptr(), dbt.data_ptr(), rows, LN_C, ws.data_ptr(), nbytes, st())
        assert LT.tail_intact(ws, nbytes // 4) and LT.tail_intact(dg, LN_C) and LT.tail_intact(dbt, LN_C)
    x, dy, dx = LT.fill_odd(empty(n, F32), 7), LT.fill_odd(empty(n, F32), 3), out_buf(n, F32)
    run(at(x), at(dy), at(dx), B * rows_img)
    assert LT.tail_intact(dx, n)
    scratch = out_buf(chunk * LN_PER, F32)

    def run_chunk(b0, nb):
        run(at(x, b0 * LN_PER), at(dy, b0 * LN_PER), at(scratch), nb * rows_img)
        assert LT.tail_intact(scratch, chunk * LN_PER)
        return scratch[:nb * LN_PER]
    LT.compare_chunks("uf_layernorm_bwd/f32/dx chunks", dx[:n], LN_PER, B, chunk, run_chunk)
    # sparse lattice for the two sums over the rows
    p = LT.plan(B * rows_img, LN_C, 4, rows_img)
    alt = (1 - 2 * (torch.arange(LN_C, device="cuda") % 2)).float()

    def fill_x(v):
        sign = LT.fill_odd(torch.empty(rows_img, 1, device="cuda"), 1)
        v.view(rows_img, LN_C).copy_(32.0 * sign * alt)
    LT.fill_sparse(x, LN_PER, p["blocks"], fill_x)
    LT.fill_sparse(dy, LN_PER, p["blocks"], lambda v: LT.fill_odd(v, 1))
    LT.check_sparse_sum(len(p["blocks"]) * rows_img, 1, 1)
    dg_ref = sum((dy[b * LN_PER:(b + 1) * LN_PER].double() * x[b * LN_PER:(b + 1) * LN_PER].double() / 32.0).view(rows_img, LN_C).sum(0) for b in p["blocks"])
    db_ref = sum(dy[b * LN_PER:(b + 1) * LN_PER].double().view(rows_img, LN_C).sum(0) for b in p["blocks"])
    run(at(x), at(dy), at(dx), B * rows_img)
    LT.assert_exact_device("uf_layernorm_bwd/f32/dgamma sparse", dg[:LN_C], dg_ref, F32)
    LT.assert_exact_device("uf_layernorm_bwd/f32/dbeta sparse", dbt[:LN_C], db_ref, F32)


GELU_BLOCK = 1 << 24                                   # elements: 2^25 bytes of bf16


@pytest.mark.parametrize("dtype,B", [(BF16, 129), (F32, 65)], ids=["bf16", "f32"])
@pytest.mark.parametrize("entry", ["uf_gelu_fwd", "uf_gelu_bwd"])
def test_gelu_past_two_to_the_31_elements(case, entry, dtype, B):
    """129 x 2^24 bf16 elements: past 2^31 elements and 2^32 bytes; 65 x 2^24 f32 elements (the f32 instantiation reads 4 per thread, not 8): past 2^32 bytes"""
    n = B * GELU_BLOCK
    assert n * esz(dtype) > B32
    chunk = LT.chunk_images([GELU_BLOCK * esz(dtype)])
    n_in = 2 if entry == "uf_gelu_bwd" else 1
    case([entry], "none", f"{n} {TAG[dtype]} elements", (n_in + 1) * n * esz(dtype) + chunk * GELU_BLOCK * esz(dtype) + (1 << 28))
    ins = [LT.fill_range(empty(n, dtype), -6, 6) for _ in range(n_in)]
    out = out_buf(n, dtype)

    def run(off, out_p, cnt):
        call(entry, *[at(t, off) for t in ins], out_p, cnt, dt(dtype), st())
    run(0, at(out), n)
    assert LT.tail_intact(out, n)
    scratch = out_buf(chunk * GELU_BLOCK, dtype)

    def run_chunk(b0, nb):
        run(b0 * GELU_BLOCK, at(scratch), nb * GELU_BLOCK)
        assert LT.tail_intact(scratch, chunk * GELU_BLOCK)
        return scratch[:nb * GELU_BLOCK]
    LT.compare_chunks(f"{entry}/{TAG[dtype]}/chunks", out[:n], GELU_BLOCK, B, chunk, run_chunk)


WP_H, WP_W, WP_C = 64, 64, 256                         # 2^21 bytes of 2-byte rows per image


@pytest.mark.parametrize("dtype,B", [(BF16, 2049), (F32, 1025)], ids=["2-byte", "4-byte"])
@pytest.mark.parametrize("entry", ["uf_window_partition", "uf_window_reverse"])
def test_window_copy_past_4gib(case, entry, dtype, B):
    """2049 images of 64 x 64 x 256 2-byte elements with the cyclic shift 4: source and destination past 2^32 bytes and 2^31 elements; 1025 images of
    4-byte elements (the copy kernel is instantiated per element size): past 2^32 bytes"""
    per = WP_H * WP_W * WP_C
    n, sz = B * per, esz(dtype)
    assert n * sz > B32
    chunk = LT.chunk_images([per * sz])
    case([entry], "none", f"{B}x{WP_H}x{WP_W}x{WP_C} {sz}-byte", 2 * n * sz + chunk * per * sz + (1 << 28))
    x = LT.fill_range(empty(n, dtype), -100, 100)
    out = out_buf(n, dtype)
    call(entry, at(x), at(out), B, WP_H, WP_W, WP_C, 4, sz, st())
    assert LT.tail_intact(out, n)
    scratch = out_buf(chunk * per, dtype)

    def run_chunk(b0, nb):
        call(entry, at(x, b0 * per), at(scratch), nb, WP_H, WP_W, WP_C, 4, sz, st())
        assert LT.tail_intact(scratch, chunk * per)
        return scratch[:nb * per]
    LT.compare_chunks(f"{entry}/{sz}-byte/chunks", out[:n], per, B, chunk, run_chunk)


def test_residual_combine_past_4gib(case):
    """out = a + scale[image] * b(window order, shift 4): a and out f32 past 2^32 bytes, b bf16 past 2^31 bytes, per-image scales from {0, 0.5, 1, 2}"""
    B = 1025
    n = B * LN_PER
    chunk = LT.chunk_images([LN_PER * 4])
    case(["uf_residual_combine"], "none", f"{B}x{LN_H}x{LN_W}x{LN_C} f32 + bf16", n * 10 + chunk * LN_PER * 4 + (1 << 28))
    a, b, out = LT.fill_odd(empty(n, F32), 7), LT.fill_odd(empty(n, BF16), 3), out_buf(n, F32)
    scale = small([X.SCALES[(i + 1) % 4] for i in range(B)])
    call("uf_residual_combine", at(a), at(b), 0, at(out), scale.data_ptr(), B, LN_H, LN_W, LN_C, 1, 4, dt(BF16), st())
    assert LT.tail_intact(out, n)
    scratch = out_buf(chunk * LN_PER, F32)

    def run_chunk(b0, nb):
        call("uf_residual_combine", at(a, b0 * LN_PER), at(b, b0 * LN_PER), 0, at(scratch), at(scale, b0), nb, LN_H, LN_W, LN_C, 1, 4, dt(BF16), st())
        assert LT.tail_intact(scratch, chunk * LN_PER)
        return scratch[:nb * LN_PER]
    LT.compare_chunks("uf_residual_combine/chunks", out[:n], LN_PER, B, chunk, run_chunk)


def test_grad_fork_past_4gib(case):
    """sum_out = g1 + g2 (f32, past 2^32 bytes), cast_out = bf16(sum * scale[image]) at the window-order row (shift 4)"""
    B = 1025
    n = B * LN_PER
    chunk = LT.chunk_images([LN_PER * 4])
    case(["uf_grad_fork"], "none", f"{B}x{LN_H}x{LN_W}x{LN_C} f32 -> bf16", n * 14 + chunk * LN_PER * 6 + (1 << 28))
    g1, g2 = LT.fill_odd(empty(n, F32), 7), LT.fill_odd(empty(n, F32), 3)
    s_out, c_out = out_buf(n, F32), out_buf(n, BF16)
    scale = small([X.SCALES[(i + 1) % 4] for i in range(B)])
    call("uf_grad_fork", at(g1), at(g2), at(s_out), at(c_out), scale.data_ptr(), B, LN_H, LN_W, LN_C, 1, 4, dt(BF16), st())
    assert LT.tail_intact(s_out, n) and LT.tail_intact(c_out, n)
    s_s, s_c = out_buf(chunk * LN_PER, F32), out_buf(chunk * LN_PER, BF16)

    def run_chunk(b0, nb):
        call("uf_grad_fork", at(g1, b0 * LN_PER), at(g2, b0 * LN_PER), at(s_s), at(s_c), at(scale, b0), nb, LN_H, LN_W, LN_C, 1, 4, dt(BF16), st())
        assert LT.tail_intact(s_s, chunk * LN_PER) and LT.tail_intact(s_c, chunk * LN_PER)
        return [s_s[:nb * LN_PER], s_c[:nb * LN_PER]]
    LT.compare_chunks("uf_grad_fork/chunks", [s_out[:n], c_out[:n]], LN_PER, B, chunk, run_chunk)


@pytest.mark.parametrize("dtype,B", [(BF16, 171), (F32, 86)], ids=["bf16", "f32"])
def test_qkv_grad_merge_past_4gib(case, dtype, B):
    """two heads of 32 channels, 171 blocks of 1024 windows: the merged bf16 gradient (rows of 3C) is past 2^32 bytes and 2^31 elements; 86 blocks in f32
    (4 elements per thread where the 2-byte instantiation moves 8): past 2^32 bytes"""
    heads, blk, sz = 2, 1024, esz(dtype)
    per_q, per_o = blk * heads * 64 * 32, blk * 64 * 3 * heads * 32
    assert B * per_o * sz > B32
    chunk = LT.chunk_images([per_o * sz])
    case(["uf_qkv_grad_merge"], "none", f"{B * blk} windows x {heads} heads {TAG[dtype]}", B * (3 * per_q + per_o) * sz + chunk * per_o * sz + (1 << 28))
    dq, dk, dvt = (LT.fill_range(empty(B * per_q, dtype), -16, 16) for _ in range(3))
    out = out_buf(B * per_o, dtype)
    call("uf_qkv_grad_merge", at(dq), at(dk), at(dvt), at(out), B * blk, heads, 32, dt(dtype), st())
    assert LT.tail_intact(out, B * per_o)
    scratch = out_buf(chunk * per_o, dtype)

    def run_chunk(b0, nb):
        call("uf_qkv_grad_merge", at(dq, b0 * per_q), at(dk, b0 * per_q), at(dvt, b0 * per_q), at(scratch), nb * blk, heads, 32, dt(dtype), st())
        assert LT.tail_intact(scratch, chunk * per_o)
        return scratch[:nb * per_o]
    LT.compare_chunks(f"uf_qkv_grad_merge/{TAG[dtype]}/chunks", out[:B * per_o], per_o, B, chunk, run_chunk)


@pytest.mark.parametrize("dtype,B", [(BF16, 129), (F32, 65)], ids=["bf16", "f32"])
def test_window_attention_fwd_past_4gib(case, dtype, B):
    """129 blocks of 4096 windows, two heads of 32 channels, bf16: q, k, v^T and the output are past 2^32 bytes and 2^31 elements each; 65 blocks in f32 (its own
    kernel instantiation on the 16 x 16 x 4 MFMA): past 2^32 bytes each"""
    heads, hd, blk, sz = 2, 32, 4096, esz(dtype)
    per = blk * heads * 64 * hd
    assert B * per * sz > B32
    chunk = LT.chunk_images([per * sz])
    case(["uf_window_attention_fwd"], "none", f"{B * blk} windows x {heads} heads x {hd} {TAG[dtype]}", 4 * B * per * sz + chunk * per * sz + (1 << 28))
    q, k, vt = (LT.fill_odd(empty(B * per, dtype), 1) for _ in range(3))
    g = torch.Generator().manual_seed(29)
    bias = small(torch.randint(-2, 3, (heads * 4096,), generator=g).double())
    out = out_buf(B * per, dtype)
    call("uf_window_attention_fwd", at(q), at(k), at(vt), bias.data_ptr(), None, 0, at(out), B * blk, heads, hd, 8, 8, 0, dt(dtype), st())
    assert LT.tail_intact(out, B * per)
    scratch = out_buf(chunk * per, dtype)

    def run_chunk(b0, nb):
        call("uf_window_attention_fwd", at(q, b0 * per), at(k, b0 * per), at(vt, b0 * per), bias.data_ptr(), None, 0, at(scratch), nb * blk, heads, hd, 8, 8, 0, dt(dtype), st())
        assert LT.tail_intact(scratch, chunk * per)
        return scratch[:nb * per]
    LT.compare_chunks(f"uf_window_attention_fwd/{TAG[dtype]}/chunks", out[:B * per], per, B, chunk, run_chunk)


@pytest.mark.parametrize("dtype,M", [(BF16, (1 << 23) + 65536), (F32, (1 << 22) + 65536)], ids=["bf16", "f32"])
def test_rows_sum_past_4gib(case, dtype, M):
    """column sums of 8454144 rows of 256 bf16 (past 2^32 bytes and 2^31 elements), and of 4259840 rows of 256 f32 (4 columns per thread, not 8: past 2^32 bytes),
    on the sparse lattice"""
    N, blk = 256, 65536
    assert M * N * esz(dtype) > B32
    nbytes = L().uf_rows_sum_workspace_bytes(M, N)
    case(["uf_rows_sum"], "none", f"{M} rows of {N} {TAG[dtype]}", M * N * esz(dtype) + nbytes + (1 << 28))
    p = LT.plan(M, N, esz(dtype), blk)
    Xa = LT.fill_sparse(empty(M * N, dtype), blk * N, p["blocks"], lambda v: LT.fill_odd(v, 3))
    LT.check_sparse_sum(len(p["blocks"]) * blk, 3, 1)
    ref = sum(LT.block_rows_of(Xa, N, blk, b, M).double().sum(0) for b in p["blocks"])
    ws, out = out_buf(nbytes // 4, F32), out_buf(N, F32)
    call("uf_rows_sum", at(Xa), N, out.data_ptr(), M, N, dt(dtype), ws.data_ptr(), nbytes, st())
    assert LT.tail_intact(ws, nbytes // 4) and LT.tail_intact(out, N)
    LT.assert_exact_device(f"uf_rows_sum/{TAG[dtype]}/sparse", out[:N], ref, F32)


# ---------------------------------------------------------------------------------------------------------------------------
# the GEMM's other loaders and epilogues (one kernel template with uf_linear_fwd: size_t offsets from int rows), outputs past 2^32 bytes
# ---------------------------------------------------------------------------------------------------------------------------
def pm1(shape, seed, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return small((torch.randint(0, 2, shape, generator=g) * 2 - 1).double(), dtype)


def ints(shape, lo, hi, seed, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return small(torch.randint(lo, hi + 1, shape, generator=g).double(), dtype)


def sentinel_buf(n, dtype):
    """an output whose pad columns the kernel must leave alone: sentinel everywhere"""
    return torch.full((n + LT.GUARD,), LT.SENTINEL, dtype=dtype, device="cuda")


@pytest.mark.parametrize("entry", ["uf_linear_pre_gelu_fwd", "uf_linear_mul_dgelu"])
def test_linear_training_epilogues_past_4gib(case, entry):
    """bf16 A[M][64] W[256][64]^T with M = 2^23 + 65536: the pre-activation and the activation (pre_gelu), or the pre-activation read and the product written
    (mul_dgelu), are M x 256 bf16 = past 2^32 bytes and 2^31 elements each"""
    N, K, blk = 256, 64, 65536
    M = (1 << 23) + blk
    B = M // blk
    chunk = LT.chunk_images([blk * N * 2])
    case([entry], "none", f"M={M} N={N} K={K} bf16", M * (K + 2 * N) * 2 + 2 * chunk * blk * N * 2 + (1 << 28))
    A, W, bias = LT.fill_odd(empty(M * K, BF16), 3), pm1((N, K), 31), ints((N,), -3, 3, 32)
    if entry == "uf_linear_pre_gelu_fwd":
        outs = [out_buf(M * N, BF16), out_buf(M * N, BF16)]
        scratch = [out_buf(chunk * blk * N, BF16), out_buf(chunk * blk * N, BF16)]

        def run(r0, rows, o):
            call(entry, at(A, r0 * K), W.data_ptr(), bias.data_ptr(), at(o[0]), at(o[1]), rows, N, K, dt(BF16), st())
    else:
        pre = LT.fill_range(empty(M * N, BF16), -6, 6)
        outs, scratch = [out_buf(M * N, BF16)], [out_buf(chunk * blk * N, BF16)]

        def run(r0, rows, o):
            call(entry, at(A, r0 * K), W.data_ptr(), bias.data_ptr(), at(pre, r0 * N), at(o[0]), rows, N, K, dt(BF16), st())
    run(0, M, outs)
    assert all(LT.tail_intact(o, M * N) for o in outs)

    def run_chunk(b0, nb):
        run(b0 * blk, nb * blk, scratch)
        assert all(LT.tail_intact(s, chunk * blk * N) for s in scratch)
        return [s[:nb * blk * N] for s in scratch]
    LT.compare_chunks(f"{entry}/bf16/chunks", [o[:M * N] for o in outs], blk * N, B, chunk, run_chunk)


def test_linear_residual_fwd_past_4gib(case):
    """out = resid + scale[image] * (A W^T + bias) at the token of window row m (shift 4): 1025 images of 64 x 64 rows of 256 floats, resid and out past
    2^32 bytes; lattice operands (every sum exact), per-image scales from {0, 0.5, 1, 2}"""
    B, H, Wd, N, K = 1025, 64, 64, 256, 64
    rows = H * Wd
    per_o, per_a = rows * N, rows * K
    chunk = LT.chunk_images([per_o * 4])
    case(["uf_linear_residual_fwd"], "none", f"{B}x{H}x{Wd} rows, N={N} K={K} bf16 -> f32", B * (2 * per_o * 4 + per_a * 2) + chunk * per_o * 4 + (1 << 28))
    A, W, bias = LT.fill_odd(empty(B * per_a, BF16), 3), pm1((N, K), 33), ints((N,), -3, 3, 34)
    resid, out = LT.fill_odd(empty(B * per_o, F32), 7), out_buf(B * per_o, F32)
    scale = small([X.SCALES[(i + 1) % 4] for i in range(B)])
    call("uf_linear_residual_fwd", at(A), W.data_ptr(), bias.data_ptr(), at(resid), at(out), scale.data_ptr(), B, H, Wd, N, K, 1, 4, dt(BF16), st())
    assert LT.tail_intact(out, B * per_o)
    scratch = out_buf(chunk * per_o, F32)

    def run_chunk(b0, nb):
        call("uf_linear_residual_fwd", at(A, b0 * per_a), W.data_ptr(), bias.data_ptr(), at(resid, b0 * per_o), at(scratch), at(scale, b0), nb, H, Wd, N, K, 1, 4, dt(BF16), st())
        assert LT.tail_intact(scratch, chunk * per_o)
        return scratch[:nb * per_o]
    LT.compare_chunks("uf_linear_residual_fwd/bf16/chunks", out[:B * per_o], per_o, B, chunk, run_chunk)


def test_qkv_fwd_past_4gib(case):
    """129 blocks of 4096 windows, C = 64 in two heads, bf16: the activation and each of q, k, v^T (head-major layouts) are past 2^32 bytes and 2^31 elements"""
    C, heads, blk, B = 64, 2, 4096 * 64, 129
    per = blk * C
    chunk = LT.chunk_images([per * 2])
    case(["uf_qkv_fwd"], "none", f"M={B * blk} C={C} heads={heads} bf16", 4 * B * per * 2 + 3 * chunk * per * 2 + (1 << 28))
    A, W, bias = LT.fill_odd(empty(B * per, BF16), 1), pm1((3 * C, C), 35), ints((3 * C,), -3, 3, 36)
    outs = [out_buf(B * per, BF16) for _ in range(3)]
    call("uf_qkv_fwd", at(A), W.data_ptr(), bias.data_ptr(), *[at(o) for o in outs], B * blk, C, heads, dt(BF16), st())
    assert all(LT.tail_intact(o, B * per) for o in outs)
    scratch = [out_buf(chunk * per, BF16) for _ in range(3)]

    def run_chunk(b0, nb):
        call("uf_qkv_fwd", at(A, b0 * per), W.data_ptr(), bias.data_ptr(), *[at(s) for s in scratch], nb * blk, C, heads, dt(BF16), st())
        assert all(LT.tail_intact(s, chunk * per) for s in scratch)
        return [s[:nb * per] for s in scratch]
    LT.compare_chunks("uf_qkv_fwd/bf16/chunks", [o[:B * per] for o in outs], per, B, chunk, run_chunk)


def test_upsample_fwd_past_4gib(case):
    """ConvTranspose2d(k2, s2) written into channels [0, 32) of a 64-channel concat buffer: 4097 images of 32 x 32 -> 64 x 64 rows of 64 floats, the output
    past 2^32 bytes; its channels [32, 64) hold the sentinel and are compared like everything else"""
    B, H, Wd, Cin, Cout, ldo = 4097, 32, 32, 64, 32, 64
    per_x, per_o = H * Wd * Cin, 4 * H * Wd * ldo
    chunk = LT.chunk_images([per_o * 4])
    case(["uf_upsample_fwd"], "none", f"{B}x{H}x{Wd}x{Cin} -> x{2 * H}x{2 * Wd}x{Cout} in rows of {ldo}, bf16 operands", B * (per_x + per_o) * 4 + chunk * per_o * 4 + (1 << 28))
    x, W, bias = LT.fill_odd(empty(B * per_x, F32), 3), pm1((4 * Cout, Cin), 37), ints((Cout,), -3, 3, 38)
    out = sentinel_buf(B * per_o, F32)
    call("uf_upsample_fwd", at(x), Cin, W.data_ptr(), bias.data_ptr(), at(out), ldo, B, H, Wd, Cin, Cout, dt(BF16), st())
    assert LT.tail_intact(out, B * per_o)
    assert bool((out[:per_o].view(-1, ldo)[:, Cout:] == LT.SENTINEL).all()) and bool((out[:per_o].view(-1, ldo)[:, :Cout] != LT.SENTINEL).all())
    scratch = sentinel_buf(chunk * per_o, F32)

    def run_chunk(b0, nb):
        call("uf_upsample_fwd", at(x, b0 * per_x), Cin, W.data_ptr(), bias.data_ptr(), at(scratch), ldo, nb, H, Wd, Cin, Cout, dt(BF16), st())
        assert LT.tail_intact(scratch, chunk * per_o)
        return scratch[:nb * per_o]
    LT.compare_chunks("uf_upsample_fwd/bf16/chunks", out[:B * per_o], per_o, B, chunk, run_chunk)


def test_downsample_fwd_past_4gib(case):
    """Conv2d(k4, s2, p1) on 16385 images of 64 x 64 x 32 (bf16 operands, second form): the f32 input is past 2^33 bytes, the output (32 x 32 rows of 64
    floats per image) past 2^32"""
    B, H, Wd, C = 16385, 64, 64, 32
    per_x, per_o = H * Wd * C, (H // 2) * (Wd // 2) * 2 * C
    chunk = LT.chunk_images([per_x * 4])
    case(["uf_downsample_fwd"], "none (second form: M*ldo < 2^33 - 4)", f"{B}x{H}x{Wd}x{C} bf16 operands", B * (per_x + per_o) * 4 + chunk * per_o * 4 + (1 << 28))
    x, W, bias = LT.fill_odd(empty(B * per_x, F32), 3), pm1((2 * C, 16 * C), 39), ints((2 * C,), -3, 3, 40)
    out = out_buf(B * per_o, F32)
    call("uf_downsample_fwd", at(x), C, W.data_ptr(), bias.data_ptr(), at(out), 2 * C, B, H, Wd, C, dt(BF16), st())
    assert LT.tail_intact(out, B * per_o)
    scratch = out_buf(chunk * per_o, F32)

    def run_chunk(b0, nb):
        call("uf_downsample_fwd", at(x, b0 * per_x), C, W.data_ptr(), bias.data_ptr(), at(scratch), 2 * C, nb, H, Wd, C, dt(BF16), st())
        assert LT.tail_intact(scratch, chunk * per_o)
        return scratch[:nb * per_o]
    LT.compare_chunks("uf_downsample_fwd/bf16/chunks", out[:B * per_o], per_o, B, chunk, run_chunk)


def test_window_attention_bwd_qkv_past_4gib(case):
    """uf_window_attention_bwd_qkv, bf16, two heads of 32 channels, 171 blocks of 1024 windows: the merged gradient dqkv (rows of 3C) is past 2^32 bytes and
    2^31 elements; against the entry point on chunks.  dbias, the sum of dS over all windows, on the sparse lattice with the "uniform" construction of section
    2.5: q = k = 0 and a zero bias make P = 1/64; v[j][d] = sigma_j u_d with balanced key signs sigma and u in {1, 2}, dO in {-1, 1}, so dP = sigma_j m_i with
    m = dO . u, the row dot vanishes and dS = sigma_j m_i / 64 exactly; windows outside the planner's blocks are zero and add nothing"""
    heads, hd, blk, B = 2, 32, 1024, 171
    C = heads * hd
    per, per_o = blk * 64 * C, blk * 64 * 3 * C
    n = B * blk
    assert B * per_o * 2 > B32
    chunk = LT.chunk_images([per_o * 2])
    nbytes = L().uf_window_attention_bwd_workspace_bytes(n, heads)
    case(["uf_window_attention_bwd_qkv"], "none", f"{n} windows x {heads} heads x {hd} bf16", B * (4 * per + per_o) * 2 + chunk * per_o * 2 + nbytes + (1 << 28))
    g = torch.Generator().manual_seed(41)
    bias = small(torch.randint(-2, 3, (heads * 4096,), generator=g).double())
    ws, dbias = out_buf(nbytes // 4, F32), out_buf(heads * 4096, F32)

    def run(b0, nb, t, out_p, bias_t):
        q, k, vt, dO = t
        call("uf_window_attention_bwd_qkv", at(q, b0 * per), at(k, b0 * per), at(vt, b0 * per), bias_t.data_ptr(), None, 0, at(dO, b0 * per), C, out_p, dbias.data_ptr(),
             nb * blk, heads, hd, 8, 8, 0, dt(BF16), ws.data_ptr(), nbytes, st())
        assert LT.tail_intact(ws, nbytes // 4) and LT.tail_intact(dbias, heads * 4096)
    t = [LT.fill_odd(empty(B * per, BF16), 1) for _ in range(4)]
    dqkv = out_buf(B * per_o, BF16)
    run(0, B, t, at(dqkv), bias)
    assert LT.tail_intact(dqkv, B * per_o)
    scratch = out_buf(chunk * per_o, BF16)

    def run_chunk(b0, nb):
        run(b0, nb, t, at(scratch), bias)
        assert LT.tail_intact(scratch, chunk * per_o)
        return scratch[:nb * per_o]
    LT.compare_chunks("uf_window_attention_bwd_qkv/bf16/dqkv chunks", dqkv[:B * per_o], per_o, B, chunk, run_chunk)
    # dbias on the sparse lattice
    q, k, vt, dO = t
    p = LT.plan(n * 64, 3 * C, 2, blk * 64)                       # boundaries of the widest operand, dqkv
    sigma = (1 - 2 * (torch.arange(64, device="cuda") % 2)).to(BF16)
    q.zero_()
    k.zero_()
    ref = torch.zeros(heads, 64, 64, dtype=torch.float64, device="cuda")

    def fill_vt(v):
        u = LT.fill_range(torch.empty(blk, heads, hd, 1, dtype=BF16, device="cuda"), 1, 2)
        v.view(blk, heads, hd, 64).copy_(u * sigma)
    LT.fill_sparse(vt, per, p["blocks"], fill_vt)
    LT.fill_sparse(dO, per, p["blocks"], lambda v: LT.fill_odd(v, 1))
    LT.check_sparse_sum(len(p["blocks"]) * blk, 64, 1)             # |m| <= 64 steps of 1/64 per window
    for b in p["blocks"]:
        u = vt[b * per:(b + 1) * per].view(blk, heads, hd, 64)[..., 0].double()                     # sigma_0 = 1
        d = dO[b * per:(b + 1) * per].view(blk, 64, heads, hd).double()
        m = torch.einsum("wihd,whd->hi", d, u)                                                      # sum over the block's windows of m[w, h, i]
        ref += m[:, :, None] * sigma.double()[None, None, :] / 64.0
    assert bool(ref.any())
    run(0, B, t, at(dqkv), small([0.0] * (heads * 4096)))
    LT.assert_exact_device("uf_window_attention_bwd_qkv/bf16/dbias sparse", dbias[:heads * 4096], ref.reshape(-1), F32)


def test_window_attention_bwd_three_outputs_past_4gib(case):
    """uf_window_attention_bwd (dq, dk, dv^T stored apart), bf16, two heads of 32 channels, 65 blocks of 1024 windows: dO has its own row stride, ldo = 8 C, and so
    passes 2^32 bytes alone while the six other window tensors stay at 0.5 GiB; the pad columns of dO are filled like the rest and nothing may read them"""
    heads, hd, blk, B = 2, 32, 1024, 65
    C = heads * hd
    ldo = 8 * C
    per, per_do = blk * 64 * C, blk * 64 * ldo
    n = B * blk
    assert B * per_do * 2 > B32
    chunk = LT.chunk_images([per_do * 2])
    nbytes = L().uf_window_attention_bwd_workspace_bytes(n, heads)
    case(["uf_window_attention_bwd"], "none", f"{n} windows x {heads} heads x {hd} bf16, ldo = {ldo}", B * (6 * per + per_do) * 2 + 3 * chunk * per * 2 + nbytes + (1 << 28))
    g = torch.Generator().manual_seed(43)
    bias = small(torch.randint(-2, 3, (heads * 4096,), generator=g).double())
    ws, dbias = out_buf(nbytes // 4, F32), out_buf(heads * 4096, F32)
    q, k, vt = (LT.fill_odd(empty(B * per, BF16), 1) for _ in range(3))
    dO = LT.fill_odd(empty(B * per_do, BF16), 1)

    def run(b0, nb, outs):
        call("uf_window_attention_bwd", at(q, b0 * per), at(k, b0 * per), at(vt, b0 * per), bias.data_ptr(), None, 0, at(dO, b0 * per_do), ldo, *[at(o) for o in outs],
             dbias.data_ptr(), nb * blk, heads, hd, 8, 8, 0, dt(BF16), ws.data_ptr(), nbytes, st())
        assert LT.tail_intact(ws, nbytes // 4) and LT.tail_intact(dbias, heads * 4096)
    outs = [out_buf(B * per, BF16) for _ in range(3)]
    run(0, B, outs)
    assert all(LT.tail_intact(o, B * per) for o in outs)
    scratch = [out_buf(chunk * per, BF16) for _ in range(3)]

    def run_chunk(b0, nb):
        run(b0, nb, scratch)
        assert all(LT.tail_intact(s, chunk * per) for s in scratch)
        return [s[:nb * per] for s in scratch]
    LT.compare_chunks("uf_window_attention_bwd/bf16/dq dk dvt chunks", [o[:B * per] for o in outs], per, B, chunk, run_chunk)


# ---------------------------------------------------------------------------------------------------------------------------
# the LayerNorm backward in window order, with the residual gradient added and the cast second output
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["uf_layernorm_bwd_fused", "uf_layernorm_bwd_cast"])
def test_layernorm_bwd_windowed_past_4gib(case, entry):
    """1025 images of 64 x 64 rows of 256: x, the added residual gradient and dx (f32) past 2^32 bytes each, dy in window order (roll 4) -- f32 for _fused, bf16
    with the bf16 cast output in window order and per-image scales for _cast; dx and the cast output against the entry point on chunks.  dgamma / dbeta on the
    sparse lattice of test_layernorm_bwd_past_4gib with ONE sign per image (xhat = s (-1)^c on every row of the image, so the window permutation, which stays
    inside an image, does not enter the float64 reference)"""
    B = 1025
    n = B * LN_PER
    rows_img = LN_H * LN_W
    cast = entry == "uf_layernorm_bwd_cast"
    dyt = BF16 if cast else F32
    chunk = LT.chunk_images([LN_PER * 4])
    nbytes = L().uf_layernorm_bwd_workspace_bytes(B * rows_img, LN_C)
    case([entry], "none", f"{B}x{LN_H}x{LN_W}x{LN_C} f32, dy {TAG[dyt]}", n * (12 + esz(dyt) + (2 if cast else 0)) + chunk * LN_PER * 6 + nbytes + (1 << 28))
    g = torch.Generator().manual_seed(47)
    gamma = small(torch.randint(1, 4, (LN_C,), generator=g).double())
    scale = small([X.SCALES[(i + 1) % 4] for i in range(B)])
    ws = out_buf(nbytes // 4, F32)
    dg, dbt = out_buf(LN_C, F32), out_buf(LN_C, F32)
    x, dy, add = LT.fill_odd(empty(n, F32), 7), LT.fill_odd(empty(n, dyt), 3), LT.fill_odd(empty(n, F32), 5)
    dx = out_buf(n, F32)
    co = out_buf(n, BF16) if cast else None

    def run(b0, nb, dx_p, co_p):
        o = b0 * LN_PER
        args = (at(x, o), LN_C, gamma.data_ptr(), at(dy, o), LN_C, 0 if cast else 1, at(add, o), dx_p, LN_C, dg.data_ptr(), dbt.data_ptr(), nb, LN_H, LN_W, LN_C, 1, 4, dt(BF16))
        if cast:
            call(entry, *args, co_p, at(scale, b0), 1, 4, ws.data_ptr(), nbytes, st())
        else:
            call(entry, *args, ws.data_ptr(), nbytes, st())
        assert LT.tail_intact(ws, nbytes // 4) and LT.tail_intact(dg, LN_C) and LT.tail_intact(dbt, LN_C)
    run(0, B, at(dx), at(co) if cast else None)
    assert LT.tail_intact(dx, n) and (not cast or LT.tail_intact(co, n))
    s_dx, s_co = out_buf(chunk * LN_PER, F32), (out_buf(chunk * LN_PER, BF16) if cast else None)

    def run_chunk(b0, nb):
        run(b0, nb, at(s_dx), at(s_co) if cast else None)
        assert LT.tail_intact(s_dx, chunk * LN_PER) and (not cast or LT.tail_intact(s_co, chunk * LN_PER))
        return [s_dx[:nb * LN_PER]] + ([s_co[:nb * LN_PER]] if cast else [])
    LT.compare_chunks(f"{entry}/dx chunks", [dx[:n]] + ([co[:n]] if cast else []), LN_PER, B, chunk, run_chunk)
    # sparse lattice for the two sums over the rows
    p = LT.plan(B * rows_img, LN_C, 4, rows_img)
    alt = (1 - 2 * (torch.arange(LN_C, device="cuda") % 2)).float()
    signs = {b: (1.0 if i % 3 else -1.0) for i, b in enumerate(p["blocks"])}
    x.zero_()
    for b in p["blocks"]:
        x[b * LN_PER:(b + 1) * LN_PER].view(rows_img, LN_C).copy_((32.0 * signs[b] * alt).expand(rows_img, LN_C))
    LT.fill_sparse(dy, LN_PER, p["blocks"], lambda v: LT.fill_odd(v, 1))
    add.zero_()
    LT.check_sparse_sum(len(p["blocks"]) * rows_img, 1, 1)
    sums = {b: dy[b * LN_PER:(b + 1) * LN_PER].double().view(rows_img, LN_C).sum(0) for b in p["blocks"]}
    dg_ref = sum(sums[b] * signs[b] * alt.double() for b in p["blocks"])
    db_ref = sum(sums.values())
    assert bool(dg_ref.any()) and bool(db_ref.any())
    run(0, B, at(dx), at(co) if cast else None)
    LT.assert_exact_device(f"{entry}/dgamma sparse", dg[:LN_C], dg_ref, F32)
    LT.assert_exact_device(f"{entry}/dbeta sparse", dbt[:LN_C], db_ref, F32)


# ---------------------------------------------------------------------------------------------------------------------------
# the backwards of the two samplers: patch gathers (uf_im2col), casts, uf_linear_wgrad, the input-gradient GEMM / LDS-patch kernel
# ---------------------------------------------------------------------------------------------------------------------------
def test_downsample_bwd_past_4gib(case):
    """Conv2d(k4, s2, p1) backward, bf16 operands, 4097 images of 64 x 64 x 32 -> 32 x 32 x 64: the patch matrix of x the weight gradient reads (rows of 16 Cin) is
    past 2^32 bytes and 2^31 elements in the workspace.  dx (LDS-patch form) against the entry point on chunks; dW_pk / db on the sparse lattice against the
    float64 convolution gradient of the planner's images"""
    B, H, Wd, Cin, Cout = 4097, 64, 64, 32, 64
    Ho, Wo, K = H // 2, Wd // 2, 16 * Cin
    per_x, per_dy = H * Wd * Cin, Ho * Wo * Cout
    assert B * Ho * Wo * K * 2 > B32
    chunk = LT.chunk_images([Ho * Wo * K * 2])
    nbytes, nb_c = L().uf_downsample_bwd_workspace_bytes(B, H, Wd, Cin, Cout, dt(BF16)), L().uf_downsample_bwd_workspace_bytes(chunk, H, Wd, Cin, Cout, dt(BF16))
    case(["uf_downsample_bwd"], "none", f"{B}x{H}x{Wd}x{Cin} -> {Cout}, bf16 operands", B * (2 * per_x + per_dy) * 4 + nbytes + nb_c + chunk * per_x * 4 + (1 << 28))
    w_t = pm1((K, Cout), 51)
    ws, ws_c = out_buf(nbytes // 4, F32), out_buf(nb_c // 4, F32)
    dW, db = out_buf(Cout * K, F32), out_buf(Cout, F32)
    x, dy, dx = LT.fill_odd(empty(B * per_x, F32), 3), LT.fill_odd(empty(B * per_dy, F32), 1), out_buf(B * per_x, F32)

    def run(b0, nb, dx_p, w, w_bytes):
        call("uf_downsample_bwd", at(x, b0 * per_x), Cin, at(dy, b0 * per_dy), w_t.data_ptr(), dx_p, Cin, 0, dW.data_ptr(), db.data_ptr(), nb, H, Wd, Cin, Cout, dt(BF16),
             w.data_ptr(), w_bytes, st())
        assert LT.tail_intact(w, w_bytes // 4) and LT.tail_intact(dW, Cout * K) and LT.tail_intact(db, Cout)
    run(0, B, at(dx), ws, nbytes)
    assert LT.tail_intact(dx, B * per_x)
    scratch = out_buf(chunk * per_x, F32)

    def run_chunk(b0, nb):
        run(b0, nb, at(scratch), ws_c, nb_c)
        assert LT.tail_intact(scratch, chunk * per_x)
        return scratch[:nb * per_x]
    LT.compare_chunks("uf_downsample_bwd/bf16/dx chunks", dx[:B * per_x], per_x, B, chunk, run_chunk)
    p = LT.plan(B * Ho * Wo, K, 2, Ho * Wo)                          # boundaries of the patch matrix
    LT.fill_sparse(x, per_x, p["blocks"], lambda v: LT.fill_odd(v, 3))
    LT.fill_sparse(dy, per_dy, p["blocks"], lambda v: LT.fill_odd(v, 1))
    LT.check_sparse_sum(len(p["blocks"]) * Ho * Wo, 3, 1)
    dW_ref = torch.zeros(Cout, K, dtype=torch.float64, device="cuda")
    db_ref = torch.zeros(Cout, dtype=torch.float64, device="cuda")
    for b in p["blocks"]:
        xp = torch.zeros(H + 2, Wd + 2, Cin, dtype=torch.float64, device="cuda")
        xp[1:H + 1, 1:Wd + 1] = x[b * per_x:(b + 1) * per_x].view(H, Wd, Cin).double()
        g = dy[b * per_dy:(b + 1) * per_dy].view(Ho * Wo, Cout).double()
        for ky in range(4):
            for kx in range(4):
                patch = xp[ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2].reshape(Ho * Wo, Cin)
                dW_ref[:, (ky * 4 + kx) * Cin:(ky * 4 + kx + 1) * Cin] += g.t() @ patch
        db_ref += g.sum(0)
    assert bool(dW_ref.any()) and bool(db_ref.any())
    run(0, B, at(dx), ws, nbytes)
    LT.assert_exact_device("uf_downsample_bwd/bf16/dW sparse", dW[:Cout * K], dW_ref.reshape(-1), F32)
    LT.assert_exact_device("uf_downsample_bwd/bf16/db sparse", db[:Cout], db_ref, F32)


def test_upsample_cat_bwd_past_4gib(case):
    """ConvTranspose2d(k2, s2) backward from the gradient of a 64-channel concat buffer whose first 32 channels are the layer's: 4097 images of 32 x 32 x 64 ->
    64 x 64, the f32 concat gradient past 2^32 bytes (its skip half is filled and must not be read).  dx against the entry point on chunks; dW_pk / db on the
    sparse lattice against the float64 gradient of the planner's images"""
    B, H, Wd, Cin, Cout, ld_d = 4097, 32, 32, 64, 32, 64
    per_d, per_x = 4 * H * Wd * ld_d, H * Wd * Cin
    assert B * per_d * 4 > B32
    chunk = LT.chunk_images([per_d * 4])
    nbytes, nb_c = L().uf_upsample_cat_bwd_workspace_bytes(B, H, Wd, Cin, Cout, dt(BF16)), L().uf_upsample_cat_bwd_workspace_bytes(chunk, H, Wd, Cin, Cout, dt(BF16))
    case(["uf_upsample_cat_bwd"], "none", f"{B}x{H}x{Wd}x{Cin} -> x{2 * H}x{2 * Wd}x{Cout} in rows of {ld_d}, bf16 operands",
         B * (per_d + 2 * per_x) * 4 + nbytes + nb_c + chunk * per_x * 4 + (1 << 28))
    w_t = pm1((Cin, 4 * Cout), 53)
    ws, ws_c = out_buf(nbytes // 4, F32), out_buf(nb_c // 4, F32)
    dW, db = out_buf(4 * Cout * Cin, F32), out_buf(Cout, F32)
    d, x, dx = LT.fill_odd(empty(B * per_d, F32), 1), LT.fill_odd(empty(B * per_x, F32), 3), out_buf(B * per_x, F32)

    def run(b0, nb, dx_p, w, w_bytes):
        call("uf_upsample_cat_bwd", at(d, b0 * per_d), ld_d, at(x, b0 * per_x), Cin, w_t.data_ptr(), dx_p, dW.data_ptr(), db.data_ptr(), nb, H, Wd, Cin, Cout, dt(BF16),
             w.data_ptr(), w_bytes, st())
        assert LT.tail_intact(w, w_bytes // 4) and LT.tail_intact(dW, 4 * Cout * Cin) and LT.tail_intact(db, Cout)
    run(0, B, at(dx), ws, nbytes)
    assert LT.tail_intact(dx, B * per_x)
    scratch = out_buf(chunk * per_x, F32)

    def run_chunk(b0, nb):
        run(b0, nb, at(scratch), ws_c, nb_c)
        assert LT.tail_intact(scratch, chunk * per_x)
        return scratch[:nb * per_x]
    LT.compare_chunks("uf_upsample_cat_bwd/bf16/dx chunks", dx[:B * per_x], per_x, B, chunk, run_chunk)
    p = LT.plan(B * 4 * H * Wd, ld_d, 4, 4 * H * Wd)
    LT.fill_sparse(d, per_d, p["blocks"], lambda v: LT.fill_odd(v, 1))
    LT.fill_sparse(x, per_x, p["blocks"], lambda v: LT.fill_odd(v, 3))
    LT.check_sparse_sum(len(p["blocks"]) * 4 * H * Wd, 3, 1)
    dW_ref = torch.zeros(4 * Cout, Cin, dtype=torch.float64, device="cuda")
    db_ref = torch.zeros(Cout, dtype=torch.float64, device="cuda")
    for b in p["blocks"]:
        di = d[b * per_d:(b + 1) * per_d].view(2 * H, 2 * Wd, ld_d)[:, :, :Cout].double()
        xi = x[b * per_x:(b + 1) * per_x].view(H * Wd, Cin).double()
        for sy in range(2):
            for sx in range(2):
                dW_ref[(sy * 2 + sx) * Cout:(sy * 2 + sx + 1) * Cout] += di[sy::2, sx::2].reshape(H * Wd, Cout).t() @ xi
        db_ref += di.sum((0, 1))
    assert bool(dW_ref.any()) and bool(db_ref.any())
    run(0, B, at(dx), ws, nbytes)
    LT.assert_exact_device("uf_upsample_cat_bwd/bf16/dW sparse", dW[:4 * Cout * Cin], dW_ref.reshape(-1), F32)
    LT.assert_exact_device("uf_upsample_cat_bwd/bf16/db sparse", db[:Cout], db_ref, F32)


# ---------------------------------------------------------------------------------------------------------------------------
# the 4 x 4-window attention core: refuses B*H*W*ld_qkv >= 2^31 - 1
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["uf_window4_attention_fwd", "uf_window4_attention_bwd"])
def test_window4_attention_under_its_refusal(case, entry):
    """5461 images of 64 x 64 rows of q | k | v (ld 96, one head of 32, bf16) are 2^31 - 131072 elements, the largest whole-image batch accepted; against the entry point
    on chunks.  5462 images are refused, with allocations of that size behind every pointer"""
    B, H, Wd, C, heads, ld = 5461, 64, 64, 32, 1, 96
    bwd = entry.endswith("bwd")
    per_q, per_o, per_s = H * Wd * ld, H * Wd * C, (H // 4) * (Wd // 4) * heads * 256
    assert B * per_q < 0x7fffffff <= (B + 1) * per_q
    chunk = LT.chunk_images([per_q * 2])
    Ba = B + 1
    case([entry], "refuses B*H*W*ld_qkv >= 2^31 - 1", f"{B} and {Ba} x {H}x{Wd} rows of {ld} bf16",
         Ba * ((2 * per_q + per_o) * 2 + per_s * 4 if bwd else (per_q + per_o) * 2) + chunk * (per_q * 2 + per_s * 4) + (1 << 28))
    tab = ints((heads * 49,), -2, 2, 55)
    qkv = LT.fill_odd(empty(Ba * per_q, BF16), 1)
    if bwd:
        dout = LT.fill_odd(empty(Ba * per_o, BF16), 1)
        outs, pers = [out_buf(Ba * per_q, BF16), out_buf(Ba * per_s, F32)], [per_q, per_s]
        scratch = [out_buf(chunk * per_q, BF16), out_buf(chunk * per_s, F32)]

        def args(b0, nb, o):
            return (at(qkv, b0 * per_q), ld, tab.data_ptr(), at(dout, b0 * per_o), C, at(o[0]), ld, at(o[1]), nb, H, Wd, C, heads, dt(BF16), st())
    else:
        outs, pers = [out_buf(Ba * per_o, BF16)], [per_o]
        scratch = [out_buf(chunk * per_o, BF16)]

        def args(b0, nb, o):
            return (at(qkv, b0 * per_q), ld, tab.data_ptr(), at(o[0]), C, nb, H, Wd, C, heads, dt(BF16), st())
    call(entry, *args(0, B, outs))
    assert all(LT.tail_intact(o, Ba * per) for o, per in zip(outs, pers))

    def run_chunk(b0, nb):
        call(entry, *args(b0, nb, scratch))
        assert all(LT.tail_intact(s, chunk * per) for s, per in zip(scratch, pers))
        return [s[:nb * per] for s, per in zip(scratch, pers)]
    LT.compare_chunks(f"{entry}/bf16/chunks", [o[:B * per] for o, per in zip(outs, pers)], pers, B, chunk, run_chunk)
    assert status(entry, *args(0, Ba, outs)) == X.UF_ERR_SHAPE


# ---------------------------------------------------------------------------------------------------------------------------
# the fused block kernels: LN + projection producers, the FFN kernel, the LeFF kernel, the block entry points
# ---------------------------------------------------------------------------------------------------------------------------
def lewin_block(C, heads, shift, dtype, conv=False):
    """(uf_block_params, its tensors by name) of a LeWin block with a modulator and random weights, its biases and tables moved away from zero"""
    from uformer_amd import model, packing
    torch.manual_seed(61 + C + shift)
    blk = model.LeWinTransformerBlock(C, (16, 16), heads, win_size=8, shift_size=shift, modulator=True, token_projection="conv" if conv else "linear")
    with torch.no_grad():
        for name, prm in blk.named_parameters():
            if prm.dim() == 1 or "table" in name:
                prm.add_(0.1 * torch.randn(prm.shape))
    return packing.pack_block({k: v.detach().cuda() for k, v in blk.state_dict().items()}, "", heads, shift, dtype)


@pytest.mark.parametrize("entry,B", [("uf_ln_convqkv_fwd", 8191), ("uf_ln_qkv_fwd", 8193)])
def test_ln_projections(case, entry, B):
    """LN1 + roll 4 + partition + modulator + the q | k | v projection (ConvProjection: with the three window stencils in front), bf16, images of 64 x 64 x 64:
    uf_ln_convqkv_fwd at 8191 images, 2^31 - 2^18 elements, the largest whole-image batch under its refusal (8192 are refused, allocated in full); uf_ln_qkv_fwd,
    which has no limit, at 8193: q, k and v^T past 2^31 elements and 2^32 bytes each, the f32 stream past 2^33 bytes"""
    H, Wd, C, heads, shift, dtype = 64, 64, 64, 2, 4, BF16
    conv = entry == "uf_ln_convqkv_fwd"
    per = H * Wd * C
    Ba = B + 1 if conv else B
    assert (B * per < 0x7fffffff <= Ba * per) if conv else (B * per * 2 > B32)
    chunk = LT.chunk_images([per * 4])
    case([entry], "refuses B*H*W*C >= 2^31 - 1" if conv else "none", f"{B}x{H}x{Wd}x{C} f32 -> bf16", Ba * per * 10 + 3 * chunk * per * 2 + (1 << 28))
    bp, kp = lewin_block(C, heads, shift, dtype, conv)
    x = empty(Ba * per, F32).normal_()
    outs = [out_buf(Ba * per, dtype) for _ in range(3)]
    front = (kp["norm1_w"].data_ptr(), kp["norm1_b"].data_ptr(), kp["modulator"].data_ptr()) + ((kp["qkv_dw9"].data_ptr(), kp["qkv_bdw"].data_ptr()) if conv else ())

    def args(b0, nb, o):
        return (at(x, b0 * per), C, *front, kp["wqkv_fm"].data_ptr(), kp["bqkv"].data_ptr(), *[at(t) for t in o], nb, H, Wd, C, heads, shift, dt(dtype), st())
    call(entry, *args(0, B, outs))
    assert all(LT.tail_intact(o, Ba * per) for o in outs)
    scratch = [out_buf(chunk * per, dtype) for _ in range(3)]

    def run_chunk(b0, nb):
        call(entry, *args(b0, nb, scratch))
        assert all(LT.tail_intact(s, chunk * per) for s in scratch)
        return [s[:nb * per] for s in scratch]
    LT.compare_chunks(f"{entry}/bf16/chunks", [o[:B * per] for o in outs], per, B, chunk, run_chunk)
    if conv:
        assert status(entry, *args(0, Ba, outs)) == X.UF_ERR_SHAPE


def test_ln_linear_gelu_fwd_past_4gib(case):
    """LN2 + linear1 + GELU, bf16, C = 64 -> 256, 8454144 rows: the hidden output is past 2^32 bytes and 2^31 elements"""
    C, N, blk, dtype = 64, 256, 65536, BF16
    M = (1 << 23) + blk
    B = M // blk
    chunk = LT.chunk_images([blk * N * 2])
    case(["uf_ln_linear_gelu_fwd"], "none", f"M={M} C={C} N={N} bf16", M * (C * 4 + N * 2) + chunk * blk * N * 2 + (1 << 28))
    bp, kp = lewin_block(C, 2, 0, dtype)
    x = empty(M * C, F32).normal_()
    out = out_buf(M * N, dtype)

    def run(r0, rows, o):
        call("uf_ln_linear_gelu_fwd", at(x, r0 * C), C, kp["norm2_w"].data_ptr(), kp["norm2_b"].data_ptr(), kp["w1_fm"].data_ptr(), kp["b1"].data_ptr(), at(o), rows, N, C, dt(dtype), st())
    run(0, M, out)
    assert LT.tail_intact(out, M * N)
    scratch = out_buf(chunk * blk * N, dtype)

    def run_chunk(b0, nb):
        run(b0 * blk, nb * blk, scratch)
        assert LT.tail_intact(scratch, chunk * blk * N)
        return scratch[:nb * blk * N]
    LT.compare_chunks("uf_ln_linear_gelu_fwd/bf16/chunks", out[:M * N], blk * N, B, chunk, run_chunk)


def test_ffn_fwd_past_4gib(case):
    """the fused Mlp kernel in place on 257 images of 65536 tokens of 64 floats: the stream is past 2^32 bytes (inside the limit M*ld < 2^33 - 4, whose own crossing
    is 32 GiB), per-image scales from {0, 0.5, 1, 2}; fc1 / fc2 are the linear1 / linear2 of a LeFF block, which have the shapes of an Mlp's"""
    C, tok, B, dtype = 64, 65536, 257, BF16
    per = tok * C
    assert B * per * 4 > B32
    chunk = LT.chunk_images([per * 4])
    case(["uf_ffn_fwd"], "refuses M*ld >= 2^33 - 4", f"{B}x{tok} rows of {C} f32, bf16 operands", 2 * B * per * 4 + chunk * per * 4 + (1 << 28))
    bp, kp = lewin_block(C, 2, 0, dtype)
    scale = small([X.SCALES[(i + 1) % 4] for i in range(B)])
    x0 = empty(B * per, F32).normal_()
    x = out_buf(B * per, F32)
    x[:B * per].copy_(x0)

    def run(x_p, b0, nb):
        call("uf_ffn_fwd", x_p, C, kp["norm2_w"].data_ptr(), kp["norm2_b"].data_ptr(), kp["w1_fm"].data_ptr(), kp["b1"].data_ptr(), kp["w2_fm"].data_ptr(), kp["b2"].data_ptr(),
             at(scale, b0), nb, nb * tok, C, dt(dtype), st())
    run(at(x), 0, B)
    assert LT.tail_intact(x, B * per)
    scratch = out_buf(chunk * per, F32)

    def run_chunk(b0, nb):
        scratch[:nb * per].copy_(x0[b0 * per:(b0 + nb) * per])
        run(at(scratch), b0, nb)
        assert LT.tail_intact(scratch, chunk * per)
        return scratch[:nb * per]
    LT.compare_chunks("uf_ffn_fwd/bf16/chunks", x[:B * per], per, B, chunk, run_chunk)


def test_dwconv_linear2_one_image_under_its_refusal(case):
    """uf_dwconv_linear2_fwd on ONE image of 2097144 x 8 pixels, C = 32, bf16: its hidden tensor is 0xffffc000 bytes, the largest image of whole 8-row tile bands under the
    refusal at 0xffffff00 (one band more, 2^32 bytes, is refused: allocated in full).  The kernel addresses an image through a 32-bit buffer descriptor, so every byte
    offset from 2^31 on is past what a signed product holds.  An image cannot be cut into images, so the reference is the entry point on bands of 131072 rows with 8
    more rows on either side (the tile grid stays where it is); the halo rows, whose stencil sees the band's edge, are not compared"""
    H, Wd, C, dtype = 2097144, 8, 32, BF16
    HID = 4 * C
    assert H * Wd * HID * 2 == 0xffffc000 and (H + 8) * Wd * HID * 2 >= 0xffffff00
    band, halo = 131072, 8
    rows_c = band + 2 * halo
    case(["uf_dwconv_linear2_fwd"], "refuses one image of the hidden tensor >= 0xffffff00 bytes", f"1x{H}x{Wd} C={C} bf16", (H + 8) * Wd * (HID * 2 + 2 * C * 4) + rows_c * Wd * C * 4 + (1 << 28))
    bp, kp = lewin_block(C, 1, 0, dtype)
    h1 = LT.fill_range(empty((H + 8) * Wd * HID, dtype), -4, 4)
    x0 = empty((H + 8) * Wd * C, F32).normal_()
    x = out_buf((H + 8) * Wd * C, F32)
    x[:(H + 8) * Wd * C].copy_(x0)

    def args(h_p, x_p, rows):
        return (h_p, kp["wdw9"].data_ptr(), kp["bdw"].data_ptr(), kp["w2_fm"].data_ptr(), kp["b2"].data_ptr(), x_p, C, 1, rows, Wd, C, dt(dtype), st())
    call("uf_dwconv_linear2_fwd", *args(at(h1), at(x), H))
    assert LT.tail_intact(x, (H + 8) * Wd * C)
    assert LT.count_diff(x[H * Wd * C:(H + 8) * Wd * C], x0[H * Wd * C:])[0] == 0, "rows behind the image were written"
    scratch = out_buf(rows_c * Wd * C, F32)
    total = differing = 0
    first = None
    for r0 in range(0, H, band):
        r1 = min(r0 + band, H)
        a, b = max(r0 - halo, 0), min(r1 + halo, H)
        scratch[:(b - a) * Wd * C].copy_(x0[a * Wd * C:b * Wd * C])
        call("uf_dwconv_linear2_fwd", *args(at(h1, a * Wd * HID), at(scratch), b - a))
        assert LT.tail_intact(scratch, rows_c * Wd * C)
        n, idx = LT.count_diff(x[r0 * Wd * C:r1 * Wd * C], scratch[(r0 - a) * Wd * C:(r1 - a) * Wd * C])
        if n and first is None:
            first = r0 + idx // (Wd * C)
        total, differing = total + (r1 - r0) * Wd * C, differing + n
    LT.record("uf_dwconv_linear2_fwd/bf16/one image/bands", total, differing)
    assert differing == 0, f"{differing} of {total} elements of the large call differ from the entry point on bands of {band} rows; first in image row {first}"
    assert status("uf_dwconv_linear2_fwd", *args(at(h1), at(x), H + 8)) == X.UF_ERR_SHAPE


BLK_H, BLK_W, BLK_C, BLK_CHUNK = 256, 256, 64, 8


@pytest.mark.parametrize("dtype,B", [(F32, 64), (BF16, 128), (BF16, 129)], ids=["f32-64", "bf16-128", "bf16-129"])
@pytest.mark.parametrize("entry", ["uf_lewin_block_fwd", "uf_lewin_attn_fwd", "uf_leff_fwd"])
def test_block_at_the_uformer_b_shape(case, entry, dtype, B):
    """a LeWin block (shift 4, modulator) of the last decoder stage of Uformer-B, C = 64 at 256 x 256: 64 images in f32, where the LeFF hidden tensor in the workspace is
    exactly 2^32 bytes, and 128 / 129 images in bf16, where it reaches / passes 2^32 bytes and 2^31 elements -- all inside the block limit of 2^33 - 4 hidden elements.
    The stream, and the hidden tensor h1 the call leaves in its workspace (whole block and FFN half), against the same entry point on chunks of 8 images, bit for bit:
    at C = 64 no launcher picks its kernel form by the number of windows or tiles, so both run one form"""
    H, Wd, C, chunk = BLK_H, BLK_W, BLK_C, BLK_CHUNK
    per, sz = H * Wd * C, esz(dtype)
    M = B * H * Wd
    assert M * 4 * C * sz >= B32
    nbytes, nb_c = L().uf_block_workspace_bytes(M, C, dt(dtype)), L().uf_block_workspace_bytes(chunk * H * Wd, C, dt(dtype))
    case([entry], "block: refuses B*H*W*4C >= 2^33 - 4 (inside it)", f"{B}x{H}x{Wd} C={C} {TAG[dtype]}", 2 * M * C * 4 + nbytes + nb_c + chunk * per * 4 + (1 << 28))
    bp, kp = lewin_block(C, 2, 4, dtype)
    hidden = entry != "uf_lewin_attn_fwd"
    x0 = empty(M * C, F32).normal_()
    x = out_buf(M * C, F32)
    x[:M * C].copy_(x0)
    ws, ws_c = out_buf(nbytes // 4, F32), out_buf(nb_c // 4, F32)

    def run(x_p, nb, w, w_bytes):
        tail = (dt(dtype), w.data_ptr(), w_bytes, st())
        call(entry, bp, x_p, C, nb, H, Wd, C, *(tail if entry == "uf_leff_fwd" else (None, 0) + tail))
        assert LT.tail_intact(w, w_bytes // 4)

    def h1_of(w, rows):                                              # the workspace is T[M][C], then h1 T[M][4C], each rounded up to 256 bytes
        off = (rows * C * sz + 255) // 256 * 256
        return w.view(torch.uint8)[off:off + rows * 4 * C * sz].view(dtype)
    run(at(x), B, ws, nbytes)
    assert LT.tail_intact(x, M * C)
    scratch = out_buf(chunk * per, F32)

    def run_chunk(b0, nb):
        scratch[:nb * per].copy_(x0[b0 * per:(b0 + nb) * per])
        run(at(scratch), nb, ws_c, nb_c)
        assert LT.tail_intact(scratch, chunk * per)
        return [scratch[:nb * per]] + ([h1_of(ws_c, nb * H * Wd)] if hidden else [])
    LT.compare_chunks(f"{entry}/{TAG[dtype]}/B{B}/chunks", [x[:M * C]] + ([h1_of(ws, M)] if hidden else []), [per, 4 * per] if hidden else [per], B, chunk, run_chunk)


@pytest.mark.parametrize("entry", ["uf_im2col", "uf_col2im"])
def test_patch_gathers_past_4gib(case, entry):
    """the k4 s2 p1 patch matrix of 4097 images of 64 x 64 x 32 (bf16 rows of 16 Cin = 512, token-row fast path): past 2^32 bytes and 2^31 elements, written by uf_im2col
    from the f32 rows and read by uf_col2im into them"""
    B, H, Wd, Cin = 4097, 64, 64, 32
    K, Mo = 16 * Cin, (H // 2) * (Wd // 2)
    per_x, per_c = H * Wd * Cin, Mo * K
    assert B * per_c * 2 > B32
    chunk = LT.chunk_images([per_c * 2])
    gather = entry == "uf_im2col"
    per_o, odt = (per_c, BF16) if gather else (per_x, F32)
    case([entry], "none", f"{B}x{H}x{Wd}x{Cin} <-> {B * Mo} rows of {K} bf16", B * (per_x * 4 + per_c * 2) + chunk * per_o * esz(odt) + (1 << 28))
    src = LT.fill_range(empty(B * per_x, F32), -100, 100) if gather else LT.fill_odd(empty(B * per_c, BF16), 3)
    out = out_buf(B * per_o, odt)

    def run(b0, nb, o):
        if gather:
            call(entry, at(src, b0 * per_x), Cin, at(o), K, nb, H, Wd, Cin, 4, 2, 1, 0, dt(BF16), st())
        else:
            call(entry, at(src, b0 * per_c), K, at(o), Cin, nb, H, Wd, Cin, 4, 2, 1, 0, 0, dt(BF16), st())
    run(0, B, out)
    assert LT.tail_intact(out, B * per_o)
    scratch = out_buf(chunk * per_o, odt)

    def run_chunk(b0, nb):
        run(b0, nb, scratch)
        assert LT.tail_intact(scratch, chunk * per_o)
        return scratch[:nb * per_o]
    LT.compare_chunks(f"{entry}/bf16/chunks", out[:B * per_o], per_o, B, chunk, run_chunk)
