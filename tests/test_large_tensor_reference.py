"""CPU: the tools of tests/large_tensor.py on small arrays with scaled-down boundaries (2^11 / 2^12 bytes and elements in place of 2^31 / 2^32).

  * the planner, on dense and padded operands and with boundaries that fall inside an image;
  * stand-ins of the faults the large-tensor tests exist for -- an offset taken modulo the boundary, a row index truncated to a signed width and
    clamped, a byte predicate that counts elements, a predicate that ignores ld, a chunk walk that drops or repeats the image at a seam, chunk
    gradients overwritten in place of added -- each of which must be caught by the chunked compare or must move the sparse lattice reference;
  * the inventory names every size constant of the sources.
"""
import pytest
import torch

import large_tensor as LT
from exact_lattice import F32, BF16, SENTINEL

P31, P32 = 1 << 11, 1 << 12                     # pretend boundaries
MARKS = dict(byte_marks=(P31, P32), elem_marks=(P31, P32))


# ---------------------------------------------------------------------------------------------------------------------------
# planner
# ---------------------------------------------------------------------------------------------------------------------------
def test_plan_dense_f32():
    """40 images of 32 rows x 4 floats (512 bytes): byte 2^11 opens image 4, byte 2^12 image 8; element 2^11 image 16, element 2^12 image 32"""
    p = LT.plan(40 * 32, 4, 4, 32, **MARKS)
    assert p["n_blocks"] == 40
    assert p["marks"] == {("byte", P31): 4, ("byte", P32): 8, ("elem", P31): 16, ("elem", P32): 32}
    assert p["blocks"] == [0, 3, 4, 7, 8, 15, 16, 31, 32, 39]


def test_plan_two_byte_type_and_short_operand():
    """2-byte elements: byte 2^12 and element 2^11 are the same place; boundaries past the operand are left out"""
    p = LT.plan(20 * 32, 4, 2, 32, **MARKS)         # 20 images of 256 bytes = 5120 bytes, 2560 elements
    assert p["marks"] == {("byte", P31): 8, ("byte", P32): 16, ("elem", P31): 16}
    assert p["blocks"] == [0, 7, 8, 15, 16, 19]


def test_plan_padded_operand_counts_ld():
    """ld > C: the boundaries move with the stride, not with the live columns"""
    dense = LT.plan(64 * 16, 8, 4, 16, **MARKS)
    padded = LT.plan(64 * 16, 12, 4, 16, **MARKS)
    assert dense["marks"][("byte", P32)] == 8 and padded["marks"][("byte", P32)] == 5       # row 128 / row 85
    assert ("elem", P32) in dense["marks"] and padded["marks"][("elem", P32)] == 21


def test_plan_boundary_inside_an_image_and_seams():
    """images of 24 rows x 4 floats = 384 bytes: byte 2^12 falls inside image 10 (row 256 = image 10, row 16 of it); its predecessor and the
    chunk seam images asked for are in the plan, out-of-range seams are not"""
    p = LT.plan(13 * 24, 4, 4, 24, extra=(6, 7, 99), **MARKS)
    assert p["marks"][("byte", P32)] == 10 and (P32 // 4 // 4) % 24 != 0
    assert {0, 12, 9, 10, 6, 7} <= set(p["blocks"]) and 99 not in p["blocks"]


def test_plan_last_block_ragged():
    p = LT.plan(100, 8, 2, 32, byte_marks=(), elem_marks=())
    assert p["n_blocks"] == 4 and p["blocks"] == [0, 3]
    assert LT.block_rows_of(torch.arange(800), 8, 32, 3, 100).shape == (4, 8)


def test_chunk_images():
    assert LT.chunk_images([1 << 26, 1 << 25]) == 8 and LT.chunk_images([1 << 30]) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# stand-ins: a row-local operation y[r][0:C] = 2 x[r][0:C] + 1 on rows of stride ld, computed the way a faulty kernel would address it
# ---------------------------------------------------------------------------------------------------------------------------
ROWS_PER_IMAGE = 16


def rowwise(x, rows, ld, C, esize, wrap_bytes=None, trunc_bits=None):
    """out (rows * ld + guard, sentinel in pad columns and tail).  wrap_bytes: byte offsets taken modulo it (a 32-bit offset register);
    trunc_bits: the row index cut to that signed width, then clamped into the array"""
    out = torch.full((rows * ld + 64,), SENTINEL, dtype=x.dtype)
    r = torch.arange(rows)
    if trunc_bits is not None:
        half = 1 << (trunc_bits - 1)
        r = (((r + half) % (2 * half)) - half).clamp(0, rows - 1)
    off = r * ld
    if wrap_bytes is not None:
        off = (off * esize % wrap_bytes) // esize
    idx = (off[:, None] + torch.arange(C)[None, :]).reshape(-1)
    out[idx] = 2 * x[idx] + 1
    return out


def launcher(x, rows, ld, C, esize, predicate):
    """the narrow form (offsets modulo the pretend 2^32) when ``predicate`` says the tensor is small, else the clean form"""
    return rowwise(x, rows, ld, C, esize, wrap_bytes=P32 if predicate(rows, ld, C, esize) else None)


def chunked_check(big, x, B, ld, C, esize, chunk=2):
    """compare_chunks on the dense live columns of a stand-in's output against the clean operation on chunks of whole images"""
    per = ROWS_PER_IMAGE * ld

    def run_chunk(b0, nb):
        return rowwise(x[b0 * per:(b0 + nb) * per], nb * ROWS_PER_IMAGE, ld, C, esize)[:nb * per]
    LT.compare_chunks("stand-in", big, per, B, chunk, run_chunk)
    assert LT.tail_intact(big, B * per)


def make_x(B, ld, dtype=F32):
    torch.manual_seed(3)
    return LT.fill_odd(torch.empty(B * ROWS_PER_IMAGE * ld, dtype=dtype))


def test_clean_operation_passes():
    """the compare holds on a correct large call: dense and padded, both types"""
    for ld, C, dtype, esize in ((8, 8, F32, 4), (12, 8, F32, 4), (16, 16, BF16, 2)):
        B = 24
        x = make_x(B, ld, dtype)
        chunked_check(rowwise(x, B * ROWS_PER_IMAGE, ld, C, esize), x, B, ld, C, esize)


def test_fault_offset_modulo_boundary():
    B, ld, C = 12, 8, 8                                   # 12 images of 512 bytes: 2^12 bytes open image 8
    x = make_x(B, ld)
    with pytest.raises(AssertionError, match="first in image 8"):
        chunked_check(rowwise(x, B * ROWS_PER_IMAGE, ld, C, 4, wrap_bytes=P32), x, B, ld, C, 4)
    chunked_check(rowwise(x, 8 * ROWS_PER_IMAGE, ld, C, 4, wrap_bytes=P32), x, 8, ld, C, 4)       # exactly 2^12 bytes: the last offset still fits


def test_fault_row_index_truncated_and_clamped():
    B, ld, C = 12, 8, 8                                   # 192 rows, index cut to 8 signed bits: rows from 128 on land on row 0
    x = make_x(B, ld)
    with pytest.raises(AssertionError, match="first in image 8"):
        chunked_check(rowwise(x, B * ROWS_PER_IMAGE, ld, C, 4, trunc_bits=8), x, B, ld, C, 4)


def test_fault_byte_predicate_counts_elements():
    """`elements < 2^12` where `bytes < 2^12` is meant keeps the narrow form up to four times the size in f32"""
    B, ld, C = 9, 8, 8                                    # 4608 bytes, 1152 elements
    x = make_x(B, ld)
    good = launcher(x, B * ROWS_PER_IMAGE, ld, C, 4, lambda rows, ld, C, es: rows * ld * es < P32)
    chunked_check(good, x, B, ld, C, 4)
    bad = launcher(x, B * ROWS_PER_IMAGE, ld, C, 4, lambda rows, ld, C, es: rows * ld < P32)
    with pytest.raises(AssertionError, match="first in image 8"):
        chunked_check(bad, x, B, ld, C, 4)
    # under the limit both predicates pick the narrow form and both are right
    chunked_check(launcher(x[:7 * ROWS_PER_IMAGE * ld], 7 * ROWS_PER_IMAGE, ld, C, 4, lambda rows, ld, C, es: rows * ld < P32), x, 7, ld, C, 4)


def test_fault_predicate_ignores_ld():
    """`rows * C * esize < 2^12` on an operand of stride ld > C: 6 images of 16 rows x 12 floats are 4608 bytes, their live columns 3072"""
    B, ld, C = 6, 12, 8
    x = make_x(B, ld)
    good = launcher(x, B * ROWS_PER_IMAGE, ld, C, 4, lambda rows, ld, C, es: rows * ld * es < P32)
    chunked_check(good, x, B, ld, C, 4)
    bad = launcher(x, B * ROWS_PER_IMAGE, ld, C, 4, lambda rows, ld, C, es: rows * C * es < P32)
    # row 86 wraps to byte 32 = element 8 of row 0, a pad column: the compare runs over the whole stride and sees the sentinel gone there first
    with pytest.raises(AssertionError, match="first in image 0 at element 8 "):
        chunked_check(bad, x, B, ld, C, 4)


def chunk_walk(x, B, ld, C, esize, chunkB, seam_shift=0):
    """a launcher that walks the batch in chunks of chunkB images (uf_dwconv3x3_bwd); seam_shift = +1 starts every later chunk one image late
    (the seam image is dropped), -1 one image early (it is done twice, the last image never)"""
    per = ROWS_PER_IMAGE * ld
    out = torch.full((B * per + 64,), SENTINEL, dtype=x.dtype)
    for i, b0 in enumerate(range(0, B, chunkB)):
        s = b0 + (seam_shift if i else 0)
        nb = min(chunkB, B - b0)
        e = min(s + nb, B) if seam_shift >= 0 else s + nb
        out[s * per:e * per] = rowwise(x[s * per:e * per], (e - s) * ROWS_PER_IMAGE, ld, C, esize)[:(e - s) * per]
    return out


def test_fault_chunk_walk_drops_or_repeats_the_seam_image():
    B, ld, C = 11, 8, 8
    x = make_x(B, ld)
    chunked_check(chunk_walk(x, B, ld, C, 4, 5), x, B, ld, C, 4, chunk=3)
    with pytest.raises(AssertionError, match="first in image 5"):
        chunked_check(chunk_walk(x, B, ld, C, 4, 5, seam_shift=1), x, B, ld, C, 4, chunk=3)
    with pytest.raises(AssertionError, match="first in image 10"):
        chunked_check(chunk_walk(x, B, ld, C, 4, 5, seam_shift=-1), x, B, ld, C, 4, chunk=3)


# ---------------------------------------------------------------------------------------------------------------------------
# stand-ins of the reductions over the rows: g[c] = sum_r d[r][c] x[r][c] on the sparse lattice
# ---------------------------------------------------------------------------------------------------------------------------
def sparse_case(B, ld, esize, chunkB=None):
    rows, per = B * ROWS_PER_IMAGE, ROWS_PER_IMAGE * ld
    seams = () if chunkB is None else tuple(s for b0 in range(chunkB, B, chunkB) for s in (b0 - 1, b0))
    p = LT.plan(rows, ld, esize, ROWS_PER_IMAGE, extra=seams, **MARKS)
    torch.manual_seed(5)
    d = LT.fill_sparse(torch.empty(B * per), per, p["blocks"], lambda v: LT.fill_odd(v, 1))
    x = LT.fill_sparse(torch.empty(B * per), per, p["blocks"], lambda v: LT.fill_odd(v, 3))
    LT.check_sparse_sum(len(p["blocks"]) * ROWS_PER_IMAGE, 1, 3)
    ref = sum((LT.block_rows_of(d, ld, ROWS_PER_IMAGE, b, rows).double() * LT.block_rows_of(x, ld, ROWS_PER_IMAGE, b, rows).double()).sum(0) for b in p["blocks"])
    assert torch.equal(ref, (d.double() * x.double()).view(rows, ld).sum(0)), "the sum over the planner's blocks is the sum over the tensor"
    return p, d, x, ref


def reduce_rows(d, x, rows, ld, esize, wrap_bytes=None, trunc_bits=None):
    r = torch.arange(rows)
    if trunc_bits is not None:
        half = 1 << (trunc_bits - 1)
        r = (((r + half) % (2 * half)) - half).clamp(0, rows - 1)
    off = r * ld
    if wrap_bytes is not None:
        off = (off * esize % wrap_bytes) // esize
    idx = off[:, None] + torch.arange(ld)[None, :]
    return (d[idx].float() * x[idx].float()).sum(0)               # float32 accumulation, exact on the lattice


def test_sparse_lattice_clean_and_faults():
    B, ld = 12, 8
    p, d, x, ref = sparse_case(B, ld, 4)
    rows = B * ROWS_PER_IMAGE
    assert {7, 8} <= set(p["blocks"]), "a non-zero block on each side of the pretend 2^32 bytes"
    assert torch.equal(reduce_rows(d, x, rows, ld, 4).double(), ref)
    assert not torch.equal(reduce_rows(d, x, rows, ld, 4, wrap_bytes=P32).double(), ref), "a wrapped offset must move the sparse reference"
    assert not torch.equal(reduce_rows(d, x, rows, ld, 4, trunc_bits=8).double(), ref), "a truncated row index must move the sparse reference"
    # a predicate that counts elements keeps the narrow form here (1536 elements < 2^12 <= 6144 bytes)
    narrow = rows * ld < P32
    assert narrow and not rows * ld * 4 < P32
    assert not torch.equal(reduce_rows(d, x, rows, ld, 4, wrap_bytes=P32 if narrow else None).double(), ref)


def chunked_reduce(d, x, B, ld, esize, chunkB, seam_shift=0, overwrite=False):
    per = ROWS_PER_IMAGE * ld
    g = torch.zeros(ld)
    for i, b0 in enumerate(range(0, B, chunkB)):
        s = b0 + (seam_shift if i else 0)
        e = min(s + min(chunkB, B - b0), B)
        part = reduce_rows(d[s * per:e * per], x[s * per:e * per], (e - s) * ROWS_PER_IMAGE, ld, esize)
        g = part if overwrite and i else g + part
    return g


def test_sparse_lattice_chunk_walk_faults():
    """the tap / bias gradients of a chunked walk: non-zero blocks in the first chunk, in the last chunk and on both sides of every seam"""
    B, ld, chunkB = 11, 8, 5
    p, d, x, ref = sparse_case(B, ld, 4, chunkB)
    assert {0, 4, 5, 9, 10} <= set(p["blocks"])
    assert torch.equal(chunked_reduce(d, x, B, ld, 4, chunkB).double(), ref)
    assert not torch.equal(chunked_reduce(d, x, B, ld, 4, chunkB, seam_shift=1).double(), ref), "a dropped seam image must move the reference"
    assert not torch.equal(chunked_reduce(d, x, B, ld, 4, chunkB, seam_shift=-1).double(), ref), "a repeated seam image must move the reference"
    assert not torch.equal(chunked_reduce(d, x, B, ld, 4, chunkB, overwrite=True).double(), ref), "chunk gradients overwritten, not added, must move the reference"


def test_check_sparse_sum_refuses_inexact_sums():
    LT.check_sparse_sum(7 * 65536, 15, 1)
    with pytest.raises(AssertionError):
        LT.check_sparse_sum(7 * 65536, 64, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------
def test_dwconv_references_against_conv2d():
    import torch.nn.functional as Fn
    torch.manual_seed(7)
    B, H, W, C = 2, 8, 12, 8
    x, dc = torch.randint(-3, 4, (B, H, W, C)).double(), torch.randint(-1, 2, (B, H, W, C)).double()
    w9, bias = torch.randint(-2, 3, (9, C)).double(), torch.randint(-2, 3, (C,)).double()
    want = Fn.conv2d(x.permute(0, 3, 1, 2), w9.t().reshape(C, 1, 3, 3), bias, padding=1, groups=C).permute(0, 2, 3, 1)
    assert torch.equal(LT.dwconv64(x, w9, bias), want)
    xr = x.clone().requires_grad_(True)
    wr, br = w9.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    (Fn.conv2d(xr.permute(0, 3, 1, 2), wr.t().reshape(C, 1, 3, 3), br, padding=1, groups=C).permute(0, 2, 3, 1) * dc).sum().backward()
    dw9, db = LT.dw_grads64(dc, x)
    assert torch.equal(dw9, wr.grad) and torch.equal(db, br.grad)
    # the input gradient of the stencil is the stencil with flipped taps
    assert torch.equal(LT.dwconv64(dc, w9.flip(0)), xr.grad)


def test_fills_are_integers_in_range():
    t = LT.fill_odd(torch.empty(4096, dtype=BF16))
    assert set(t.double().unique().tolist()) == {-3.0, -1.0, 1.0, 3.0}
    t = LT.fill_range(torch.empty(4096, dtype=F32), 8, 15)
    assert set(t.unique().tolist()) == {float(v) for v in range(8, 16)}
    g = LT.guarded(100, F32, "cpu")
    assert LT.tail_intact(g, 100) and g.numel() == 100 + LT.GUARD
    g[100] = 0
    assert not LT.tail_intact(g, 100)


def test_count_diff_names_the_first_element():
    a = torch.zeros(1000, dtype=BF16)
    b = a.clone()
    assert LT.count_diff(a, b) == (0, -1)
    b[417] = 1
    b[900] = 2
    assert LT.count_diff(a, b) == (2, 417)
    assert LT.count_diff(torch.tensor([0.0]), torch.tensor([-0.0])) == (1, 0), "bit patterns, not values"


# ---------------------------------------------------------------------------------------------------------------------------
# the inventory
# ---------------------------------------------------------------------------------------------------------------------------
def test_inventory_names_every_size_constant():
    occ = LT.scan_sources()
    assert len(occ) >= 30, "the scan found the sources"
    unnamed = LT.unnamed_occurrences(occ)
    assert not unnamed, "size constants no row of large_tensor.INVENTORY names:\n" + "\n".join(f"{f}:{no}: {line.strip()}" for f, no, line in unnamed)
    assert not LT.stale_rows(occ), f"inventory rows that name no source line any more: {LT.stale_rows(occ)}"
    assert not LT.miscounted(occ), f"(file, text, lines expected, lines found): a named text on another number of source lines than its rows say: {LT.miscounted(occ)}"


def test_inventory_scan_catches_a_new_limit():
    occ = LT.scan_sources() + [("uf_attn.hip", 1, "    UF_REQUIRE((long long)n_windows * heads < 0x7fffffffLL, UF_ERR_SHAPE, \"new limit\");")]
    assert [f for f, _, _ in LT.unnamed_occurrences(occ)] == ["uf_attn.hip"]
    # a new limit that shares its text with a named one is not hidden by it: the text is then on one line more than its rows expect
    twin = LT.scan_sources() + [("uf_bwd.hip", 1, "    UF_REQUIRE((long long)B * H * W * C < 0x7fffffffLL, UF_ERR_SHAPE, \"another entry point\");")]
    assert not LT.unnamed_occurrences(twin) and LT.miscounted(twin) == [("uf_bwd.hip", "B * H * W * C < 0x7fffffffLL", 1, 2)]
    pad = LT.scan_sources() + [("uf_gemm.hip", 1, "    const unsigned off = ok ? row * 2u : 0xffffff00u;")]
    assert LT.miscounted(pad) == [("uf_gemm.hip", "* 2u : 0xffffff00u", 2, 3)]


def test_scan_ignores_both_kinds_of_comment():
    src = "a = 1; /* limit 0xffffffff\n still 0x7fffffff */ b = 0xffffff00u; // 65535\nc = 2;\n"
    code = LT.strip_comments(src)
    assert code.count("\n") == src.count("\n") and "0xffffff00u" in code
    assert not any(k in code for k in ("0xffffffff", "0x7fffffff", "65535"))


def test_inventory_rows_are_complete():
    for r in LT.INVENTORY:
        assert r["entry_points"] and r["predicate"] and r["crossing"], r
        assert r["kind"] == "none" or r["match"], r
    from uformer_amd import _lib
    unknown = [e for e in LT.entry_points() if e not in _lib.SIGNATURES]
    assert not unknown, f"inventory names entry points the library does not bind: {unknown}"
    assert set(LT.entry_points(True)).isdisjoint(LT.entry_points(False))
