"""Large-tensor tests: the launchers' size predicates as data, and the tools that compare a call on a tensor of 4 GiB / 2^31 elements and more with
what is already held to float64 at small shapes.  Importable without a GPU; tests/test_large_tensor_reference.py checks every tool
here on small arrays with scaled-down boundaries, tests/test_gpu_large_tensor.py uses them at the real ones.

Two comparisons:

  * operations local to an image, a row or a window: the large call against the SAME entry point run on chunks of whole images through offset
    pointers (every offset inside a chunk call is far below 2^31 bytes), bit for bit over the whole tensor (``compare_chunks``).  The chunk calls
    are the calls 2.1-2.5 hold to the float64 reference; on lattice inputs the planner's blocks are also compared with float64 directly.
  * reductions over the rows: a SPARSE lattice -- small non-zero integers in the planner's blocks (block 0, the last block, the block that
    holds each boundary offset and the one in front of it), zero everywhere else.  Float32 accumulation of such a tensor is exact in any order
    (``check_sparse_sum``), the float64 reference is a sum over those few blocks, and a row index that wraps or is cut at a boundary moves it.
"""
import os

import torch

import exact_lattice as X
from exact_lattice import SENTINEL

GIB = 1 << 30
B31, B32 = 1 << 31, 1 << 32
GUARD = 4096                        # elements of sentinel behind every output and workspace
MEMORY_CAP = 24 * GIB               # no test may hold more device memory than this
CHUNK_BYTES = 1 << 29               # a chunk of the reference driver stays at or under this many bytes in every operand

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uformer_amd", "csrc")
SIZE_CONSTANTS = ("0x7fffffff", "0xffffffff", "0xffffff00", "1LL << 40", "65535")


# ---------------------------------------------------------------------------------------------------------------------------
# the inventory: every size predicate of the launchers, and every entry point that has none
# ---------------------------------------------------------------------------------------------------------------------------
def _row(file, match, predicate, kind, entry_points, crossing, run):
    """``match``: a substring of the source line that carries the predicate (line numbers move); ``run``: True, or "not run: reason"."""
    assert kind in ("form", "chunk", "refuse", "none") and (run is True or run.startswith("not run: "))
    return {"file": file, "match": match, "predicate": predicate, "kind": kind, "entry_points": list(entry_points), "crossing": crossing, "run": run}


OVER_CAP_STREAM = "not run: the largest accepted stream, 2^33 f32 elements, is 32 GiB, over the 24 GiB cap"
OUT_OF_SCOPE_TAIL = "not run: the tail kernels of uf_train.hip index with long long throughout (out of scope of 2.6)"
OUT_OF_SCOPE_UNET = "not run: no UNet workload comes near this limit (out of scope of 2.6)"

INVENTORY = [
    # ---- form chosen by size
    _row("uf_elementwise.hip", "B * H * W * C * sizeof(T) < 0xffffffffULL", "walking stencil iff B*H*W*C*sizeof(T) < 0xffffffff, else the one-column form", "form",
         ["uf_dwconv3x3_fwd", "uf_dwconv3x3_gelu_fwd", "uf_dwconv3x3_pre_gelu_fwd", "uf_dwconv3x3_gelu_in_pre_gelu_fwd"],
         "64 x 256 x 256 x 256 f32 = 2^32 bytes; 128 such images in a 2-byte type", True),
    _row("uf_elementwise.hip", "B * H * W * ld_x * 4 < 0xffffff00LL", "LDS-DMA form iff B*H*W*ld_x*4 < 0xffffff00, else the first form", "form", ["uf_output_proj_fwd"],
         "128 x 512 x 512 rows of 32 floats = 2^32 bytes", True),
    _row("uf_elementwise.hip", "if (nt < 0x7fffffffLL)", "LDS-DMA form iff its tile count fits a grid", "form", ["uf_output_proj_fwd"],
         "2^31 tiles", "not run: unreachable -- 2^31 tiles of at least 4 x 32 pixels of 16 floats are 2^42 elements, refused two lines above at 2^32"),
    _row("uf_gemm.hip", "(long long)p.M * p.lda * 2 < 0xffffff00LL", "LDS-DMA staging iff M*lda*2 < 0xffffff00 and N*K*2 < 0xffffff00 (2-byte types, K % 64 == 0, K >= 128)", "form",
         ["uf_linear_fwd"], "M = 4194304 rows of K = 512 (2^32 bytes); every 2-byte entry point of the C ABI passes lda = K, so a padded operand cannot be built", True),
    _row("uf_gemm.hip", "(long long)p.M * p.ldo >= 0x7fffffffLL * 4", "second Downsample form iff M*ldo < 2^33 - 4", "form", ["uf_downsample_fwd", "uf_downsample_fm_fwd"],
         "2^33 output elements", "not run: the f32 output alone is 32 GiB, over the 24 GiB cap"),
    _row("uf_bwd.hip", "const bool v3 = v2 && M >= 256", "third version iff (M+64)*ldy*2 and (M+64)*ldx*2 are both < 0xffffff00, else the second", "form", ["uf_linear_wgrad"],
         "M = 16777151 at ld = 128; M = 8388544 at ld = 256 (either operand alone)", True),
    _row("uf_bwd.hip", "const bool v4 = v2 && wgrad4_shape", "fourth version (N, K multiples of 256, M >= 65536) under the same two limits, else the third / second", "form", ["uf_linear_wgrad"],
         "M = 4194240 at N = K = ld = 512", True),
    # ---- chunked walk
    _row("uf_bwd.hip", "lim_env ? lim_env : 0xffffffffULL", "chunks of whole images, each under 0xffffffff bytes; tap / bias gradients added in chunk order", "chunk", ["uf_dwconv3x3_bwd"],
         "64 x 256 x 256 x 256 f32: chunks of 63 + 1 images; 128 such images in a 2-byte type", True),
    # ---- refusals
    _row("uf_win4.hip", "B * H * W * ld < 0x7fffffffLL", "B*H*W*ld_qkv < 2^31 - 1", "refuse", ["uf_window4_attention_fwd", "uf_window4_attention_bwd"], "2^31 elements of the q | k | v rows", True),
    _row("uf_win4.hip", "n < 0x7fffffffLL * 16LL", "elements < (2^31 - 1) * 16", "refuse", ["uf_window4_partition", "uf_window4_reverse"], "2^35 elements", "not run: 2^35 elements are over the 24 GiB cap"),
    _row("uf_elementwise.hip", "B * Cin * H * W < 0x7fffffffLL", "B*Cin*H*W < 2^31 - 1 and Cin*9*E < 2^31 - 1", "refuse", ["uf_input_proj_fwd"], "2^31 image elements (8 GiB f32, 85 GiB of tokens at E = 32)",
         "not run: the token output of the largest accepted image is over the 24 GiB cap"),
    _row("uf_elementwise.hip", "H <= 65535 && B <= 65535", "H, B <= 65535 (launch grid)", "refuse", ["uf_input_proj_fwd"], "65536 image rows or images", "not run: a grid limit, not an addressing limit; the tokens of 65536 rows at any supported width are over the cap or trivial"),
    _row("uf_elementwise.hip", "(H + 3) / 4 <= 65535", "second stem form iff its grid fits", "form", ["uf_input_proj_fwd"], "262141 image rows", "not run: a grid limit, unreachable under H <= 65535 one line above"),
    _row("uf_elementwise.hip", "B * H * W * ld_x < 0xffffffffLL", "B*H*W*ld_x < 2^32 - 1, H/4 < 65535, B <= 65535", "refuse", ["uf_output_proj_fwd"], "2^32 elements = 16 GiB f32",
         True),
    _row("uf_lngemm.hip", "(long long)C < 0x7fffffffLL", "B*H*W*C < 2^31 - 1", "refuse", ["uf_ln_convqkv_fwd"], "2^31 elements", True),
    _row("uf_trainblk.hip", "B * H * W * 4 * C < 0x7fffffffLL", "B*H*W*4C < 2^31 - 1", "refuse", ["uf_lewin_block_train_fwd", "uf_leff_bwd", "uf_lewin_attn_bwd"], "2^31 hidden elements",
         "not run: the block plan keeps six hidden tensors T[M][4C]; at the largest accepted shape they are 24 GiB in a 2-byte type, and at 64 x 256 x 256, C = 64 they are 24 GiB in f32 and, "
         "with the ten T[M][C] tensors, dqkv, x1, dx1 and the three streams of the call, 23 GiB in bf16 before the chunk calls' workspace: over the 24 GiB cap"),
    _row("uf_leff2.hip", "H * W * 4LL * C * (long long)dtype_size(dtype) < 0xffffff00LL", "one image of the hidden tensor < 0xffffff00 bytes", "refuse", ["uf_dwconv_linear2_fwd"], "one image of 2^32 bytes", True),
    _row("uf_leff2.hip", "B * H * W < 0x7fffffffLL / 4", "tokens < 2^29", "refuse", ["uf_dwconv_linear2_fwd"], "2^29 tokens",
         "not run: 2^29 tokens of the narrowest hidden tensor (C = 16, 2-byte) are 64 GiB, over the 24 GiB cap"),
    _row("uf_bwd.hip", "B * H * W * C < 0x7fffffffLL", "B*H*W*C < 2^31 - 1", "refuse", ["uf_dwconv3x3_wgrad"], "128 x 256 x 256 x 256 = 2^31 elements", True),
    _row("uf_ffn.hip", "(long long)M * ld < 0x7fffffffLL * 4", "M*ld < 2^33 - 4", "refuse", ["uf_ffn_fwd"], "2^33 elements", OVER_CAP_STREAM),
    _row("uf_crossattn.hip", "(long long)M * ld < 0x7fffffffLL * 4", "M*ld < 2^33 - 4", "refuse", ["uf_cross_attn_fwd"], "2^33 elements", OVER_CAP_STREAM),
    _row("uf_model.hip", "B * H * W * 4LL * C < 0x7fffffffLL * 4", "B*H*W*4C < 2^33 - 4", "refuse", ["uf_lewin_block_fwd", "uf_leff_fwd", "uf_lewin_attn_fwd"], "2^33 hidden elements (the shapes run sit inside the limit: its own crossing is 16 GiB of 2-byte hidden tensor, twice in the workspace, over the cap)", True),
    _row("uf_conv.hip", "blocks < 0x7fffffffLL", "workgroups < 2^31 - 1", "refuse", ["uf_conv3x3_fwd", "uf_conv4s2_fwd", "uf_conv1x1_fwd"], "2^31 workgroups", OUT_OF_SCOPE_UNET),
    _row("uf_conv.hip", "B * H * W * ld_x < (1LL << 40)", "B*H*W*ld_x < 2^40", "refuse", ["uf_conv3x3_fwd", "uf_conv4s2_fwd", "uf_conv1x1_fwd"], "2^40 elements", OUT_OF_SCOPE_UNET),
    _row("uf_conv.hip", "n / 256 < 0x7fffffffLL", "elements / 256 < 2^31 - 1", "refuse", ["uf_conv1x1_nchw_fwd"], "2^39 elements", OUT_OF_SCOPE_UNET),
    _row("uf_train.hip", "uf_adamw_step: too many elements", "chunks < 2^31 - 1", "refuse", ["uf_adamw_step"], "2^31 chunks", OUT_OF_SCOPE_TAIL),
    _row("uf_train.hip", "uf_grad_scaler_check: too many elements", "chunks < 2^31 - 1", "refuse", ["uf_grad_scaler_check"], "2^31 chunks", OUT_OF_SCOPE_TAIL),
    _row("uf_train.hip", "uf_batch_ssim: workspace too small", "blocks < 2^31 - 1", "refuse", ["uf_batch_ssim"], "2^31 blocks", OUT_OF_SCOPE_TAIL),
    # ---- no predicate: every other entry point that takes an operand of M = B*H*W rows
    _row("uf_elementwise.hip", None, "none: always the one-column form (size_t offsets)", "none", ["uf_dwconv3x3_mul_dgelu"], "past 2^32 bytes", True),
    _row("uf_elementwise.hip", None, "none: int rows, size_t offsets", "none", ["uf_layernorm_fwd"], "past 2^32 bytes", True),
    _row("uf_elementwise.hip", None, "none: long long index, int rows, size_t offsets", "none", ["uf_window_partition", "uf_window_reverse"], "past 2^32 bytes", True),
    _row("uf_bwd.hip", None, "none: long long element count", "none", ["uf_gelu_fwd", "uf_gelu_bwd"], "past 2^32 bytes", True),
    _row("uf_bwd.hip", None, "none: int rows, size_t offsets; grid-stride over row blocks, sums added in workgroup order", "none", ["uf_layernorm_bwd"], "past 2^32 bytes", True),
    _row("uf_bwd.hip", None, "none: the kernel of uf_layernorm_bwd with window-order rows and a second output (int rows, size_t offsets)", "none", ["uf_layernorm_bwd_fused", "uf_layernorm_bwd_cast"],
         "past 2^32 bytes", True),
    _row("uf_bwd.hip", None, "none: long long grid-stride index, int rows, size_t offsets", "none", ["uf_residual_combine", "uf_grad_fork", "uf_qkv_grad_merge"], "past 2^32 bytes", True),
    _row("uf_bwd.hip", None, "none: int rows (m += 128: M <= 2^31 - 129), size_t offsets", "none", ["uf_rows_sum"], "past 2^32 bytes", True),
    _row("uf_bwd.hip", None, "none: its operands do not scale with M (heads x 64 x 64 in, 225 x heads out)", "none", ["uf_rpb_table_grad"], "-", "not run: no operand of it grows with the batch or the frame"),
    _row("uf_attn.hip", None, "none: int (window, head) pair, size_t offsets", "none", ["uf_window_attention_fwd"], "past 2^32 bytes", True),
    _row("uf_gemm.hip", None, "none: int rows and tiles, size_t offsets in every loader and epilogue", "none", ["uf_linear_residual_fwd", "uf_linear_pre_gelu_fwd", "uf_linear_mul_dgelu", "uf_qkv_fwd", "uf_upsample_fwd"],
         "past 2^32 bytes", True),
    _row("uf_gemm.hip", None, "none below the form limit above: int tiles, size_t offsets (second form, bf16 operands)", "none", ["uf_downsample_fwd"], "input past 2^33 bytes, output past 2^32", True),
    _row("uf_bwd.hip", None, "none: int window, size_t offsets; dS summed per (head, chunk of windows), chunks added in order", "none", ["uf_window_attention_bwd_qkv"], "dqkv past 2^32 bytes", True),
    _row("uf_bwd.hip", None, "none: the kernels of uf_window_attention_bwd_qkv with three outputs", "none", ["uf_window_attention_bwd"], "dO (row stride ldo = 8 C) past 2^32 bytes", True),
    _row("uf_bwd.hip", None, "none: long long grid-stride index, int b * H + y, size_t offsets", "none", ["uf_im2col", "uf_col2im"], "the patch matrix past 2^32 bytes", True),
    _row("uf_lngemm.hip", None, "none: int rows, size_t offsets", "none", ["uf_ln_qkv_fwd", "uf_ln_linear_gelu_fwd"], "past 2^32 bytes", True),
    _row("uf_model.hip", None, "none beyond the block limit", "none", ["uf_mlp_fwd"], "past 2^32 bytes",
         "not run: uf_mlp_fwd is uf_ffn_fwd behind the block checks (int rows, size_t offsets); see the uf_ffn_fwd row"),
    _row("uf_trainblk.hip", None, "none: int rows; uf_im2col, uf_grad_fork, uf_linear_wgrad, uf_linear_fwd / down_dx_kernel (int tile, size_t offsets), uf_residual_combine behind them", "none",
         ["uf_upsample_cat_bwd", "uf_downsample_bwd"], "the concat-buffer gradient / the patch matrix past 2^32 bytes", True),
]

# occurrences of the size constants that are no size predicate, by (file, substring of the line, what it is[, number of source lines that carry it: 1])
NOT_PREDICATES = [
    ("uf_elementwise.hip", "unsigned voff = 0xffffff00u", "out-of-range buffer offset: the DMA returns zeros (padding)"),
    ("uf_leff2.hip", "0xffffffffu : 0u", "lane mask"),
    ("uf_leff2.hip", "voff[s] = 0xffffff00u", "out-of-range buffer offset: zeros"),
    ("uf_leff2.hip", "dma_buffer_to_lds(rsrc, 0xffffff00u", "out-of-range buffer offset: padding slot"),
    ("uf_bwd.hip", "* 2u : 0xffffff00u", "out-of-range buffer offset: zeros past N / K", 3),
    ("uf_gemm.hip", "* 2u : 0xffffff00u", "out-of-range buffer offset: zeros past M / N", 2),
]


def entry_points(run=None):
    """entry points of the inventory; run=True: those with at least one row that runs, run=False: those with none"""
    ran = {e for r in INVENTORY if r["run"] is True for e in r["entry_points"]}
    every = {e for r in INVENTORY for e in r["entry_points"]}
    return sorted(every if run is None else (ran if run else every - ran))


def strip_comments(text):
    """the source text with // and /* */ comments blanked out, line breaks kept (string literals hold no comment markers in these sources)"""
    out, i, n = [], 0, len(text)
    while i < n:
        if text.startswith("//", i):
            j = text.find("\n", i)
            i = n if j < 0 else j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("".join(c if c == "\n" else " " for c in text[i:j]))
            i = j
        else:
            out.append(text[i])
            i += 1
    return "".join(out)


def scan_sources(csrc=CSRC):
    """[(file, line number, line)] of every source line that holds one of SIZE_CONSTANTS outside a comment"""
    out = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        with open(os.path.join(csrc, f)) as fh:
            text = fh.read()
        for no, (code, line) in enumerate(zip(strip_comments(text).split("\n"), text.split("\n")), 1):
            if any(c in code for c in SIZE_CONSTANTS):
                out.append((f, no, line))
    return out


def _named(inventory, not_predicates):
    """{(file, match): number of source lines expected to carry it}"""
    inventory = INVENTORY if inventory is None else inventory
    not_predicates = NOT_PREDICATES if not_predicates is None else not_predicates
    named = {}
    for f, m, n in [(r["file"], r["match"], r.get("count", 1)) for r in inventory if r["match"]] + [(e[0], e[1], e[3] if len(e) > 3 else 1) for e in not_predicates]:
        named[(f, m)] = named.get((f, m), 0) + n
    return named


def unnamed_occurrences(occ, inventory=None, not_predicates=None):
    """the occurrences no inventory row and no NOT_PREDICATES entry names"""
    named = _named(inventory, not_predicates)
    return [(f, no, line) for f, no, line in occ if not any(f == nf and m in line for nf, m in named)]


def miscounted(occ, inventory=None, not_predicates=None):
    """[(file, match, expected, found)]: a named substring carried by another number of source lines than its rows expect -- more: a limit added later
    that happens to share the text of a named one; fewer: a stale row"""
    named = _named(inventory, not_predicates)
    found = {k: sum(1 for f, _, line in occ if f == k[0] and k[1] in line) for k in named}
    return [(f, m, n, found[(f, m)]) for (f, m), n in sorted(named.items()) if found[(f, m)] != n]


def stale_rows(occ, inventory=None, not_predicates=None):
    """rows whose ``match`` names no source line any more"""
    return [(f, m) for f, m, _, found in miscounted(occ, inventory, not_predicates) if found == 0]


# ---------------------------------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------------------------------
def plan(rows, ld, esize, block_rows, byte_marks=(B31, B32), elem_marks=(B31, B32), extra=()):
    """Blocks (``block_rows`` rows each: an image, or a row block of a GEMM operand) of an operand of ``rows`` rows of stride ``ld`` elements
    of ``esize`` bytes that a wrong index width would treat differently: block 0, the last block, and for every boundary inside the operand --
    byte offsets ``byte_marks`` and element indices ``elem_marks`` from its base -- the block that holds it and the block in front of it;
    plus ``extra`` (chunk seams).  Returns {"blocks": sorted block indices, "marks": {("byte" | "elem", mark): block}, "n_blocks": n}."""
    assert rows > 0 and ld > 0 and esize in (1, 2, 4, 8) and block_rows > 0
    n_blocks = (rows + block_rows - 1) // block_rows
    extent = rows * ld                                        # elements from the base, pad columns included
    blocks, marks = {0, n_blocks - 1}, {}
    for kind, ms in (("byte", byte_marks), ("elem", elem_marks)):
        for m in ms:
            e = m // esize if kind == "byte" else m
            if e >= extent:
                continue
            blk = (e // ld) // block_rows
            marks[(kind, m)] = blk
            blocks.add(blk)
            if blk > 0:
                blocks.add(blk - 1)
    for b in extra:
        if 0 <= b < n_blocks:
            blocks.add(b)
    return {"blocks": sorted(blocks), "marks": marks, "n_blocks": n_blocks}


def chunk_images(per_image_bytes, chunk_bytes=CHUNK_BYTES):
    """whole images per chunk of the reference driver: the widest operand of a chunk stays at or under ``chunk_bytes``"""
    return max(1, chunk_bytes // max(per_image_bytes))


# ---------------------------------------------------------------------------------------------------------------------------
# comparison on the device: counts and the first differing index come back, never a large tensor
# ---------------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def count_diff(a, b):
    """(number of differing elements, flat index of the first one or -1) of two equally shaped tensors, compared as bit patterns"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    d = bits(a.reshape(-1)) != bits(b.reshape(-1))
    n = int(torch.count_nonzero(d))                       # (a sum would widen the mask to int64 first: eight bytes per element)
    return n, (int(d.to(torch.uint8).argmax()) if n else -1)


def record(name, elements, differing, **extra):
    rec = X.RECORDS.setdefault(name, {"elements": 0, "differing": 0})
    rec["elements"] += int(elements)
    rec["differing"] += int(differing)
    rec.update(extra)


def compare_chunks(name, big_outs, per_image, B, chunk, run_chunk, total=None, **extra):
    """``big_outs``: flat tensor (or a list of them) whose first B * per_image elements the large call wrote -- ``total`` of them when the last image
    is ragged (row blocks of a GEMM operand).  ``run_chunk(b0, nb)`` runs the same operation on images [b0, b0 + nb) alone and returns its output(s).
    Every element of the large output is compared, as bit patterns; the failure names the first differing image.  Records {elements, differing}
    under ``name`` (``name[i]`` for output i of several)."""
    single = torch.is_tensor(big_outs)
    bigs = [big_outs] if single else list(big_outs)
    pers = list(per_image) if isinstance(per_image, (list, tuple)) else [per_image] * len(bigs)      # outputs of several sizes per image: one entry each
    assert len(pers) == len(bigs) and (total is None or len(set(pers)) == 1)
    totals = [B * per if total is None else total for per in pers]
    assert all((B - 1) * per < t <= B * per for per, t in zip(pers, totals))
    counts, first = [0] * len(bigs), [None] * len(bigs)
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        smalls = run_chunk(b0, nb)
        smalls = [smalls] if torch.is_tensor(smalls) else list(smalls)
        assert len(smalls) == len(bigs)
        for i, (big, small) in enumerate(zip(bigs, smalls)):
            lo, hi = b0 * pers[i], min((b0 + nb) * pers[i], totals[i])
            n, idx = count_diff(big[lo:hi], small.reshape(-1)[:hi - lo])
            if n and first[i] is None:
                first[i] = (b0 + idx // pers[i], idx % pers[i])
            counts[i] += n
    for i, n in enumerate(counts):
        record(name if single else f"{name}[{i}]", totals[i], n, **extra)
    bad = [(i, n, first[i]) for i, n in enumerate(counts) if n]
    assert not bad, "; ".join(f"{name} output {i}: {n} of {totals[i]} elements of the large call differ from the same entry point run on chunks of {chunk} images; "
                              f"first in image {f[0]} at element {f[1]} of it" for i, n, f in bad)


def assert_exact_device(name, got, ref64, dtype, **extra):
    """exact_lattice.assert_exact without the trip to the host: ``got`` must hold the bits of ``ref64`` rounded once to ``dtype``"""
    assert got.dtype == dtype, f"{name}: output dtype {got.dtype}, expected {dtype}"
    n, idx = count_diff(got.reshape(-1), ref64.to(dtype).reshape(-1))
    record(name, got.numel(), n, **extra)
    assert n == 0, (f"{name}: {n} of {got.numel()} elements differ from the float64 reference rounded to {X.TAG[dtype]}; first at flat {idx}: "
                    f"got {float(got.reshape(-1)[idx])!r}, expected {float(ref64.reshape(-1)[idx])!r}")


def guarded(n, dtype, device, guard=GUARD):
    """n elements (uninitialised) with a sentinel tail behind them"""
    t = torch.empty(n + guard, dtype=dtype, device=device)
    t[n:] = SENTINEL
    return t


def tail_intact(t, n):
    return bool((t[n:] == torch.full((), SENTINEL, dtype=t.dtype, device=t.device)).all())


# ---------------------------------------------------------------------------------------------------------------------------
# fills, all in place
# ---------------------------------------------------------------------------------------------------------------------------
def fill_odd(t, amp=3):
    """whole tensor, in place: odd integers of [-amp, amp] (no zero: a dropped term always moves a sum)"""
    assert amp % 2 == 1
    return t.random_(0, amp + 1).mul_(2).sub_(amp)


def fill_range(t, lo, hi):
    """whole tensor, in place: integers of [lo, hi]"""
    return t.random_(0, hi - lo + 1).add_(lo)


def fill_sparse(t, per_block, blocks, fill):
    """zero everywhere, ``fill(view)`` on the given blocks of ``per_block`` elements"""
    t.zero_()
    for b in blocks:
        fill(t[b * per_block:(b + 1) * per_block])
    return t


def check_sparse_sum(n_terms, max_a, max_b):
    """condition 1 of exact_lattice for a sum over ``n_terms`` products of integers up to max_a, max_b: exact in float32 in any order"""
    bound = n_terms * max_a * max_b
    assert bound < X.ACC_STEPS, f"partial sums of up to {bound} lattice steps are not exact in float32"
    return bound


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references (any device), plain slicing
# ---------------------------------------------------------------------------------------------------------------------------
def dwconv64(x, w9, bias=None):
    """depthwise 3x3, zero padding 1: x (B, H, W, C), w9 (9, C) with tap = ky * 3 + kx, bias (C,) -> float64 (B, H, W, C)"""
    x = x.double()
    B, H, W, C = x.shape
    xp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = torch.zeros_like(x) if bias is None else bias.double().expand(B, H, W, C).clone()
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W] * w9[ky * 3 + kx].double()
    return out


def dw_grads64(dc, h):
    """tap and bias gradients of the depthwise 3x3: dw9[ky * 3 + kx][c] = sum dc[b, y, x, c] h[b, y + ky - 1, x + kx - 1, c], dbias[c] = sum dc"""
    dc, h = dc.double(), h.double()
    B, H, W, C = dc.shape
    hp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64, device=dc.device)
    hp[:, 1:H + 1, 1:W + 1] = h
    dw9 = torch.stack([(dc * hp[:, ky:ky + H, kx:kx + W]).sum((0, 1, 2)) for ky in range(3) for kx in range(3)])
    return dw9, dc.sum((0, 1, 2))


def block_rows_of(t, ld, block_rows, b, rows):
    """rows of block b of a flat operand of stride ld: (n, ld) view"""
    r0, r1 = b * block_rows, min((b + 1) * block_rows, rows)
    return t[r0 * ld:r1 * ld].view(r1 - r0, ld)
