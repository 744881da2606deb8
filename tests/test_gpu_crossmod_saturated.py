"""GPU: ``uf_cross_attn_fwd`` on the saturated lattices of tests/crossmod_lattice.py -- a one-hot softmax (Hadamard-coded queries and keys, the winner
ahead by 160 in the log2 domain) and a uniform one (Wq = 0: the mean over the 64 keys).  On these inputs the whole kernel is a linear map on small
integers in its own float32 arithmetic, so the gate is exact_lattice.assert_exact on EVERY element, in all three operand types, inside a
poisoned buffer, and twice.  tests/test_crossmod_saturated_reference.py is the CPU twin (the conditions, and the faults the cases see)."""
import pytest
import torch

import crossmod_lattice as XL
import exact_lattice as X
from uformer_amd import ops

pytestmark = pytest.mark.gpu

IDS = [f"M{M}-C{C}-h{h}" for M, C, h in XL.CASES]


def run(c, dtype, pad=8):
    """the kernel on rows of stride C + pad inside a buffer whose pad columns and 8 extra rows hold a sentinel"""
    M, C = c["x"].shape
    buf = torch.full((M + 8, C + pad), X.SENTINEL, dtype=torch.float32)
    buf[:M, :C] = c["x"].float()
    buf = buf.cuda()
    d = {n: c[n].cuda() for n in ("wq", "bq", "k", "vt", "wp", "bp")}
    ops.cross_attn(buf[:M], d["wq"].to(dtype), d["bq"].float(), d["k"].to(dtype), d["vt"].to(dtype), d["wp"].to(dtype), d["bp"].float(), C=C)
    torch.cuda.synchronize()
    return buf.cpu()


@pytest.mark.parametrize("dtype", XL.MODES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", XL.CASES, ids=IDS)
@pytest.mark.parametrize("kind", XL.KINDS)
def test_cross_attn_exact_on_a_saturated_lattice(kind, case, dtype):
    M, C, heads = case
    c = XL.cross_case(kind, M, C, heads, dtype)
    for rep in range(2):
        buf = run(c, dtype)
        X.assert_exact(f"uf_cross_attn_fwd/{kind}-M{M}-C{C}-h{heads}-{X.TAG[dtype]}", buf[:M, :C], c["out"], torch.float32)
        assert bool((buf[:M, C:] == X.SENTINEL).all()) and bool((buf[M:] == X.SENTINEL).all()), "written outside the rows / columns of x"
