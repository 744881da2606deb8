"""The launch rule of uformer_amd ("Launch wrappers"): a wrapper passes tensors to ``ops._launch`` and never takes the
address of an expression's result -- such a temporary dies before the entry point runs and its block is handed to the next one.

CPU only: an ``ast`` walk over the package, and the helper against a fake library."""
import ast
import contextlib
import ctypes
import glob
import os

import pytest
import torch

from uformer_amd import _lib, ops
from uformer_amd._lib import UformerHipError

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uformer_amd")
NAMED = (ast.Name, ast.Attribute, ast.Subscript)


def address_of_temporary(source: str, filename: str = "<string>"):
    """(line, text) of every ``<expr>.data_ptr()`` and ``_ptr(<expr>)`` whose <expr> is not a name, attribute or subscript."""
    bad = []
    for node in ast.walk(ast.parse(source, filename)):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        if isinstance(f, ast.Attribute) and f.attr == "data_ptr":
            operands = [f.value]
        elif (isinstance(f, ast.Name) and f.id == "_ptr") or (isinstance(f, ast.Attribute) and f.attr == "_ptr"):
            operands = list(node.args) + [kw.value for kw in node.keywords]
        else:
            continue
        for op in operands:
            if not isinstance(op, NAMED):
                bad.append((node.lineno, ast.get_source_segment(source, node) or ast.dump(node)))
    return bad


def test_no_address_of_a_temporary_in_the_package():
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) >= 10 and any(f.endswith("ops.py") for f in files)
    bad = []
    for path in files:
        with open(path) as fh:
            bad += [(os.path.basename(path),) + hit for hit in address_of_temporary(fh.read(), path)]
    assert not bad, "address taken of an expression's result:\n" + "\n".join("%s:%d: %s" % b for b in bad)


# ops.layernorm as it stood before the launch helper: gamma, beta and the modulator are converted inside the argument expression
OLD_LAYERNORM = '''
def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, *, B: int, H: int, W: int, dtype, windowed: bool = False,
              shift: int = 0, modulator: Optional[Tensor] = None) -> Tensor:
    """x f32 (B*H*W, C) rows -> T (rows, C); optionally roll+partition+modulator (model.py:952-969)."""
    _dev(x, gamma, beta, modulator)
    dt = uf_dtype(dtype)
    x = _c(x, torch.float32)
    Cc = x.shape[-1]
    out = torch.empty((B * H * W, Cc), dtype=torch_dtype(dt), device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().uf_layernorm_fwd(_ptr(x), Cc, _ptr(_c(gamma, torch.float32)), _ptr(_c(beta, torch.float32)),
                                                _ptr(None if modulator is None else _c(modulator, torch.float32)),
                                                _ptr(out), B, H, W, Cc, int(windowed), shift, dt, _stream()),
                   "uf_layernorm_fwd")
    return out
'''


def test_the_walk_flags_the_old_layernorm_and_its_kin():
    hits = address_of_temporary(OLD_LAYERNORM)
    assert len(hits) == 3 and all("_ptr(" in text for _, text in hits)          # gamma, beta, modulator; _ptr(x) and _ptr(out) are fine
    assert [t for _, t in address_of_temporary("f(w.contiguous().data_ptr(), (a if c else b).data_ptr(), ops._ptr(g.float()))")] == \
        ["w.contiguous().data_ptr()", "(a if c else b).data_ptr()", "ops._ptr(g.float())"]
    assert address_of_temporary("f(w.data_ptr(), self.buf.data_ptr(), keep['w2'].data_ptr(), _ptr(x), _ptr(None))") \
        == [(1, "_ptr(None)")]                                                  # a constant is no tensor either: say None itself


class FakeLib:
    """Stands in for the loaded library: each entry point records its arguments and what the addresses hold at call time."""

    def __init__(self, n, rc=0):
        self.n, self.rc, self.calls = n, rc, []

    def _read(self, addr):
        return list((ctypes.c_float * self.n).from_address(addr))

    def uf_fake_entry(self, *args):
        g, b = args[0], args[2]
        self.calls.append(dict(args=args, g=self._read(g), b=self._read(b)))
        return self.rc

    def uf_last_error(self, buf, n):
        buf.value = b"fake failure"


@pytest.fixture
def fake(monkeypatch):
    def install(n, rc=0):
        lib = FakeLib(n, rc)
        monkeypatch.setattr(_lib, "load", lambda: lib)
        monkeypatch.setattr(ops, "_stream", lambda: 0x5EED)
        monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())     # torch.cuda.device(None) raises without a GPU
        return lib
    return install


def test_launch_keeps_temporaries_alive_until_the_entry_point_has_run(fake):
    n = 1024
    lib = fake(n)
    g = (torch.arange(n, dtype=torch.float32) / 8).to(torch.bfloat16)          # bf16-exact, distinct
    b = (-1 - torch.arange(n, dtype=torch.float32) / 8).to(torch.bfloat16)
    assert ops._launch("uf_fake_entry", None, g.to(torch.float32), 7, b.to(torch.float32), None, 2.5) is None
    (call,) = lib.calls
    pg, seven, pb, null, real, stream = call["args"]
    assert isinstance(pg, int) and isinstance(pb, int) and pg != 0 and pb != 0 and pg != pb
    assert call["g"] == g.float().tolist() and call["b"] == b.float().tolist()
    assert null is None and seven == 7 and type(seven) is int and real == 2.5
    assert stream == 0x5EED and len(call["args"]) == 6


def test_launch_raises_naming_the_entry_point(fake):
    fake(4, rc=3)
    t = torch.zeros(4)
    with pytest.raises(UformerHipError, match=r"uf_fake_entry failed \(code 3\): fake failure"):
        ops._launch("uf_fake_entry", None, t, 0, t)


def test_f32_keeps_none_and_converts_the_rest():
    assert ops._f32(None) is None
    t = torch.ones(3, 2)
    assert ops._f32(t) is t
    v = torch.ones(3, 2, dtype=torch.bfloat16).t()
    out = ops._f32(v)
    assert out.dtype == torch.float32 and out.is_contiguous() and torch.equal(out, v.float())
