"""CPU: the C-ABI library builds/loads and exports every symbol include/uformer_hip.h declares,
and the ctypes binding, which uformer_amd/_lib.py derives from that header, lists exactly those symbols with the types and the
struct layouts a C compiler gives them.  No compute (no GPU here)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(REPO, "include", "uformer_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(uf_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound():
    from uformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    names = declared_functions()
    assert len(names) >= 20
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/uformer_hip.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, set(_lib.SIGNATURES) ^ set(names)
    bound = _lib.load()
    assert bound.uf_version() == _lib.ABI_VERSION


def test_type_table_anchors():
    """Literal expectations, known by hand from the header, that pin the parser's type table."""
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_longlong, c_size_t, c_void_p
    from uformer_amd import _lib
    S, P, I = _lib.SIGNATURES, c_void_p, c_int
    assert S["uf_linear_fwd"] == (c_int, [P, P, P, P, I, I, I, I, I, P])
    assert S["uf_weight_fm_elems"] == (c_size_t, [I, I])
    assert S["uf_gelu_fwd"][1][2] is c_longlong
    assert S["uf_conv3x3_bwd"][1][4] is c_float
    assert [i for i, t in enumerate(S["uf_adamw_step"][1]) if t is c_double] == [6, 7, 8, 9, 10, 12]
    assert S["uf_last_error"] == (c_int, [c_char_p, c_size_t])
    assert S["uf_uformer_win4_fwd"][1][:2] == [POINTER(_lib.ModelDesc), POINTER(_lib.Block4Params)]
    assert dict(_lib.ModelDesc._fields_)["down_w_fm"] is c_void_p * 4
    assert dict(_lib.BlockParams._fields_)["shift"] is c_int32
    # every struct-pointer argument is typed as the header names it
    assert S["uf_pack_block_train"][1][0] is POINTER(_lib.BlockRawParams) and S["uf_pack_block_train"][1][7:9] == [POINTER(_lib.BlockParams), POINTER(_lib.BlockTrainParams)]
    assert S["uf_lewin_block_bwd"][1][0] is POINTER(_lib.BlockTrainParams) and S["uf_lewin_block_bwd"][1][6] is POINTER(_lib.BlockGrads)
    for half in ("uf_leff_bwd", "uf_lewin_attn_bwd"):
        assert S[half][1][0] is POINTER(_lib.BlockTrainParams) and S[half][1][5] is POINTER(_lib.BlockGrads)
    assert _lib.ABI_VERSION == 1
    assert {c.__name__ for c in _lib._structs.values()} == {"BlockParams", "BlockTrainParams", "BlockRawParams", "BlockGrads", "Block4Params", "CrossParams",
                                                            "ModelDesc", "UnetDesc"}


def _host_cc():
    for cc in ("cc", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(cc)
        if path:
            return path
    return None


def test_struct_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of every struct and field, printed by a C program that includes the header, against the generated ctypes classes."""
    from uformer_amd import _lib
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler (cc, or clang of the ROCm tree) to take sizeof / offsetof from")
    lines = ['#include <stdio.h>', '#include "uformer_hip.h"', "int main(void) {"]
    for cname, cls in _lib._structs.items():
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), "-o", exe, str(tmp_path / "layout.c")], check=True)
    got = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()}
    want = {}
    for cname, cls in _lib._structs.items():
        want[cname] = (ctypes.sizeof(cls),)
        for f, _ in cls._fields_:
            want[f"{cname}.{f}"] = (getattr(cls, f).offset, getattr(cls, f).size)
    assert len(_lib._structs) == 8 and got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    assert want["uf_block_params"] == (176,) and want["uf_block_params.qkv_dw9"] == (160, 8)          # the figures of a hand-written probe
    assert want["uf_model_desc"] == (256,) and want["uf_model_desc.cross"] == (248, 8)


GOOD_HEADER = """
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define UF_ABI_VERSION 7
typedef enum { UF_F32 = 0 } uf_dtype;
typedef struct uf_pair {
    const float* a;  float* b;      /* two on a line; a comment with uf_ghost(int) inside */
    int32_t shift, heads;           // and another uf_ghost2(
    const void* w[3];
    int32_t n[2], m;
} uf_pair;
size_t uf_bytes(int n, uf_dtype dtype);
int uf_run(const uf_pair* p, uf_pair* q /* may be NULL */, float* const* xs, const long long* numel, long long n, double lr,
           float eps, char* buf, size_t len, void* stream);
int uf_none(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_a_well_formed_sample():
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_longlong, c_size_t, c_void_p
    from uformer_amd import _lib
    structs, sigs, version = _lib.parse_header(GOOD_HEADER)
    pair = structs["uf_pair"]
    assert version == 7 and list(structs) == ["uf_pair"]
    assert pair._fields_ == [("a", c_void_p), ("b", c_void_p), ("shift", c_int32), ("heads", c_int32), ("w", c_void_p * 3), ("n", c_int32 * 2), ("m", c_int32)]
    assert (pair.w.offset, pair.n.offset, pair.m.offset, ctypes.sizeof(pair)) == (24, 48, 56, 64)
    assert sigs == {"uf_bytes": (c_size_t, [c_int, c_int]),
                    "uf_run": (c_int, [POINTER(pair), POINTER(pair), c_void_p, c_void_p, c_longlong, c_double, c_float, c_char_p, c_size_t, c_void_p]),
                    "uf_none": (c_int, [])}
    with pytest.raises(AttributeError):
        pair().c = 1


def _wrap(body):
    return "#define UF_ABI_VERSION 1\ntypedef struct uf_s { int32_t a; } uf_s;\n" + body


@pytest.mark.parametrize("body, named", [
    ("int uf_bad(uf_foo_t x, void* stream);", "uf_bad"),                                         # a type outside the table
    ("int uf_bad(const uf_foo_t* x);", "uf_bad"),                                                # ... also behind a pointer
    ("uf_foo_t uf_bad(int x);", "uf_bad"),                                                       # ... and as the result
    ("int uf_early(const uf_late* p);\ntypedef struct uf_late { int32_t a; } uf_late;", "uf_early"),   # a struct used above its definition
    ("typedef struct uf_outer { const uf_late* p; } uf_outer;\ntypedef struct uf_late { int32_t a; } uf_late;", "uf_outer.p"),
    ("int uf_cb(int (*fn)(int), void* stream);", "uf_cb"),                                       # a prototype the regex cannot take
    ("int uf_unnamed(int, float);", "uf_unnamed"),
    ("int uf_open(int a, int b;\nint uf_next(void);", "uf_open"),
    ("typedef struct uf_bits { int32_t a : 3; int32_t b; } uf_bits;", "uf_bits"),                # a bit-field
    ("typedef struct uf_arr { float* a[]; } uf_arr;", "uf_arr"),
    ("typedef struct uf_val { uf_s inner; } uf_val;", "uf_val.inner"),                           # a struct by value
    ("typedef struct uf_open { int32_t a;\nint uf_next(void);", "uf_open"),                      # an unterminated struct
    ("typedef struct uf_open { int32_t a;\nint uf_next(void);\ntypedef struct uf_t { int32_t a; } uf_t;", "uf_open"),
    ("typedef struct uf_a { int32_t a; } uf_b;", "uf_a"),
    ("static inline int uf_inline(int a) { return a; }\nint uf_next(void);", "uf_inline"),       # a uf_*( that is no prototype
    ("typedef int (*uf_fn)(int);", "uf_fn"),
    ("typedef enum { UF_A = 0 } uf_kind;", "uf_kind"),                                           # an enum the table does not know
], ids=lambda v: v if v.startswith("uf_") and " " not in v else None)
def test_parser_is_strict(body, named):
    from uformer_amd import _lib
    structs, sigs, _ = _lib.parse_header(_wrap("int uf_fine(const uf_s* s);"))           # the wrapping itself parses
    assert sigs == {"uf_fine": (ctypes.c_int, [ctypes.POINTER(structs["uf_s"])])}
    with pytest.raises(_lib.UformerHipError, match=re.escape(named)):
        _lib.parse_header(_wrap(body))


def test_parser_needs_the_abi_version():
    from uformer_amd import _lib
    with pytest.raises(_lib.UformerHipError, match="UF_ABI_VERSION"):
        _lib.parse_header("int uf_version(void);")


def test_abi_version_comes_from_the_header(monkeypatch):
    from uformer_amd import _lib
    text = open(os.path.join(REPO, "include", "uformer_hip.h")).read()
    assert "#define UF_ABI_VERSION 1\n" in text
    structs, sigs, version = _lib.parse_header(text.replace("#define UF_ABI_VERSION 1\n", "#define UF_ABI_VERSION 2\n"))
    assert version == 2 and sorted(sigs) == sorted(_lib.SIGNATURES) and list(structs) == list(_lib._structs)
    _lib.load()                                            # the real library against the real header: fine
    monkeypatch.setattr(_lib, "_lib", None)                # a fresh load() of the same library against the edited header's version
    monkeypatch.setattr(_lib, "ABI_VERSION", version)
    with pytest.raises(_lib.UformerHipError, match="ABI version mismatch: library reports 1, binding expects 2"):
        _lib.load()
    assert _lib._lib is None


def test_structs_refuse_stray_attributes():
    """A misspelt field must not become a Python attribute that the C side then reads as NULL."""
    from uformer_amd import _lib
    for cls in _lib._structs.values():
        assert cls.__slots__ == () and not hasattr(cls(), "__dict__")
    with pytest.raises(AttributeError):
        _lib.BlockParams().wqkv_fn = 1
    with pytest.raises(AttributeError):
        _lib.ModelDesc().wqkv_fn = 1
    with pytest.raises(AttributeError):
        setattr((_lib.BlockParams * 2)()[1], "norm1_v", None)
    bp = _lib.BlockParams()
    bp.wqkv_fm, bp.heads = 4096, 3                          # fields, arrays of the struct, byref and array assignment still work
    arr = (_lib.BlockParams * 2)()
    arr[1] = bp
    assert arr[1].wqkv_fm == 4096 and arr[1].heads == 3 and arr[0].wqkv_fm is None
    assert ctypes.cast(ctypes.byref(bp), ctypes.POINTER(_lib.BlockParams))[0].heads == 3


def test_packers_assign_fields_only():
    """Every packer that fills a struct from a list of names runs here on CPU tensors: with the slots a name that is no field raises,
    and each name it did assign reads back as the tensor's address."""
    import torch
    from uformer_amd import _lib, model, ops, packing, spec
    cfg = spec.arch_config("tiny32", img_size=64)                  # 4x4-window bottleneck: pack_block and pack_block4
    pk = packing.PackedModel(cfg, spec.synth_state_dict(cfg, 3), torch.bfloat16)
    assert pk.win4 and pk.bneck[0].rpb4 is not None and pk.blocks[0].wqkv_fm is not None and pk.desc.in_w27 is not None
    blk = model.LeWinTransformerBlock(32, (16, 16), 2, cross_modulator=True)
    for pack, args, skip in ((packing.pack_block, ("", 2, 4, torch.bfloat16), ("shift", "heads")), (packing.pack_cross, ("", 2, torch.bfloat16), ("heads",))):
        st, keep = pack(blk.state_dict(), *args)
        names = [n for n, _ in type(st)._fields_ if n not in skip]
        assert set(keep) <= set(names) and all(getattr(st, n) == (keep[n].data_ptr() if n in keep else None) for n in names)
    bp4, keep = packing.pack_block4(model.LeWinTransformerBlock(32, (4, 4), 2).state_dict(), "", 2, torch.float32)
    assert set(keep) == {n for n, _ in _lib.Block4Params._fields_} - {"heads"} and all(getattr(bp4, n) == t.data_ptr() for n, t in keep.items())
    un = packing.PackedUNet(spec.synth_unet_state_dict(16, 7), 16, torch.bfloat16)
    fields = {n for n, _ in _lib.UnetDesc._fields_}
    assert {k.split(".")[0] for k in un.keep} <= fields and all(getattr(un.desc, k) == t.data_ptr() for k, t in un.keep.items() if "." not in k)
    for has_mod in (False, True):
        _, g, views = ops._block_grads(32, 2, has_mod, "cpu")
        assert all(getattr(g, n) == (views[n].data_ptr() if n in views else None) for n, _ in _lib.BlockGrads._fields_)


def test_errors_cross_the_abi_as_codes():
    """Argument validation happens before any launch, so it is checkable without a GPU."""
    from uformer_amd import _lib
    lib = _lib.load()
    rc = lib.uf_linear_fwd(None, None, None, None, 64, 64, 64, 0, 0, None)
    assert rc == -6 and "null" in _lib.last_error()
    rc = lib.uf_window_partition(16, 32, 1, 12, 16, 4, 0, 4, None)
    assert rc == -1 and "H=12" in _lib.last_error()
    rc = lib.uf_window_attention_fwd(16, 16, 16, 16, None, 0, 16, 4, 2, 24, 16, 16, 0, 1, None)
    assert rc == -2 and "head_dim" in _lib.last_error()
    assert lib.uf_block_workspace_bytes(4096, 64, 1) == 4096 * 64 * 2 * 9
    with pytest.raises(_lib.UformerHipError):
        _lib.check(rc, "x")


def test_cpu_tensors_raise_no_fallback():
    import torch
    from uformer_amd import model, ops
    from uformer_amd._lib import UformerHipError
    with pytest.raises(UformerHipError):
        ops.window_partition(torch.zeros(1, 8, 8, 4), 8, 0)
    m = model.get_arch("Uformer_T", 128).eval()
    with pytest.raises(UformerHipError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 128, 128))
    with pytest.raises(UformerHipError, match="no CPU fallback"):      # the training path is HIP-only as well
        m.train()(torch.zeros(1, 3, 128, 128))


def test_product_never_imports_oracle():
    pkg = os.path.join(REPO, "uformer_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(root, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "uformer_oracle" not in txt, f
