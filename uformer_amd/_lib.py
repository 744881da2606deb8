"""ctypes binding of ``libuformer_hip.so``, derived at import from the C ABI declared in ``include/uformer_hip.h``.

There is NO fallback: if the library is missing or a call fails this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libuformer_hip.so")
# A/B builds and out-of-tree installs: UFORMER_HIP_LIB=/path/to/libuformer_hip.so overrides the in-tree library
LIB_PATH = os.environ.get("UFORMER_HIP_LIB", LIB_PATH)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "uformer_hip.h")

UF_F32, UF_BF16, UF_F16 = 0, 1, 2


class UformerHipError(RuntimeError):
    pass


# the module attribute of each struct of the header: the only table kept by hand
_CLASS_NAMES = {"uf_block_params": "BlockParams", "uf_block_train_params": "BlockTrainParams", "uf_block_raw_params": "BlockRawParams",
                "uf_block_grads": "BlockGrads", "uf_block4_params": "Block4Params", "uf_cross_params": "CrossParams",
                "uf_model_desc": "ModelDesc", "uf_unet_desc": "UnetDesc"}
# the closed table of by-value types (a leading `const` is dropped); a pointer to one of _POINTEES is c_void_p
_VALUES = {"int": C.c_int, "uf_dtype": C.c_int, "int32_t": C.c_int32, "size_t": C.c_size_t, "long long": C.c_longlong,
           "float": C.c_float, "double": C.c_double, "char*": C.c_char_p}
_POINTEES = r"(?:void|char|float|double|int|long long|size_t|u?int(?:8|16|32|64)_t)"
_NAME = r"([A-Za-z_]\w*)"


def _fail(what: str):
    raise UformerHipError("include/uformer_hip.h: " + what)


def _ctype(decl: str, structs: dict, where: str):
    """The ctypes type of the C type ``decl``; ``structs`` are the struct classes defined so far."""
    t = re.sub(r"\s*\*\s*", "*", decl.strip())
    t = t[len("const "):] if t.startswith("const ") else t
    if t in _VALUES:
        return _VALUES[t]
    if t.endswith("*") and t[:-1] in structs:
        return C.POINTER(structs[t[:-1]])
    if re.fullmatch(_POINTEES + r"(?:\*(?:const)?)+", t):
        return C.c_void_p
    _fail(f"type `{decl.strip()}` of `{where}` is not one the binding knows (a struct must be defined above its use)")


def _fields(cname: str, body: str, structs: dict):
    """``T a; T b, c[4];`` -> [(name, ctype)]"""
    *members, tail = body.split(";")
    if tail.strip():
        _fail(f"struct {cname} ends in `{tail.strip()}` without a `;`")
    fields = []
    for member in members:
        first, *more = [d.strip() for d in member.split(",")]
        head = re.fullmatch(rf"(.+?)\b{_NAME}(?:\[(\d+)\])?", first)
        rest = [re.fullmatch(rf"{_NAME}(?:\[(\d+)\])?", d) for d in more]
        if not head or not all(rest):
            _fail(f"cannot split field `{member.strip()}` of struct {cname}")
        t = _ctype(head[1], structs, f"{cname}.{head[2]}")
        for name, n in [head.groups()[1:]] + [r.groups() for r in rest]:
            fields.append((name, t * int(n) if n else t))
    return fields


def parse_header(text: str):
    """C ABI header text -> ({C struct name: ctypes.Structure class}, {function: (restype, [argtypes])}, UF_ABI_VERSION).

    The header is regular (typedef'd structs of scalars, pointers and arrays; plain prototypes) and this is no C parser: a
    declaration that does not fit raises UformerHipError naming it, nothing is skipped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+UF_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, re.M)
    if not version:
        _fail("no `#define UF_ABI_VERSION <integer>`")
    text = re.sub(r"#[ \t]*ifdef __cplusplus.*?#[ \t]*endif", " ", text, flags=re.S)      # extern "C" { and its closing brace
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)                                   # every other preprocessor line
    text = " ".join(text.split())
    structs, sigs, pos = {}, {}, 0
    statement = re.compile(r" ?((?:[^;{}]|\{[^{}]*\})*);")       # up to the `;` that ends it outside braces
    while text[pos:].strip():
        m = statement.match(text, pos)
        if not m:
            _fail(f"unterminated declaration `{text[pos:pos + 80].strip()} ...`")
        decl, pos = m[1].strip(), m.end()
        struct = re.fullmatch(r"typedef struct (\w+) ?\{(.*)\} ?(\w+)", decl)
        proto = re.fullmatch(r"(.+?)\b(uf_\w+) ?\((.*)\)", decl)
        enum = re.fullmatch(r"typedef enum ?\{[^{}]*\} ?(\w+)", decl)
        if struct and struct[1] == struct[3]:
            cname = struct[1]
            structs[cname] = type(_CLASS_NAMES.get(cname, cname), (C.Structure,), {
                "__slots__": (),           # no instance dict: assigning to a name that is no field raises AttributeError
                "_fields_": _fields(cname, struct[2], structs), "__doc__": f"``{cname}`` (include/uformer_hip.h)."})
        elif proto:
            res, name, params = proto.groups()
            args = [] if params.strip() in ("", "void") else [re.fullmatch(rf"(.+?)\b{_NAME}", a.strip()) for a in params.split(",")]
            if not all(args):
                _fail(f"cannot split the arguments of `{decl}`")
            sigs[name] = (_ctype(res, structs, name), [_ctype(a[1], structs, f"{name}({a[2]})") for a in args])
        elif not (enum and enum[1] in _VALUES):      # an enum travels as int, through its name in _VALUES
            _fail(f"cannot parse `{decl[:120]}`")
    missed = set(re.findall(r"\b(uf_\w+) ?\(", text)) - set(sigs)
    if missed:
        _fail(f"`{sorted(missed)[0]}(` is not part of a prototype the binding understood")
    return structs, sigs, int(version[1])


# read once per process: name -> (restype, argtypes) of every function the header declares, its structs, its UF_ABI_VERSION
with open(HEADER_PATH) as _f:
    _structs, SIGNATURES, ABI_VERSION = parse_header(_f.read())
if set(_structs) != set(_CLASS_NAMES):
    _fail(f"the structs are not those of _lib._CLASS_NAMES: {sorted(set(_structs) ^ set(_CLASS_NAMES))}")
globals().update({_CLASS_NAMES[c]: cls for c, cls in _structs.items()})      # BlockParams, ..., UnetDesc

_lock = threading.Lock()
_lib = None


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise UformerHipError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                "(hipcc --offload-arch=gfx950).  There is no CPU / PyTorch fallback for the hot path.")
        lib = C.CDLL(LIB_PATH)
        older = os.environ.get("UF_ALLOW_OLDER_LIB") == "1"   # A/B against a library of an earlier round (scripts/official_run.sh): skip what it lacks
        for name, (res, args) in SIGNATURES.items():
            if older and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)  # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        if lib.uf_version() != ABI_VERSION:
            raise UformerHipError(f"ABI version mismatch: library reports {lib.uf_version()}, binding expects {ABI_VERSION}")
        _lib = lib
    return _lib


def last_error() -> str:
    buf = C.create_string_buffer(512)
    load().uf_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise UformerHipError(f"{what} failed (code {rc}): {last_error()}")
