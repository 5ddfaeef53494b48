"""ctypes binding of the C-ABI shared library ``libagcn_hip.so``, derived from its one declaration.

``include/agcn_hip.h`` is the only place an entry point is written out: the sources under ``csrc/`` include it (a
definition that drifts is a compile error) and this module parses its text at import (``parse_header``) into
``DECLARATIONS``, the ctypes table ``SIGNATURES`` and the ``AGCN_ERR_*`` codes.  Importing needs the header, not the
library.

``call(name, *args)`` / ``status(name, *args)`` are the checked way in: tensors are passed as they are and converted by
the DECLARED parameter types (a wrong device, layout or element type raises before the foreign call), a
``const int* host_<name>`` parameter takes a host sequence of ints, the trailing ``void* stream`` is the current stream,
and ``call`` turns a non-zero status into a ``RuntimeError`` that names the entry point.  ``load()`` returns the bare handle for size queries and for callers that pass addresses themselves (``ptr``,
``ptr_bits``, ``stream``, ``check``).

The library is built in-tree by ``__graft_entry__.build()`` (``hipcc --offload-arch=gfx950``).  There is NO
fallback: if the library is missing or a call fails, a ``RuntimeError`` is raised (the product path never
routes through the CPU oracle or stock PyTorch operators for the hot path).
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagcn_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "agcn_hip.h")

# the closed set of types the header may use; anything else is an error of parse_header
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double}
_FP32, _FP64, _INT32 = ("fp32", (torch.float32,)), ("float64", (torch.float64,)), ("int32", (torch.int32,))
_BITS32, _ANY = ("int32", (torch.int32, torch.uint32)), ("", None)
# pointer type -> (the element kind in words, the dtypes a tensor argument may have; None: any)
_POINTERS = {"float*": _FP32, "const float*": _FP32, "double*": _FP64, "const double*": _FP64,
             "int*": _INT32, "const int*": _INT32, "unsigned*": _BITS32, "const unsigned*": _BITS32,
             "const long long*": ("int64", (torch.int64,)), "const unsigned char*": ("uint8", (torch.uint8,)),
             "void*": _ANY, "const void*": _ANY}
_TYPE_WORDS = {"const", "void", "char", "int", "long", "unsigned", "signed", "short", "float", "double", "size_t"}


def _c_type(tokens):
    return " ".join(tokens).replace(" *", "*")


def parse_header(text):
    """The header's text -> ({name: (return type, [(C type, parameter name), ...])}, {AGCN_* code: value}).  Strict: a
    declaration that does not read as ``type name(type name, ...)``, a parameter without a name or a type outside the
    closed set above raises RuntimeError naming the declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)      # the prose holds parentheses and semicolons
    codes = {m.group(1): int(m.group(2))
             for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(AGCN_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    decls = {}
    for chunk in text.split(";"):
        decl = " ".join(chunk.split())
        if decl in ("", "}"):
            continue
        m = re.fullmatch(r"([\w\s*]+?)\b(\w+) ?\(([^()]*)\)", decl)
        if m is None:
            raise RuntimeError(f"agcn_amd: cannot read the declaration `{decl}` of the C ABI header")
        ret, name = _c_type(m.group(1).replace("*", " * ").split()), m.group(2)
        if ret not in _RETURNS:
            raise RuntimeError(f"agcn_amd: return type `{ret}` outside the binding's set in `{decl}`")
        params = []
        for p in ([] if m.group(3).strip() in ("", "void") else m.group(3).split(",")):
            tokens = p.replace("*", " * ").split()
            if len(tokens) < 2 or tokens[-1] == "*" or tokens[-1] in _TYPE_WORDS:
                raise RuntimeError(f"agcn_amd: parameter `{p.strip()}` has no name in `{decl}`")
            ctype = _c_type(tokens[:-1])
            if ctype not in _SCALARS and ctype not in _POINTERS:
                raise RuntimeError(f"agcn_amd: parameter type `{ctype}` outside the binding's set in `{decl}`")
            params.append((ctype, tokens[-1]))
        decls[name] = (ret, params)
    return decls, codes


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise RuntimeError(f"agcn_amd: the C ABI header {HEADER_PATH} is missing ({e}); the binding is derived from "
                           f"it") from e


def _pointer_converter(ctype, where):
    """Tensor -> device address for one pointer parameter: None is NULL, a Python int is an address the caller vouches
    for, a tensor must be contiguous on a GPU and of the declared element type."""
    kind, dtypes = _POINTERS[ctype]
    want = f"{where}: expected a contiguous {kind + ' ' if kind else ''}GPU tensor"

    def convert(t):
        if t is None or type(t) is int:
            return t
        if not (t.is_cuda and t.is_contiguous() and (dtypes is None or t.dtype in dtypes)):
            raise RuntimeError(f"agcn_amd: {want}, got {t.dtype} {tuple(t.shape)} on {t.device} "
                               f"contiguous={t.is_contiguous()}")
        return t.data_ptr()
    return convert


def _host_ints_converter(where):
    """A HOST array for one ``const int* host_<name>`` parameter, the only pointers of the header that are not device
    pointers: a sequence of Python ints (or a numpy / CPU int array) becomes a C int array that lives for the call; None
    is NULL.  The entry point validates the values; a device tensor, a float or a bool is refused here."""
    def convert(values):
        if values is None:
            return None
        if torch.is_tensor(values):
            if values.is_cuda or values.dtype.is_floating_point or values.dtype == torch.bool:
                raise RuntimeError(f"agcn_amd: {where}: expected a host sequence of ints, got {values.dtype} on "
                                   f"{values.device}")
            values = values.tolist()
        values = list(values)
        if any(isinstance(v, bool) or int(v) != v for v in values):
            raise RuntimeError(f"agcn_amd: {where}: expected a host sequence of ints, got {values!r}")
        return (ctypes.c_int * len(values))(*[int(v) for v in values])
    return convert


def _converter(ctype, pname, name):
    if pname.startswith("host_"):
        assert ctype == "const int*", f"{name}({pname}): host arrays are `const int*`"
        return _host_ints_converter(f"{name}({pname})")
    return _pointer_converter(ctype, f"{name}({pname})")


DECLARATIONS, _CODES = parse_header(_read_header())
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = (_CODES[k] for k in ("AGCN_ERR_ARG", "AGCN_ERR_WORKSPACE",
                                                                "AGCN_ERR_UNSUPPORTED"))
# name -> (restype, argtypes): plain ctypes types, c_void_p for every pointer
SIGNATURES = {name: (_RETURNS[ret], [_SCALARS.get(t, ctypes.c_void_p) for t, _ in params])
              for name, (ret, params) in DECLARATIONS.items()}
# name -> one converter per parameter in front of the stream (None: a scalar, passed as it is), for every entry point
# that enqueues work: it returns a status and ends in `void* stream`, which status() supplies
_CONVERTERS = {}
for _name, (_ret, _params) in DECLARATIONS.items():
    if any(t in _POINTERS for t, _ in _params):
        assert _ret == "int" and _params[-1] == ("void*", "stream"), f"{_name}: not `int {_name}(..., void* stream)`"
        _CONVERTERS[_name] = tuple(_converter(t, p, _name) if t in _POINTERS else None for t, p in _params[:-1])

_lib = None


def load():
    """Load the shared library (once).  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"agcn_amd: HIP extension {LIB_PATH} not found -- run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback for the hot path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


ptr = _pointer_converter("const float*", "ptr")
ptr.__doc__ = "Device pointer of a tensor (None -> NULL).  The tensor must be contiguous fp32 on a GPU."
ptr_bits = _pointer_converter("const int*", "ptr_bits")
ptr_bits.__doc__ = "Device pointer of an int32 sign-bit-mask tensor (None -> NULL)."


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"agcn_amd: {what} failed with code {rc}")


def status(name, *args):
    """Enqueue entry point ``name`` on the current stream and return its status code.  ``args``: everything in front of
    the stream, tensors as they are (converted by the declared parameter types, see _pointer_converter)."""
    convert = _CONVERTERS.get(name)
    if convert is None:
        raise RuntimeError(f"agcn_amd: {name} is not a stream entry point of include/agcn_hip.h")
    if len(args) != len(convert):
        raise RuntimeError(f"agcn_amd: {name} takes {len(convert)} arguments in front of the stream, got {len(args)}")
    return getattr(_lib or load(), name)(*[a if c is None else c(a) for c, a in zip(convert, args)], stream())


def call(name, *args):
    """``status`` that raises RuntimeError, naming the entry point, on a non-zero code."""
    check(status(name, *args), name)
