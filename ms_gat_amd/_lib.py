"""ctypes binding of libmsgat_hip.so -- the only door between Python and the HIP kernels.

include/msgat_hip.h is the one declaration of the ABI: `parse_header` reads its constants, structures and
prototypes at import and the ctypes tables below are built from what it returns; nothing here repeats the header
by hand, and a header this module cannot read completely is an error.  `lib()` hands out the raw entry points
(status codes come back as integers), `checked()` the same entry points raising `MsgatError` on a negative
status.  There is no CPU fallback anywhere in this package: if the library is missing, both raise.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

import torch

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libmsgat_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(PKG), "include", "msgat_hip.h")

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int32)


class MsgatError(RuntimeError):
    pass


class Sell(C.Structure):
    """msgat_sell_t: degree-sorted sliced-ELLPACK form of the CSR rows / CSC columns (n_slices = 0: absent)."""


class Graph(C.Structure):
    pass


class Shape(C.Structure):
    pass


class Fwd(C.Structure):
    pass


class Bwd(C.Structure):
    pass


class Seg(C.Structure):
    pass


_STRUCTS = {"msgat_sell_t": Sell, "msgat_graph_t": Graph, "msgat_shape_t": Shape, "msgat_fwd_t": Fwd,
            "msgat_bwd_t": Bwd, "msgat_seg_t": Seg}
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "size_t": C.c_size_t,
            "float": C.c_float, "double": C.c_double}
_POINTEES = {*_SCALARS, "void", "char", "uint8_t", "uint16_t"}  # what a c_void_p / c_char_p may stand for

# Parameters whose callers hand over ctypes objects (a byref'd counter, a float array), typed as such rather than
# c_void_p.  parse_header refuses a key that names no parameter of the header or one of another C type.
_TYPED_POINTERS = {
    ("msgat_graph_count", "nnz_out"): c_int_p,
    ("msgat_graph_sell_count", "n_slices_out"): c_int_p,
    ("msgat_graph_sell_count", "n_pos_out"): c_int_p,
    ("msgat_graph_sell_count", "pair_trips_out"): c_int_p,
    ("msgat_edge_validity", "table"): c_float_p,
    ("msgat_edge_validity_backward", "table"): c_float_p,
    ("msgat_quantile_metrics", "levels"): c_float_p,
    ("msgat_quantile_grad", "levels"): c_float_p,
    ("msgat_forecast_score", "levels"): c_float_p,
}
_TYPED_POINTER_C = {c_int_p: "int32_t*", c_float_p: "const float*"}


def _ctype(text: str, where: str, field: bool = False):
    """The ctypes type of the C type `text` (`int32_t`, `const float*`, `const msgat_graph_t*`, `float* const*`) as a
    parameter or return type, or as a structure field (every pointer an address, a nested structure by value)."""
    m = re.fullmatch(r"(?:const\s+)?(\w+)((?:\s*\*(?:\s*const\b)?)*)", text.strip())
    base, stars = (m.group(1), m.group(2).count("*")) if m else (None, 0)
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and field and base in _STRUCTS:
        return _STRUCTS[base]
    if stars == 1 and not field and base in _STRUCTS:
        return C.POINTER(_STRUCTS[base])
    if stars == 1 and not field and base == "char":
        return C.c_char_p
    if stars and base in _POINTEES:
        return C.c_void_p
    raise MsgatError(f"include/msgat_hip.h: unknown type `{' '.join(text.split())}` in {where}")


def _declarators(body: str, sep: str, where: str):
    """[(type text, name)] of the `sep`-separated declarators `type name` in `body`."""
    found = [(d, re.fullmatch(r"(.*\W)(\w+)", d.strip(), re.S)) for d in body.split(sep) if d.strip()]
    for d, m in found:
        if m is None:
            raise MsgatError(f"include/msgat_hip.h: cannot read `{' '.join(d.split())}` in {where}")
    return [m.groups() for _, m in found]


def parse_header(text: str, typed_pointers=_TYPED_POINTERS):
    """(constants, structs, prototypes) of the header `text`: {MSGAT_NAME: int} from its #defines and enums,
    {msgat_x_t: [(field, ctype)]} and {function: (restype, [argtypes])}.  Raises MsgatError for a type it does not
    know, for an entry of `typed_pointers` the header does not bear out, and when anything but whitespace is left once
    comments, preprocessor lines, the extern "C" braces, enums, structures and prototypes have been taken out."""
    consts, structs, protos, c_types = {}, {}, {}, {}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts.update((n, int(v)) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MSGAT_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'\bextern\s+"C"\s*\{(.*)\}', r"\1", text, count=1, flags=re.S)

    def enum(m):
        consts.update((n, int(v)) for n, v in re.findall(r"(MSGAT_\w+)\s*=\s*(-?\d+)", m.group(1)))
        return ""

    def struct(m):
        structs[m.group(2)] = [(name, _ctype(t, f"{m.group(2)}.{name}", field=True))
                               for t, name in _declarators(m.group(1), ";", m.group(2))]
        return ""

    def function(m):
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else _declarators(params, ",", name)
        protos[name] = (_ctype(ret, name), [_ctype(t, f"{name}({p})") for t, p in params])
        c_types[name] = {p: " ".join(t.split()).replace(" *", "*") for t, p in params}
        return ""

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"((?:const\s+)?\w+\s*\*?)\s*\b(msgat_\w+)\s*\(([^()]*)\)\s*;", function, text)
    if text.strip():
        raise MsgatError(f"include/msgat_hip.h: cannot read `{' '.join(text.split())[:120]}`")
    for (fn, param), typ in typed_pointers.items():
        if c_types.get(fn, {}).get(param) != _TYPED_POINTER_C[typ]:
            raise MsgatError(f"include/msgat_hip.h: {fn} has no parameter `{_TYPED_POINTER_C[typ]} {param}`")
        protos[fn][1][list(c_types[fn]).index(param)] = typ
    return consts, structs, protos


with open(HEADER_PATH) as _f:
    _CONSTANTS, _fields, _PROTOTYPES = parse_header(_f.read())
for _cname, _cls in _STRUCTS.items():
    _cls._fields_ = _fields[_cname]

MSGAT_OK = _CONSTANTS["MSGAT_OK"]
ABI_VERSION = _CONSTANTS["MSGAT_ABI_VERSION"]
MODE_PLAIN, MODE_AGG_FIRST, MODE_PROJ_FIRST = (_CONSTANTS["MSGAT_MODE_" + m] for m in ("PLAIN", "AGG_FIRST", "PROJ_FIRST"))
SELL_SLACK = _CONSTANTS["MSGAT_SELL_SLACK"]
GUARD_FLOATS = _CONSTANTS["MSGAT_GUARD_FLOATS"]  # {norm, coef, skipped steps, largest finite norm, finite}

_lock = threading.Lock()
_handle = None
_checked = None


def _error(status: int, what: str) -> MsgatError:
    msg = lib().msgat_status_string(status)
    return MsgatError(f"{what} failed: {msg.decode() if msg else status} (status {status})")


def _raise_on_error(status, fn, args):
    """The errcheck of checked()'s entry points: a negative status raises under the entry point's own name."""
    if status < 0:
        raise _error(status, fn.__name__)
    return status


def _open(errcheck=None) -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise MsgatError(
            f"{LIB_PATH} is missing: build it with `python -m ms_gat_amd.build` "
            "(hipcc --offload-arch=gfx950). ms_gat_amd has no CPU or eager fallback.")
    h = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOTYPES.items():
        fn = getattr(h, name)  # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
        if errcheck is not None and res is C.c_int:
            fn.errcheck = errcheck
    if h.msgat_abi_version() != ABI_VERSION:
        raise MsgatError("libmsgat_hip.so ABI version mismatch; rebuild")
    return h


def lib() -> C.CDLL:
    """The loaded library, raw: an entry point returns its status code.  Raises if the library has not been built
    (no fallback path exists)."""
    global _handle
    if _handle is not None:
        return _handle
    with _lock:
        if _handle is None:
            _handle = _open()
    return _handle


def checked() -> C.CDLL:
    """The same library through a second set of function objects: an entry point that returns a negative status
    raises MsgatError naming itself; sizes, modes and yes/no answers pass through."""
    global _checked
    if _checked is not None:
        return _checked
    with _lock:
        if _checked is None:
            _checked = _open(_raise_on_error)
    return _checked


def check(status: int, what: str) -> None:
    if status != MSGAT_OK:
        raise _error(status, what)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_handle(device) -> int:
    """The current HIP stream of `device` as an integer handle.  (`torch.cuda.current_stream(...).cuda_stream` builds a
    Stream object per call, ~5 us -- a tenth of the host time of a PEMSD4-sized forward.)"""
    if _raw_stream is not None:
        return _raw_stream(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


def contract_form_name(Ca: int, Cb: int, with_ones: bool, n_positions: int, with_mix: bool) -> str:
    """Which kernel form the backward of a 1x1 convolution (with_mix) or a plain channel-pair contraction takes for this
    shape: `msgat_contract_form_name` (host only, no device needed)."""
    buf = C.create_string_buffer(160)
    checked().msgat_contract_form_name(Ca, Cb, int(with_ones), n_positions, int(with_mix), buf, 160)
    return buf.value.decode()


def exported_symbols():
    return sorted(_PROTOTYPES)
