"""ctypes binding of liblgnn.so, derived from include/lgnn.h (the one statement of the C ABI).

At import the header is parsed: its `#define LGNN_*` integers become module attributes, its
prototypes become SIGNATURES (ctypes restype / argtypes) and PARAMS (each argument's declared C
type and name). A type the parser does not know raises; nothing defaults to a pointer. `call`
marshals with PARAMS: tensors become addresses after a dtype check against the declared pointee,
lists become the host arrays the parameter declares.

The library is loaded from this package directory only (in-tree build, `make` or
``__graft_entry__.build()``). There is no fallback: if the library or a GPU is missing, every
product op raises. torch is imported first so that the HIP runtime torch ships
(libamdhip64.so.7) is the one the library binds to — one runtime per process.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# LGNN_LIB_PATH: an alternative build of the same library (A/B timing of kernel variants,
# tools/ab_lib.sh); the default is the in-tree build
LIB_PATH = os.environ.get("LGNN_LIB_PATH") or os.path.join(_HERE, "liblgnn.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lgnn.h")


class LgnnError(RuntimeError):
    pass


# ----------------------------------------------------------------------------------------------
# the header
# ----------------------------------------------------------------------------------------------

_VALUE_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
                "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_RETURN_TYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_INT4 = frozenset({torch.int32, torch.uint32})
_INT8 = frozenset({torch.int64, torch.uint64})
_ANY = frozenset(v for v in vars(torch).values() if isinstance(v, torch.dtype))
# pointee type -> the tensor dtypes a pointer to it accepts
_POINTEE_DTYPES = {
    "float": frozenset({torch.float32}), "double": frozenset({torch.float64}),
    "int32_t": _INT4, "int": _INT4, "unsigned int": _INT4, "uint32_t": _INT4,
    "int64_t": _INT8, "uint64_t": _INT8, "uint8_t": frozenset({torch.uint8}),
    "uint16_t": frozenset({torch.int16, torch.uint16, torch.bfloat16}),  # the bf16 planes
    "void": _ANY,
}
# the host arrays a list / tuple becomes, by declared type
_HOST_ARRAYS = {"const int*": ctypes.c_int, "const int64_t*": ctypes.c_int64}


def _evaluate(expr: str, names: dict, what: str) -> int:
    """An integer expression over integers, known names, + - * and parentheses."""
    toks = re.findall(r"\d+|\w+|\S", expr) + [""]  # "": the end

    def fail():
        raise LgnnError(f"lgnn.h: {what}: cannot evaluate {expr!r}")

    def factor() -> int:
        t = toks.pop(0)
        if t == "-":
            return -factor()
        if t == "(":
            v = total()
            return v if toks.pop(0) == ")" else fail()
        return int(t) if t.isdigit() else names[t] if t in names else fail()

    def term() -> int:
        v = factor()
        while toks[0] == "*":
            toks.pop(0)
            v *= factor()
        return v

    def total() -> int:
        v = term()
        while toks[0] in ("+", "-"):
            v = v + term() if toks.pop(0) == "+" else v - term()
        return v

    v = total()
    return v if toks == [""] else fail()


def parse_header(text: str):
    """(constants, signatures, params) of header text: every `#define LGNN_<NAME> <integer
    expression>`, and per prototype `<ret> lgnn_<name>(<params>);` its (restype, argtypes) and its
    [(declared C type, parameter name)]. Raises LgnnError on any type it does not know."""
    text = re.sub(r"/\*.*?\*/", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    constants: dict[str, int] = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(LGNN_\w+)[ \t]+(\S.*?)[ \t]*$", text,
                         flags=re.M):
        constants[m.group(1)] = _evaluate(m.group(2), constants, m.group(1))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs = set(re.findall(r"typedef\s+struct\s+\w*\s*\{[^}]*\}\s*(\w+)\s*;", text))
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{[^}]*\}\s*\w+\s*;", " ", text)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text).replace("}", " ")
    signatures: dict[str, tuple] = {}
    params: dict[str, list] = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        m = re.fullmatch(r"(.*?)\s*\b(lgnn_\w+) ?\((.*)\)", stmt)
        if m is None:
            if "(" in stmt:
                raise LgnnError(f"lgnn.h: cannot parse {stmt!r}")
            continue  # a forward declaration, or nothing
        ret, name, plist = _ctype_name(m.group(1)), m.group(2), m.group(3).strip()
        if ret not in _RETURN_TYPES:
            raise LgnnError(f"lgnn.h: {name}: unknown return type {ret!r}")
        decl, argtypes = [], []
        for p in ([] if plist in ("", "void") else plist.split(",")):
            pm = re.fullmatch(r"(.*?)\b(\w+)", p.strip())
            ctype = _ctype_name(pm.group(1)) if pm else ""
            if "*" in ctype:
                if _pointee(ctype) not in _POINTEE_DTYPES and _pointee(ctype) not in structs:
                    raise LgnnError(f"lgnn.h: {name}: unknown parameter type {ctype!r}")
                argtypes.append(ctypes.c_void_p)
            elif ctype in _VALUE_TYPES:
                argtypes.append(_VALUE_TYPES[ctype])
            else:
                raise LgnnError(f"lgnn.h: {name}: unknown parameter type in {p.strip()!r}")
            decl.append((ctype, pm.group(2)))
        signatures[name] = (_RETURN_TYPES[ret], argtypes)
        params[name] = decl
    return constants, signatures, params


def _ctype_name(s: str) -> str:
    """A declared type in one spelling: single spaces, each * attached to what precedes it."""
    return re.sub(r"\s*\*", "*", " ".join(s.split()))


def _pointee(ctype: str) -> str:
    """What a pointer type points at, without qualifiers: `const float* const*` -> `float`."""
    return " ".join(w for w in ctype.replace("*", " ").split() if w not in ("const", "struct"))


with open(HEADER_PATH) as _f:
    _CONSTANTS, SIGNATURES, PARAMS = parse_header(_f.read())
globals().update(_CONSTANTS)  # LGNN_ACT_ELU, LGNN_TILE_OPEN_EXTRA, ... as the header defines them
ABI_VERSION = _CONSTANTS["LGNN_ABI_VERSION"]


def _marshal_plan(decl: list) -> tuple:
    """Per parameter (tensor dtypes accepted, host array element type or None, whether that
    array holds addresses, declared type, name): everything `call` looks up per argument."""
    plan = []
    for ctype, pname in decl:
        stars = ctype.count("*")
        dtypes = _POINTEE_DTYPES.get(_pointee(ctype), frozenset()) if stars else frozenset()
        array = ctypes.c_void_p if stars == 2 else _HOST_ARRAYS.get(ctype)
        plan.append((dtypes, array, stars == 2, ctype, pname))
    return tuple(plan)


_PLANS = {name: _marshal_plan(decl) for name, decl in PARAMS.items()}

P = ctypes.c_void_p


class CeSrc(ctypes.Structure):
    """lgnn_ce_src (include/lgnn.h): the readout's CE factors the logits gradient is formed from,
    dlogits[i][c] = gloss * wt[i] / wsum * pm[i][c]."""
    _fields_ = [("pm", P), ("wt", P), ("wsum", P), ("gloss", P)]


class PlaneJob(ctypes.Structure):
    """lgnn_plane_job (include/lgnn.h): the split-3 weight planes lgnn_graph_build_planes writes
    beside the build (lgnn_weight_planes' arguments)."""
    _fields_ = [("nl", ctypes.c_int),
                ("widths", ctypes.c_int * (_CONSTANTS["LGNN_PLANE_JOB_MAX"] + 1)),
                ("W", P * _CONSTANTS["LGNN_PLANE_JOB_MAX"]), ("planes", P), ("planes_t", P)]


# ----------------------------------------------------------------------------------------------
# the library
# ----------------------------------------------------------------------------------------------

_lib = None


def bind(cdll: ctypes.CDLL, missing_ok: bool = False) -> ctypes.CDLL:
    """Type the entry points of `cdll` (this library or an alternative build of it) from
    SIGNATURES. missing_ok: skip the ones it lacks (a variant built from an older source)."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(cdll, name, None) if missing_ok else getattr(cdll, name)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return cdll


def load() -> ctypes.CDLL:
    """Load and type the library (no GPU needed to load)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LgnnError(f"{LIB_PATH} is missing: build it with `make` or __graft_entry__.build()")
    lib = bind(ctypes.CDLL(LIB_PATH))
    if lib.lgnn_abi_version() != ABI_VERSION:  # the built library is older than the header
        raise LgnnError("liblgnn.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().lgnn_status_string(status)
        raise LgnnError(f"{what} failed: {status} ({msg.decode() if msg else '?'})")


@contextlib.contextmanager
def path_option(option: int, value: int):
    """Set one of the library's process-wide path options (lgnn_set_option: the alternative kernel
    a test checks the default against) for the duration of a with-block."""
    lib = load()
    old = lib.lgnn_set_option(option, int(value))
    if old < 0:
        raise LgnnError(f"lgnn_set_option({option}, {value}) failed: {old}")
    try:
        yield
    finally:
        lib.lgnn_set_option(option, old)


def ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def stream(device: torch.device | None = None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(*tensors: torch.Tensor) -> None:
    """The product path is HIP-only: refuse CPU tensors instead of silently falling back."""
    for t in tensors:
        # meta tensors only while torch.compile / torch.export traces (shape propagation
        # through the fake kernels of library.py; nothing is launched)
        if t is not None and not t.is_cuda and not (t.is_meta and torch.compiler.is_compiling()):
            raise LgnnError("lesion_gnn_amd ops run on the GPU only (HIP kernels); got a CPU "
                            "tensor. There is no CPU fallback by design.")


# Measurement hook (bench.py's per-entry HIP-event timing): when set, every call() runs as
# _TRACER(name, args, launch) so the tracer can bracket the launch with events on its stream.
# args are the marshalled ones: addresses as int or None, scalars, ctypes arrays.
_TRACER = None


def set_tracer(tracer) -> None:
    global _TRACER
    _TRACER = tracer


def _convert(name: str, param: tuple, a, in_array: bool = False):
    """One argument off the fast path of _marshaller: not a plain tensor of an accepted dtype,
    None or a number."""
    dtypes, array, of_pointers, ctype, pname = param
    if isinstance(a, torch.Tensor):
        if a.dtype not in dtypes:
            raise LgnnError(f"{name}: parameter {pname} is declared {ctype}, got a {a.dtype} "
                            "tensor")
        return a.data_ptr()
    if in_array:
        if a is None or type(a) is int:
            return a
        raise LgnnError(f"{name}: parameter {pname} ({ctype}) takes tensors, got "
                        f"{type(a).__name__}")
    if type(a) is bool:
        return int(a)
    if type(a) in (list, tuple):
        if array is None:
            raise LgnnError(f"{name}: parameter {pname} ({ctype}) takes no list")
        if of_pointers:
            a = [_convert(name, param, e, True) for e in a]
        return (array * len(a))(*a)
    return a  # a ctypes object (byref, an array)


def _marshaller(name: str, plan: tuple):
    """The marshalling of one entry as a function of its arguments, one conditional expression
    per parameter (a loop over the parameters costs twice as much per eager launch): a plain
    tensor of an accepted dtype -> its address, None and numbers as they are, the rest to
    _convert."""
    ns = {"T": torch.Tensor, "P": torch.nn.Parameter, "convert": _convert, "name": name,
          "plan": plan}
    exprs = []
    for k, param in enumerate(plan):
        ns[f"d{k}"] = param[0]
        rest = f"convert(name, plan[{k}], a{k})"
        if param[0]:  # a pointer that takes tensors
            exprs.append(f"a{k}.data_ptr() if ((t := type(a{k})) is T or t is P) and "
                         f"a{k}.dtype in d{k} else a{k} if a{k} is None or t is int else {rest}")
        else:  # a scalar, or a struct pointer
            exprs.append(f"a{k} if (t := type(a{k})) is int or t is float else {rest}")
    params = ", ".join(f"a{k}" for k in range(len(plan)))
    exec(f"def marshal({params}):\n    return ({''.join(e + ', ' for e in exprs)})", ns)
    return ns["marshal"]


_MARSHAL = {name: _marshaller(name, plan) for name, plan in _PLANS.items()}


def marshal(name: str, args: tuple) -> tuple:
    """The arguments of entry `name` as ctypes takes them: a tensor -> its address (its dtype
    checked against the declared pointee), a list / tuple -> the host array the parameter declares
    (of addresses, int or int64_t), bool -> int; None, numbers and ctypes objects unchanged.
    The tensors stay referenced by `args` for as long as the caller holds it."""
    if len(args) != len(_PLANS[name]):
        raise LgnnError(f"{name} takes {len(_PLANS[name])} arguments, got {len(args)}")
    return _MARSHAL[name](*args)


def call(name: str, *args) -> None:
    """Launch entry `name` (marshal's argument rules) and raise on a non-zero status."""
    fn = getattr(load(), name)
    a = marshal(name, args)
    if _TRACER is None:
        check(fn(*a), name)
    else:
        check(_TRACER(name, a, lambda: fn(*a)), name)


def query(name: str, *args) -> int:
    """The value an entry returns (a count, a size, a diagnostic), arguments marshalled as by
    `call`; no status check and no tracer."""
    return getattr(load(), name)(*marshal(name, args))
