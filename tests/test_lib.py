"""CPU checks of the C-ABI library: it loads without a GPU, exports every symbol include/lgnn.h
declares, and the ctypes signature table, constants and structs _lib derives from the header
match this file's own parse of it; how _lib.call marshals its arguments. No compute calls."""
import ctypes
import os
import re

import pytest

from lesion_gnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgnn.h")


def declared_functions() -> dict[str, int]:
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"^\s*[a-zA-Z_][\w\s\*]*?\b(lgnn_\w+)\s*\(([^;]*?)\)\s*;", text,
                         flags=re.M | re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_header_parses():
    fns = declared_functions()
    assert "lgnn_node_linear_fwd" in fns and "lgnn_graph_build" in fns
    assert len(fns) >= 12


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_functions():
        assert hasattr(lib, name), f"liblgnn.so does not export {name}"


def test_ctypes_table_matches_header():
    fns = declared_functions()
    assert set(fns) == set(_lib.SIGNATURES), set(fns) ^ set(_lib.SIGNATURES)
    for name, nargs in fns.items():
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


def _header_text() -> str:
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _ctype(decl: str):
    """The ctypes type of one declared C type, by this file's own map (not _lib's)."""
    decl = " ".join(decl.split())
    if "*" in decl:
        return ctypes.c_char_p if decl.replace(" ", "") == "constchar*" else ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double, "size_t": ctypes.c_size_t}[decl]


def declared_prototypes() -> dict[str, tuple]:
    """name -> (restype, [argtypes]) from this file's own parse of the header."""
    out = {}
    for m in re.finditer(r"^\s*([a-zA-Z_][\w\s\*]*?)\b(lgnn_\w+)\s*\(([^;]*?)\)\s*;",
                         _header_text(), flags=re.M | re.S):
        args = m.group(3).strip()
        params = [] if args in ("", "void") else [p.strip() for p in args.split(",")]
        # a parameter is its type followed by its name: drop the trailing identifier
        out[m.group(2)] = (_ctype(m.group(1)),
                           [_ctype(re.sub(r"\w+$", "", p)) for p in params])
    return out


def test_ctypes_types_match_header():
    protos = declared_prototypes()
    assert set(protos) == set(_lib.SIGNATURES) and len(protos) == len(declared_functions())
    for name, (res, args) in protos.items():
        assert _lib.SIGNATURES[name][0] is res, name
        assert list(_lib.SIGNATURES[name][1]) == args, name
        assert len(_lib.PARAMS[name]) == len(args), name


def test_ctypes_types_pinned():
    """One entry per scalar kind, written out: float, double, int64_t / size_t, const char*,
    a size_t return, a struct pointer."""
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    F32, F64, SZ = ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    pins = {
        "lgnn_adam_step": (I32, [I32, P, P, P, P, P, P, P, F32, F32, F32, F32, F32, I32, I32,
                                 I32, P]),
        "lgnn_bn_finalize": (I32, [P, F64, P, P, F32, F32, I32, I32, P, P, P, P, P, P, P, P]),
        "lgnn_graph_build": (I32, [P, I64, I64, I32, I32, P, P, P, P, P, P, P, P, P, I64, P, P,
                                   P, SZ, P]),
        "lgnn_status_string": (ctypes.c_char_p, [I32]),
        "lgnn_graph_workspace_bytes": (SZ, [I64, I64]),
        "lgnn_gcn_stack_bwd_s3f_ce": (I32, [P, P, I32, I64, P, P, P, P, P, P, P, I64, I32, P, P,
                                            P, P, P, P, P, I32, P, P, P, P, I32, P, P]),
    }
    for name, (res, args) in pins.items():
        assert _lib.SIGNATURES[name][0] is res, name
        assert list(_lib.SIGNATURES[name][1]) == args, name
    assert _lib.PARAMS["lgnn_gcn_stack_bwd_s3f_ce"][23] == ("const struct lgnn_ce_src*", "ce")
    assert _lib.PARAMS["lgnn_graph_build"][:2] == [("const int64_t*", "edge_index"),
                                                   ("int64_t", "num_edges")]
    assert _lib.PARAMS["lgnn_adam_step"][7] == ("unsigned int*", "ticket")


def _ref_eval(expr: str, known: dict) -> int:
    """A #define's value: an integer, a parenthesised integer, or a sum of known names."""
    expr = expr.strip()
    while expr.startswith("(") and expr.endswith(")"):
        expr = expr[1:-1].strip()
    return sum(known[t] if t in known else int(t) for t in (s.strip() for s in expr.split("+")))


def test_constants_come_from_header():
    known = {}
    for m in re.finditer(r"^#define[ \t]+(LGNN_\w+)[ \t]+(\S[^\n]*)$", _header_text(), flags=re.M):
        known[m.group(1)] = _ref_eval(m.group(2), known)
    assert len(known) >= 25 and "LGNN_H" not in known
    for name, value in known.items():
        assert getattr(_lib, name) == value, name
    assert _lib.LGNN_TILE_OPEN_EXTRA == 263
    assert _lib.LGNN_EINVAL == -22
    assert _lib.LGNN_BN_GIN == 4
    assert _lib.ABI_VERSION == _lib.LGNN_ABI_VERSION == _lib.load().lgnn_abi_version()


@pytest.mark.parametrize("text", ["long lgnn_x(int a);", "int lgnn_x(unsigned a);",
                                  "int lgnn_x(long* a);", "#define LGNN_A (1 / 2)\n",
                                  "#define LGNN_A LGNN_B\n"])
def test_parser_refuses_what_it_does_not_know(text):
    with pytest.raises(_lib.LgnnError):
        _lib.parse_header(text)


def test_parser_accepts_what_it_knows():
    consts, sigs, params = _lib.parse_header(
        "#define LGNN_A 3\n#define LGNN_B (LGNN_A * (2 + LGNN_A) - 1) /* c */\n"
        "size_t lgnn_x(const float* const* a, int64_t n,\n  void* s);\nint lgnn_y(void);\n")
    assert consts == {"LGNN_A": 3, "LGNN_B": 14}
    assert sigs["lgnn_x"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p])
    assert params["lgnn_x"] == [("const float* const*", "a"), ("int64_t", "n"), ("void*", "s")]
    assert sigs["lgnn_y"] == (ctypes.c_int, []) and params["lgnn_y"] == []


def test_struct_fields_match_header():
    bodies = {m.group(2): m.group(1) for m in re.finditer(
        r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", _header_text(), flags=re.S)}
    assert set(bodies) == {"lgnn_ce_src", "lgnn_plane_job"}
    for cname, struct in (("lgnn_ce_src", _lib.CeSrc), ("lgnn_plane_job", _lib.PlaneJob)):
        fields = [re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", f).group(1)
                  for f in bodies[cname].split(";") if f.strip()]
        assert fields == [f[0] for f in struct._fields_], cname
    assert len(_lib.PlaneJob().W) == _lib.LGNN_PLANE_JOB_MAX == 8
    assert len(_lib.PlaneJob().widths) == 9


class _Recorder:
    """A tracer that records what call() hands it and launches."""

    def __init__(self):
        self.calls = []

    def __call__(self, name, args, launch):
        self.calls.append((name, args))
        return launch()

    def __enter__(self):
        _lib.set_tracer(self)
        return self

    def __exit__(self, *exc):
        _lib.set_tracer(None)


def test_call_marshals_tensors_for_the_tracer():
    """M = 0 returns LGNN_OK before any launch: no GPU is touched."""
    import torch

    X, W, Y = (torch.zeros(4, 4) for _ in range(3))
    with _Recorder() as rec:
        _lib.call("lgnn_node_linear_fwd", X, 0, 4, None, None, None, 0.0, W, None, 4, 0, Y, None,
                  None)
    (name, a), = rec.calls
    assert name == "lgnn_node_linear_fwd" and len(a) == 14
    for i, t in ((0, X), (7, W), (11, Y)):
        assert type(a[i]) is int and a[i] == t.data_ptr()
    assert all(a[i] is None for i in (3, 4, 5, 8, 12, 13))
    assert a[1:3] == (0, 4) and a[6] == 0.0 and a[9:11] == (4, 0)


def test_call_marshals_lists_for_the_tracer():
    import torch

    t = torch.zeros(4)
    with _Recorder() as rec:
        _lib.call("lgnn_reduce_jobs", 1, [t], [None], [0], [1], [0], [t], None)
    (name, a), = rec.calls
    assert name == "lgnn_reduce_jobs" and a[0] == 1
    assert all(isinstance(a[i], ctypes.Array) for i in range(1, 7))
    assert list(a[4]) == [1] and list(a[5]) == [0] and list(a[3]) == [0]
    assert a[1][0] == t.data_ptr() and a[6][0] == t.data_ptr() and a[2][0] is None
    assert a[1]._type_ is ctypes.c_void_p and a[4]._type_ is ctypes.c_int
    assert a[5]._type_ is ctypes.c_int64
    assert bool(a[2]) and a[7] is None


def test_call_checks_dtypes_before_the_launch():
    import torch

    X, W, Y = (torch.zeros(4, 4) for _ in range(3))
    bad = torch.zeros(4, 4, dtype=torch.int32)
    with _Recorder() as rec:
        with pytest.raises(_lib.LgnnError, match=r"lgnn_node_linear_fwd.*\bW\b"):
            _lib.call("lgnn_node_linear_fwd", X, 0, 4, None, None, None, 0.0, bad, None, 4, 0, Y,
                      None, None)
        # inside a pointer array too
        with pytest.raises(_lib.LgnnError, match=r"lgnn_reduce_jobs.*\bpartials\b"):
            _lib.call("lgnn_reduce_jobs", 1, [bad], [None], [0], [1], [0], [Y], None)
        # a list where a scalar is declared, and where a plain typed pointer is
        with pytest.raises(_lib.LgnnError, match=r"lgnn_node_linear_fwd.*\bM\b"):
            _lib.call("lgnn_node_linear_fwd", X, [0], 4, None, None, None, 0.0, W, None, 4, 0, Y,
                      None, None)
        with pytest.raises(_lib.LgnnError, match=r"lgnn_node_linear_fwd.*\bX\b"):
            _lib.call("lgnn_node_linear_fwd", [X], 0, 4, None, None, None, 0.0, W, None, 4, 0, Y,
                      None, None)
        # a tensor where a scalar is declared; the wrong number of arguments
        with pytest.raises(_lib.LgnnError, match=r"lgnn_node_linear_fwd.*\bK\b"):
            _lib.call("lgnn_node_linear_fwd", X, 0, Y, None, None, None, 0.0, W, None, 4, 0, Y,
                      None, None)
        with pytest.raises(_lib.LgnnError, match="lgnn_node_linear_fwd"):
            _lib.call("lgnn_node_linear_fwd", X, 0, 4)
    assert rec.calls == []
    # the allowed sets: 4-byte integers for int32_t*, 2-byte for uint16_t*, anything for void*
    allowed = {p[4]: p[0] for p in _lib._PLANS["lgnn_gat_fwd"]}
    assert allowed["rowptr"] == {torch.int32, torch.uint32}
    assert allowed["Y_bf16"] == {torch.int16, torch.uint16, torch.bfloat16}
    assert allowed["XP"] == {torch.float32} and allowed["M"] == set()
    assert {torch.uint8, torch.float32, torch.int64, torch.bfloat16} <= allowed["stream"]
    assert {p[4]: p[0] for p in _lib._PLANS["lgnn_knn_graph"]}["pos"] == {torch.float64}
    assert {p[4]: p[0] for p in _lib._PLANS["lgnn_knn_graph"]}["batch"] == \
        {torch.int64, torch.uint64}


def test_abi_version_and_status_strings():
    lib = _lib.load()
    assert lib.lgnn_abi_version() == _lib.ABI_VERSION
    assert lib.lgnn_status_string(0) == b"ok"
    assert lib.lgnn_status_string(-22) == b"invalid argument"


def test_argument_validation_without_gpu():
    lib = _lib.load()
    # invalid shapes are rejected before any launch
    assert lib.lgnn_node_linear_fwd(None, 10, 0, None, None, None, 0.0, None, None, 4, 0, None,
                                    None, None) == -22
    assert lib.lgnn_bwd_num_partials(100, 0, 128, 0) == -22
    assert lib.lgnn_bwd_num_partials(65536, 128, 128, 0) > 0
    assert lib.lgnn_graph_build(None, 0, -1, 1, 1, None, None, None, None, None, None, None,
                                None, None, 0, None, None, None, 0, None) == -22
    # too large for the 30-bit chained scan
    assert lib.lgnn_graph_build(None, 1 << 30, 1, 1, 1, 1, 1, None, None, None, None, None,
                                None, None, 0, None, None, None, 0, None) == -22


def test_product_path_refuses_cpu_tensors():
    import torch

    from lesion_gnn_amd.graph import Graph

    with pytest.raises(_lib.LgnnError):
        Graph(torch.zeros(2, 3, dtype=torch.long), 4)


def test_stack_fwd_validation_without_gpu():
    import ctypes

    lib = _lib.load()
    arr = (ctypes.c_void_p * 2)(None, None)
    widths = (ctypes.c_int * 2)(128, 128)
    assert lib.lgnn_gcn_stack_fwd(None, -1, 128, 1, None, None, None, 1, arr, arr, widths, arr,
                                  None, None) == -22
    big = (ctypes.c_int * 2)(256, 128)  # widths beyond the tile fast path are refused
    assert lib.lgnn_gcn_stack_fwd(None, 10, 128, 1, None, None, None, 1, arr, arr, big, arr,
                                  None, None) == -22
    # a conv stack needs the tile flags (closed tiles are aggregated on chip)
    assert lib.lgnn_gcn_stack_fwd(None, 10, 128, 1, 1, 1, None, 1, arr, arr, widths, arr,
                                  None, None) == -22
    assert lib.lgnn_tile_count(65) == 2 and lib.lgnn_tile_count(64) == 1


def test_dropout_seeds_distinct_without_cpu_draws():
    """Two unsalted constructions with no CPU generator draw in between (a lone conv, meta
    parameters) get different dropout seeds: derived_seed mixes a per-process counter into the
    hash of the generator state, and leaves the generator untouched."""
    import torch

    from lesion_gnn_amd import dropout

    torch.manual_seed(0)
    before = torch.default_generator.get_state().clone()
    a, b = dropout.derived_seed(), dropout.derived_seed()
    assert a != b
    assert torch.equal(torch.default_generator.get_state(), before)
    assert 0 <= a < 2 ** 62 and 0 <= b < 2 ** 62


def test_dropout_seed_reproducible_under_manual_seed():
    """Re-seeding and rebuilding reproduces a model's dropout seed, whatever was built in
    between (the seed is salted with the model's initial weights, not a process counter); two
    models with different weights get different seeds, and building leaves the generator where
    weight init left it."""
    import torch

    from lesion_gnn_amd.models.gat import GAT
    from lesion_gnn_amd.models.gcn import GCN
    from lesion_gnn_amd.models.gin import GIN

    builders = {"GCN": lambda: GCN(16, [32, 32], 3, 0.35), "GIN": lambda: GIN(16, [32, 32], 3, 0.35),
                "GAT": lambda: GAT(16, [32, 32], 3, 2, 0.35)}
    for name, build in builders.items():
        torch.manual_seed(7)
        m1 = build()
        after = torch.default_generator.get_state().clone()
        build()  # a construction in between
        torch.manual_seed(7)
        m2 = build()
        assert torch.equal(torch.default_generator.get_state(), after)
        m3 = build()
        s1, s2, s3 = (int(m._dropout_rng[0]) for m in (m1, m2, m3))
        assert s1 == s2 and s3 != s1, name


def test_dropout_scale_is_fp32_rounding_without_torch_scalars():
    """dropout.threshold_scale rounds 1 / (1 - p) to fp32 in plain Python (a torch scalar there
    was a Tensor.item() graph break under torch.compile): equal to numpy's float32 rounding."""
    import random

    import numpy as np

    from lesion_gnn_amd import dropout

    rnd = random.Random(7)
    ps = [0.0, 0.1, 0.25, 0.35, 0.5, 0.9, 1 / 3] + [rnd.random() * 0.999 for _ in range(20000)]
    for p in ps:
        thr, scale = dropout.threshold_scale(p)
        assert scale == float(np.float32(1.0 / (1.0 - p))), p
        assert thr == int(p * 16777216.0)
