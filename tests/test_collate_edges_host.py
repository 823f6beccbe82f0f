"""Host-side surface of the edge collation (no GPU): the lgnn_collate_edges entry, bound from
include/lgnn.h, and its argument checks, which return before any launch."""
import ctypes

from lesion_gnn_amd import _lib


def test_entries_are_bound_from_the_header():
    lib = _lib.load()
    for name in ("lgnn_collate_edges", "lgnn_collate_edges_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    params = _lib.PARAMS["lgnn_collate_edges"]
    assert [n for _, n in params] == [
        "ids", "num_sel", "src_ptr", "src_edge_ptr", "num_src_graphs", "edge_index",
        "num_src_edges", "edge_weight", "weight_bytes", "out_ptr", "out_edge_index",
        "out_edge_weight", "out_edge_ptr", "out_capacity", "err", "workspace", "workspace_bytes",
        "stream"]
    assert dict((n, c) for c, n in params)["edge_weight"] == "const void*"
    assert lib.lgnn_abi_version() == _lib.ABI_VERSION  # additions only


def test_workspace_bytes():
    f = _lib.load().lgnn_collate_edges_workspace_bytes
    assert f(0) > 0
    sizes = [f(n) for n in (0, 1, 2, 255, 256, 257, 10000, 10001)]
    assert sizes == sorted(sizes) and sizes[-1] >= 2 * 8 * 10001


def test_invalid_arguments_return_before_any_launch():
    lib, E, N = _lib.load(), _lib.LGNN_EINVAL, None
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)  # a non-NULL host address: every case below returns before a launch
    need = lib.lgnn_collate_edges_workspace_bytes(4)

    def call(ids=p, num_sel=4, src_ptr=p, src_edge_ptr=p, graphs=4, edge_index=p, edges=9,
             weight=N, weight_bytes=0, out_ptr=p, out_ei=p, out_w=N, out_eptr=p, capacity=8,
             err=p, ws=p, ws_bytes=need):
        return lib.lgnn_collate_edges(ids, num_sel, src_ptr, src_edge_ptr, graphs, edge_index,
                                      edges, weight, weight_bytes, out_ptr, out_ei, out_w,
                                      out_eptr, capacity, err, ws, ws_bytes, N)

    # a negative count
    assert call(num_sel=-1) == E
    assert call(graphs=-1) == E
    assert call(edges=-1) == E
    assert call(capacity=-1) == E
    # a required pointer that is NULL
    assert call(ids=N) == E
    assert call(src_ptr=N) == E
    assert call(src_edge_ptr=N) == E
    assert call(edge_index=N) == E
    assert call(out_ptr=N) == E
    assert call(out_ei=N) == E
    assert call(out_eptr=N) == E
    assert call(err=N) == E
    assert call(ws=N) == E
    # weights: an element size other than 4 or 8, or nowhere to write them
    for wb in (0, 1, 2, 3, 5, 16):
        assert call(weight=p, weight_bytes=wb, out_w=p) == E
    assert call(weight=p, weight_bytes=4, out_w=N) == E
    assert call(weight=p, weight_bytes=8, out_w=N) == E
    # a workspace that is too small
    assert call(ws_bytes=need - 1) == E
    assert call(ws_bytes=0) == E
    assert call(num_sel=0, ids=N, out_ptr=N, ws_bytes=lib.lgnn_collate_edges_workspace_bytes(0)
                - 1) == E
