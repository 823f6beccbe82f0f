"""Host-side surface of the graph loader (no GPU): the lgnn_collate entry and its argument checks
(which run before any launch), the epoch order and its cut into batches, the class weights, and
the reference collate of tests/loader_ref.py on a case written out by hand."""
import pytest
import torch

from lesion_gnn_amd import _lib, ops
from lesion_gnn_amd.datasets import (GraphStore, batch_bounds, class_weights, epoch_order)
from lesion_gnn_amd.utils import ClassWeights
from tests import loader_ref


def test_collate_entry_is_exported_and_refuses_bad_arguments():
    lib = _lib.load()
    for name in ("lgnn_collate", "lgnn_collate_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert [c for c, _ in _lib.PARAMS["lgnn_collate"]][:2] == ["const int64_t*", "int64_t"]
    assert _lib.LGNN_COLLATE_OVERFLOW == 1 << 30
    E = _lib.LGNN_EINVAL
    assert E == -22
    # lgnn_collate(ids, num_sel, src_ptr, num_src, x, channels, pos, dims, y, out_x, out_pos,
    #              out_y, out_batch, out_ptr, out_capacity, err, workspace, bytes, stream)
    N = None
    assert lib.lgnn_collate(N, -1, N, 4, N, 3, N, 0, N, N, N, N, N, N, 8, N, N, 0, N) == E
    assert lib.lgnn_collate(N, 4, N, 4, N, 0, N, 0, N, N, N, N, N, N, 8, N, N, 0, N) == E
    assert lib.lgnn_collate(N, 4, N, 4, N, 3, N, 1, N, N, N, N, N, N, 8, N, N, 0, N) == E
    assert lib.lgnn_collate(N, 4, N, 4, N, 3, N, 0, N, N, N, N, N, N, 8, N, N, 8, N) == E
    # the same with every pointer set: each call is wrong in one argument only
    b = torch.zeros(1 << 12, dtype=torch.uint8)  # host memory: never dereferenced
    p = (b.data_ptr() + 15) // 16 * 16
    need = lib.lgnn_collate_workspace_bytes(4)
    assert need >= 8 and lib.lgnn_collate_workspace_bytes(0) == 0
    assert lib.lgnn_collate_workspace_bytes(8) >= lib.lgnn_collate_workspace_bytes(4)
    assert lib.lgnn_collate(p, -1, p, 4, p, 3, p, 2, p, p, p, p, p, p, 8, p, p, need, N) == E
    assert lib.lgnn_collate(p, 4, p, -1, p, 3, p, 2, p, p, p, p, p, p, 8, p, p, need, N) == E
    assert lib.lgnn_collate(p, 4, p, 4, p, 3, p, 2, p, p, p, p, p, p, -1, p, p, need, N) == E
    assert lib.lgnn_collate(p, 4, p, 4, p, 0, p, 2, p, p, p, p, p, p, 8, p, p, need, N) == E
    assert lib.lgnn_collate(p, 4, p, 4, p, 3, p, 1, p, p, p, p, p, p, 8, p, p, need, N) == E
    assert lib.lgnn_collate(p, 4, p, 4, p, 3, p, 4, p, p, p, p, p, p, 8, p, p, need, N) == E
    assert lib.lgnn_collate(p, 4, p, 4, p, 3, p, 2, p, p, p, p, p, p, 8, p, p, need - 1, N) == E
    assert lib.lgnn_collate(p, 4, p, 4, p, 3, p, 2, p, p, N, p, p, p, 8, p, p, need, N) == E
    assert lib.lgnn_collate(N, 4, p, 4, p, 3, p, 2, p, p, p, p, p, p, 8, p, p, need, N) == E
    assert lib.lgnn_collate(p, 4, p, 4, N, 3, p, 2, p, p, p, p, p, p, 8, p, p, need, N) == E
    assert lib.lgnn_collate(p, 4, p, 4, p, 3, p, 2, p, p, p, p, p, N, 8, p, p, need, N) == E
    assert lib.lgnn_collate(p, 4, p, 4, p, 3, p, 2, p, p, p, p, p, p, 8, N, p, need, N) == E
    # all of out_x's stores are 16-byte stores
    assert lib.lgnn_collate(p, 4, p, 4, p, 3, p, 2, p, p + 4, p, p, p, p, 8, p, p, need, N) == E


def test_epoch_order():
    g = torch.Generator().manual_seed(5)
    a = epoch_order(37, True, g)
    assert a.dtype == torch.int64 and not a.is_cuda
    assert torch.equal(a.sort().values, torch.arange(37))
    assert not torch.equal(a, torch.arange(37))
    b = epoch_order(37, True, g)  # the next epoch from the same generator
    assert torch.equal(b.sort().values, torch.arange(37)) and not torch.equal(a, b)
    assert torch.equal(epoch_order(37, True, torch.Generator().manual_seed(5)), a)
    assert torch.equal(epoch_order(37, True, torch.Generator().manual_seed(5)),
                       torch.randperm(37, generator=torch.Generator().manual_seed(5)))
    assert torch.equal(epoch_order(37, False, g), torch.arange(37))
    assert torch.equal(epoch_order(37, False), torch.arange(37))
    # no generator: seeded from the default generator, so torch.manual_seed fixes it
    torch.manual_seed(3)
    c = epoch_order(37, True)
    d = epoch_order(37, True)
    torch.manual_seed(3)
    assert torch.equal(epoch_order(37, True), c) and not torch.equal(c, d)
    assert epoch_order(0, True, g).numel() == 0


def test_batch_bounds():
    b = batch_bounds(37, 8)
    assert b == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 37)]
    assert len(b) == 5 and b[-1][1] - b[-1][0] == 5
    assert batch_bounds(37, 8, drop_last=True) == b[:4]
    assert batch_bounds(32, 8, drop_last=True) == b[:4] == batch_bounds(32, 8)
    assert batch_bounds(0, 8) == [] == batch_bounds(0, 8, drop_last=True)
    assert batch_bounds(5, 8) == [(0, 5)] and batch_bounds(5, 8, drop_last=True) == []
    with pytest.raises(ValueError):
        batch_bounds(5, 0)


def test_class_weights_modes():
    counts = torch.tensor([6, 3, 1])
    w = class_weights(counts, ClassWeights.UNIFORM)
    assert w.dtype == torch.float32 and w.tolist() == [1.0, 1.0, 1.0]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    assert torch.equal(class_weights(counts, ClassWeights.INVERSE), f32([1 / 6, 1 / 3, 1.0]))
    assert torch.equal(class_weights(counts, ClassWeights.QUADRATIC_INVERSE),
                       f32([1 / 36, 1 / 9, 1.0]))
    assert torch.equal(class_weights(counts, ClassWeights.INVERSE_FREQUENCY),
                       f32([10 / 18, 10 / 9, 10 / 3]))
    assert torch.equal(class_weights(counts), class_weights(counts, "inverse_frequency"))
    with pytest.raises(ValueError):
        class_weights(counts, "nope")


def test_reference_collate_known_answer():
    """Three graphs of 2, 1 and 3 nodes, 2 channels; the selection (2, 0, 2)."""
    x = torch.tensor([[0., 1.], [2., 3.], [4., 5.], [6., 7.], [8., 9.], [10., 11.]])
    pos = torch.tensor([[.0, .1], [.2, .3], [.4, .5], [.6, .7], [.8, .9], [1., 1.1]],
                       dtype=torch.float64)
    y = torch.tensor([4, 0, 2])
    ptr = torch.tensor([0, 2, 3, 6])
    ox, op, oy, ob, optr = loader_ref.collate_ref(x, pos, y, ptr, [2, 0, 2])
    assert ox.tolist() == [[6., 7.], [8., 9.], [10., 11.], [0., 1.], [2., 3.],
                           [6., 7.], [8., 9.], [10., 11.]]
    assert op.tolist() == [[.6, .7], [.8, .9], [1., 1.1], [.0, .1], [.2, .3],
                           [.6, .7], [.8, .9], [1., 1.1]]
    assert oy.tolist() == [2, 4, 2]
    assert ob.tolist() == [0, 0, 0, 1, 1, 2, 2, 2]
    assert optr.tolist() == [0, 3, 5, 8]
    assert ob.dtype == optr.dtype == oy.dtype == torch.int64
    ox, op, oy, ob, optr = loader_ref.collate_ref(x, None, y, ptr, [])
    assert ox.shape == (0, 2) and op is None and oy.numel() == ob.numel() == 0
    assert optr.tolist() == [0]


def test_reference_cases_cover_the_edge_sizes():
    for G, sizes in loader_ref.STORE_SIZES.items():
        assert len(sizes) == G
    assert {1, 2, 63, 64, 65, 512} <= set(loader_ref.STORE_SIZES[37])
    for G in loader_ref.STORE_SIZES:
        for name, ids in loader_ref.id_cases(G).items():
            assert all(0 <= i < G for i in ids), (G, name)
    c = loader_ref.id_cases(37)
    assert len(set(c["repeats"])) < len(c["repeats"]) and c["empty"] == []
    assert len(c["single"]) == 1 and len(c["shuffled_subset"]) < 37


def test_cpu_tensors_raise():
    x, pos, y, ptr = loader_ref.make_store_tensors(2, 3, 2)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        GraphStore.from_tensors(x, pos, y, ptr)
    assert callable(ops.collate)
