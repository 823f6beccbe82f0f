"""Farthest point sampling and the bipartite radius search on the GPU (lgnn_fps,
lgnn_radius_pairs_count / lgnn_radius_pairs, lgnn_pairs_transpose), bit-exact against the float64
restatement (tests/pointnet_ref.py): the outputs are integers."""
import functools

import pytest
import torch

from tests import pointnet_cases as cases
from tests import pointnet_ref as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fps_points(dims):
    return cases.points(cases.FPS_SIZES, dims, 40 + dims)


@pytest.mark.parametrize("ratio", [0.5, 0.25, 1.0, 0.3])
def test_fps_matches_restatement(cuda, ratio):
    import lesion_gnn_amd

    sizes = cases.FPS_SIZES
    assert sizes[-1] == lesion_gnn_amd._lib.LGNN_FPS_CAPACITY + 1 and 0 in sizes
    pos = _fps_points(2)
    batch = cases.batch_of(sizes).to(cuda)
    counts = ref.fps_counts(sizes, ratio)
    want = ref.fps(pos, sizes, counts, [0] * len(sizes))
    got = lesion_gnn_amd.fps(pos.to(cuda), batch, ratio, random_start=False,
                             num_graphs=len(sizes))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    again = lesion_gnn_amd.fps(pos.float().to(cuda), batch, ratio, random_start=False,
                               num_graphs=len(sizes))  # fp32 positions widen exactly
    cases.poison(cuda)
    third = lesion_gnn_amd.fps(pos.to(cuda), batch, ratio, random_start=False,
                               num_graphs=len(sizes))
    assert torch.equal(again, got) and torch.equal(third, got)


@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_fps_explicit_start(cuda, where):
    import lesion_gnn_amd

    sizes = cases.FPS_SIZES
    start = [{"first": 0, "last": max(n - 1, 0), "middle": n // 2}[where] for n in sizes]
    pos = _fps_points(2)
    want = ref.fps(pos, sizes, ref.fps_counts(sizes, 0.5), start)
    got = lesion_gnn_amd.fps(pos.to(cuda), cases.batch_of(sizes).to(cuda), 0.5,
                             num_graphs=len(sizes), start=torch.tensor(start))
    assert torch.equal(got.cpu(), want)


def test_fps_equal_and_duplicated_positions(cuda):
    """All-equal positions: after the start every distance is zero and the graph's first point
    repeats; duplicated points are taken once before any repeats."""
    import lesion_gnn_amd

    pts = cases.points([4], 2, 9)
    pos = torch.cat([pts[:1].expand(5, 2), pts[[0, 1, 1, 2, 0, 3, 3]]])
    sizes = [5, 7]
    want = ref.fps(pos, sizes, sizes, [3, 2])
    assert want[:5].tolist() == [3, 0, 0, 0, 0] and len(set(want[5:9].tolist())) == 4
    got = lesion_gnn_amd.fps(pos.to(cuda), cases.batch_of(sizes).to(cuda), 1.0, num_graphs=2,
                             start=torch.tensor([3, 2]))
    assert torch.equal(got.cpu(), want)


def test_fps_three_dimensions_and_no_batch(cuda):
    import lesion_gnn_amd

    sizes = cases.FPS_SIZES
    pos = _fps_points(3)
    want = ref.fps(pos, sizes, ref.fps_counts(sizes, 0.5), [0] * len(sizes))
    got = lesion_gnn_amd.fps(pos.to(cuda), cases.batch_of(sizes).to(cuda), 0.5,
                             random_start=False, num_graphs=len(sizes))
    assert torch.equal(got.cpu(), want)
    one = lesion_gnn_amd.fps(pos[:300].to(cuda), ratio=0.25, random_start=False)
    assert torch.equal(one.cpu(), ref.fps(pos[:300], [300], [75], [0]))


def test_fps_random_start_is_reproducible(cuda):
    import lesion_gnn_amd

    sizes = cases.FPS_SIZES
    pos, batch = _fps_points(2).to(cuda), cases.batch_of(sizes).to(cuda)
    torch.manual_seed(123)
    a = lesion_gnn_amd.fps(pos, batch, 0.5, num_graphs=len(sizes))
    torch.manual_seed(123)
    b = lesion_gnn_amd.fps(pos, batch, 0.5, num_graphs=len(sizes))
    torch.manual_seed(123)
    n = torch.tensor(sizes, device=cuda)
    start = (torch.rand(len(sizes), device=cuda) * n.float()).long()  # torch_cluster's rule
    assert torch.equal(a, b)
    want = ref.fps(_fps_points(2), sizes, ref.fps_counts(sizes, 0.5), start.tolist())
    assert torch.equal(a.cpu(), want) and start.max().item() > 0


@functools.lru_cache(maxsize=None)
def _radius_points():
    """(pos, sizes, centroid counts, centroid indices in FPS selection order)."""
    sizes = cases.GEOMETRY_SIZES
    pos = cases.points(sizes, 2, cases.GEOMETRY_SEED)
    counts = ref.fps_counts(sizes, 0.5)
    return pos, sizes, counts, ref.fps(pos, sizes, counts, [0] * len(sizes))


def _check_pairs(cuda, x, y, sizes_x, sizes_y, r, max_nn):
    from lesion_gnn_amd import cluster

    want = ref.radius(x, y, r, sizes_x, sizes_y, max_nn)
    pg = cluster.radius_sets(x.to(cuda), y.to(cuda), cases.device_sets(sizes_x, cuda),
                             cases.device_sets(sizes_y, cuda), r, max_nn)
    assert pg.pairs.dtype == torch.int64 and torch.equal(pg.pairs.cpu(), want)
    counts = torch.bincount(want[0], minlength=y.size(0))
    assert pg.rowoff.cpu().tolist() == ref.offsets(counts.tolist())  # the counts' scan
    # the candidate-grouped view: a stable sort of the pairs by candidate
    tptr, perm = pg.transpose()
    assert torch.equal(perm.cpu(), torch.argsort(want[1], stable=True))
    assert tptr.cpu().tolist() == ref.offsets(
        torch.bincount(want[1], minlength=x.size(0)).tolist())
    return pg, want


@pytest.mark.parametrize("r", [0.2, 0.4])
@pytest.mark.parametrize("max_nn", [1, 64])
def test_radius_matches_restatement(cuda, r, max_nn):
    import lesion_gnn_amd

    pos, sizes, counts, idx = _radius_points()
    assert sizes[0] == 200 and 0 in sizes
    pg, want = _check_pairs(cuda, pos, pos[idx], sizes, counts, r, max_nn)
    if (r, max_nn) == (0.4, 64):
        assert torch.bincount(want[0]).max().item() == 64  # the cap binds
    # the public wrapper, from the batch vectors; twice and after NaN-filled memory was freed
    bx, by = cases.batch_of(sizes).to(cuda), cases.batch_of(counts).to(cuda)
    x, y = pos.to(cuda), pos[idx].to(cuda)
    got = lesion_gnn_amd.radius(x, y, r, bx, by, max_nn, num_graphs=len(sizes))
    cases.poison(cuda)
    again = lesion_gnn_amd.radius(x, y, r, bx, by, max_nn, num_graphs=len(sizes))
    assert torch.equal(got.cpu(), want) and torch.equal(again, got)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_radius_scan_lengths(cuda, N):
    """The counts' scans of lgnn_radius_pairs_count (over the queries) and lgnn_pairs_transpose
    (over the candidates) at the wave edge, the tile edge (1024) and with a carry over two tiles:
    every point is a query, so both scans have N elements; graphs of 60 points and an empty one."""
    sizes = [min(60, N - a) for a in range(0, N, 60)]
    sizes.insert(1, 0)
    pos = cases.points(sizes, 2, N)
    _check_pairs(cuda, pos, pos, sizes, sizes, 0.15, 8)


def test_radius_graphs_without_queries_and_queries_without_neighbours(cuda):
    pos, sizes, counts, idx = _radius_points()
    # no query in graphs 0 and 3 (their candidates stay); a far query in graph 5
    keep = [0, 0, counts[2], 0, counts[4], counts[5]]
    off = ref.offsets(counts)
    y = torch.cat([pos[idx[off[g]:off[g] + keep[g]]] for g in range(len(sizes))])
    y[-1] = torch.tensor([5.0, 5.0], dtype=torch.float64)
    pg, want = _check_pairs(cuda, pos, y, sizes, keep, 0.4, 64)
    assert pg.rowoff[-1].item() == pg.rowoff[-2].item() == want.size(1)  # the far query: none
    _check_pairs(cuda, pos, y[:0], sizes, [0] * len(sizes), 0.4, 64)  # no query at all


def test_radius_three_dimensions_single_graph(cuda):
    import lesion_gnn_amd

    pos = cases.points([300], 3, 5)
    y = pos[::7].contiguous()
    want = ref.radius(pos, y, 0.3, [300], [y.size(0)], 32)
    got = lesion_gnn_amd.radius(pos.to(cuda), y.to(cuda), 0.3)
    assert torch.equal(got.cpu(), want)
