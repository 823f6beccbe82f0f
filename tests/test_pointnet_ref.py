"""The float64 PointNet++ restatement (tests/pointnet_ref.py) against known answers, and the
preconditions of the GPU cases (tests/pointnet_cases.py) asserted on the CPU: no input sits near
an argmax tie, and the radius case reaches the 64-neighbour cap."""
import pytest
import torch
import torch.nn.functional as F

from tests import pointnet_cases as cases
from tests import pointnet_ref as ref


def test_fps_square_corners_and_centre():
    # corners 0..3, centre 4: from a corner the farthest is the opposite corner, then the two
    # remaining corners tie (lowest index first), the centre comes last
    pos = torch.tensor([[0., 0.], [1., 0.], [1., 1.], [0., 1.], [.5, .5]], dtype=torch.float64)
    assert ref.fps(pos, [5], [5], [0]).tolist() == [0, 2, 1, 3, 4]
    assert ref.fps(pos, [5], [3], [4]).tolist() == [4, 0, 1]  # centre: all corners tie -> 0
    assert ref.fps(pos, [5], [2], [3]).tolist() == [3, 1]


def test_fps_collinear_points_and_repeats():
    pos = torch.tensor([[0., 0.], [1., 0.], [2., 0.], [4., 0.], [8., 0.]], dtype=torch.float64)
    assert ref.fps(pos, [5], [4], [0]).tolist() == [0, 4, 3, 2]
    # two graphs, global indices; the second holds equal positions: d is all zero, index 0 repeats
    pos = torch.cat([pos, torch.ones(3, 2, dtype=torch.float64)])
    assert ref.fps(pos, [5, 3], [2, 3], [1, 2]).tolist() == [1, 4, 7, 5, 5]


def test_fps_counts_follow_fp32_arithmetic():
    assert ref.fps_counts([10, 64, 65, 1, 0, 3], 0.3) == [3, 20, 20, 1, 0, 1]
    assert ref.fps_counts([10, 5, 1], 0.5) == [5, 3, 1]
    assert ref.fps_counts([7], 1.0) == [7]


def test_radius_on_a_grid_between_two_spacings():
    # 5 x 5 unit grid, r between 1 and sqrt(2): the 4-neighbourhood plus the point itself
    ij = torch.stack(torch.meshgrid(torch.arange(5.), torch.arange(5.), indexing="ij"), -1)
    x = ij.reshape(25, 2).double()
    y = x[[12, 0, 9]]  # centre, a corner, an edge point
    pairs = ref.radius(x, y, 1.2, [25], [3], 32)
    assert pairs[0].tolist() == [0] * 5 + [1] * 3 + [2] * 4
    assert pairs[1].tolist() == [7, 11, 12, 13, 17, 0, 1, 5, 4, 8, 9, 14]
    assert ref.radius(x, y, 1.0, [25], [3], 32)[1].tolist() == [12, 0, 9]  # strict <
    assert ref.radius(x, y, 1.2, [25], [3], 2)[1].tolist() == [7, 11, 0, 1, 4, 8]  # the first 2


def test_split_first_layer_equals_the_concatenated_form():
    """cat[x_j, pos_j - pos_i] W1^T + b1 == U[j] - V[i] to 1e-12 in float64."""
    theirs, x, pos, sizes = cases.conv_case(37)
    idx, pairs, _ = theirs.sample(pos, sizes)
    row, col = pairs
    lin = theirs.conv.local_nn.lins[0]
    want = lin(torch.cat([x[col], pos[col] - pos[idx][row]], dim=1))
    U = torch.cat([x, pos], dim=1) @ lin.weight.T + lin.bias
    V = pos[idx] @ lin.weight[:, 37:].T
    assert (U[col] - V[row] - want).abs().max().item() <= 1e-12


def test_restatement_state_dict_has_the_reference_keys():
    m = ref.PointNet(37, 2, 5)
    keys = set(m.state_dict())
    assert "sa1_module.conv.local_nn.lins.0.weight" in keys
    assert "sa2_module.conv.local_nn.norms.1.module.num_batches_tracked" in keys
    assert "sa3_module.nn.norms.0.module.running_var" in keys
    assert {k for k in keys if k.startswith("mlp.")} == {
        f"mlp.lins.{i}.{p}" for i in range(3) for p in ("weight", "bias")}
    assert m.sa1_module.conv.local_nn.lins[0].in_features == 39


def test_empty_neighbourhood_and_empty_graph_give_zero_rows():
    x = torch.randn(4, 3, dtype=torch.float64)
    assert ref.segment_max(x, [0, 0, 3, 3, 4]).tolist()[0] == [0.0] * 3
    assert torch.equal(ref.segment_max(x, [0, 0, 3, 3, 4])[1], x[:3].max(0).values)


@pytest.mark.parametrize("c_in", list(cases.CONV_SEEDS))
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_conv_cases_are_clear_of_argmax_ties(c_in, mode):
    theirs, x, pos, sizes = cases.conv_case(c_in)
    theirs.train(mode == "train")
    gap = cases.conv_gap(theirs, x, pos, sizes)
    print(f"c_in {c_in} {mode}: top-two gap {gap:.3e}")
    assert gap >= cases.GAP


def test_model_case_is_clear_of_argmax_ties():
    """In training mode, and in eval mode after one Adam step (the two states the GPU test
    compares)."""
    b, sizes = cases.model_batch()
    assert 0 in sizes and len(sizes) == 12
    theirs = cases.reference_model().train()
    x, pos = b.x.double(), b.pos
    gaps = cases.model_gaps(theirs, x, pos, sizes)
    print("train:", {k: f"{v:.3e}" for k, v in gaps.items()})
    assert min(gaps.values()) >= cases.GAP
    opt = torch.optim.Adam(theirs.parameters(), lr=cases.MODEL_LR, weight_decay=cases.MODEL_WD)
    F.nll_loss(theirs(x, pos, sizes), b.y).backward()
    opt.step()
    gaps = cases.model_gaps(theirs.eval(), x, pos, sizes)
    print("eval after one step:", {k: f"{v:.3e}" for k, v in gaps.items()})
    assert min(gaps.values()) >= cases.GAP


def test_radius_case_reaches_the_cap():
    """The 200-node graph of the GPU radius test: at r = 0.4 some query has more than 64
    candidates in range, so the cap of 64 binds."""
    sizes = cases.GEOMETRY_SIZES
    pos = cases.points(sizes, 2, cases.GEOMETRY_SEED)
    counts = ref.fps_counts(sizes, 0.5)
    idx = ref.fps(pos, sizes, counts, [0] * len(sizes))
    capped = ref.radius(pos, pos[idx], 0.4, sizes, counts, 64)
    free = ref.radius(pos, pos[idx], 0.4, sizes, counts, 10 ** 6)
    per_query = torch.bincount(capped[0], minlength=idx.numel())
    assert per_query.max().item() == 64 and free.size(1) > capped.size(1)
