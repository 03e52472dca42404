"""CPU: the host side of the multi-label (overlapping label groups) feature (mivp_amd/multilabel.py) and the float64
reference that tests/test_hip_multilabel.py holds the kernels against (tests/multilabel_ref.py).

1. ``LabelGroups``, ``MultiLabelSpec`` and the thresholds refuse each invalid argument with a ValueError;
2. worked examples of the two tables (BraTS; a pair of groups that is not nested needs ``write``);
3. the reference itself against an independent definition: ``F.binary_cross_entropy_with_logits`` on the one-hot planes,
   to 1e-12 in float64;
4. the CPU path of ``multilabel_loss`` against the reference at the kernels' bars (value 2e-5 max(1, |want|), gradient
   rel-L2 < 1e-4), with exact zeros at the invalid voxels;
5. ``group_scores`` on hand-counted tables; the header declares the entry points and the package exports the names."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multilabel_ref as R  # noqa: E402

from conftest import ROOT  # noqa: E402

F32, F64 = torch.float32, torch.float64


def ML():
    import mivp_amd
    return mivp_amd.multilabel


# ============================================================================================= 1. validation
@pytest.mark.parametrize("groups,kw", [
    ([], {}), ([(1,)] * 9, {}), ([()], {}), ([(1, 1)], {}), ([(256,)], {}), ([(-1,)], {}), ([(1.0,)], {}), ([(True,)], {}),
    ("12", {}), (3, {}), ([3], {}),
    ([(1, 2)], {}),                                               # two labels no later group contains
    ([(1, 2), (3, 4)], {}),                                       # not nested: write is needed
    ([(1,), (2,)], {"labels": (0, 1)}),                           # a group label that is not known
    ([(1,), (2,)], {"labels": (0, 1, 2, 2)}),
    ([(1,), (2,)], {"write": (1,)}), ([(1,), (2,)], {"write": (1, 300)}), ([(1,), (2,)], {"write": (1, 2.5)}),
])
def test_label_groups_refuses(groups, kw):
    with pytest.raises(ValueError):
        ML().LabelGroups(groups, **kw)


@pytest.mark.parametrize("kw", [
    {"alpha": -0.1}, {"beta": float("nan")}, {"alpha": "1"}, {"batch": 1}, {"focal_gamma": 0.5}, {"focal_gamma": -1.0},
    {"group_weights": (1.0, -1.0)}, {"group_weights": ()}, {"group_weights": (1.0,) * 9}, {"group_weights": 2.0},
    {"pos_weight": (float("inf"),)}, {"pos_weight": (1e39,)}, {"ignore_index": 1.5}, {"ignore_index": 2 ** 25},
    {"lambda_region": 0.0, "lambda_voxel": 0.0}, {"lambda_voxel": -1.0}, {"lambda_region": 1e39},
])
def test_spec_refuses(kw):
    with pytest.raises(ValueError):
        ML().MultiLabelSpec(**kw)


def test_values_are_immutable_and_comparable():
    M = ML()
    a, b = M.LabelGroups(R.BRATS), M.LabelGroups([list(g) for g in R.BRATS])
    assert a == b and hash(a) == hash(b) and a != M.LabelGroups([(1,)])
    assert repr(a) == "LabelGroups(groups=[(1, 2, 3), (2, 3), (3,)], labels=[0, 1, 2, 3], write=[1, 2, 3])"
    with pytest.raises(AttributeError):
        a.groups = ()
    s = M.MultiLabelSpec(alpha=0.3, beta=0.7, group_weights=[1, 2, 0])
    assert s == M.MultiLabelSpec(0.3, 0.7, group_weights=(1.0, 2.0, 0.0)) and "alpha=0.3" in repr(s)
    with pytest.raises(AttributeError):
        s.alpha = 1.0
    # a model keeps its configuration: the values survive deepcopy and pickle, inside the module as well
    import copy
    import pickle
    mod = M.MultiLabelLoss(a, s)
    for clone in (copy.deepcopy(mod), pickle.loads(pickle.dumps(mod))):
        assert clone.groups == a and clone.spec == s and torch.equal(clone.group_weights, mod.group_weights)


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.2, float("nan"), "0.5", True, (0.5, 0.5), (0.3, 0.5, 0.7, 0.9), (0.3, 0.5, 1.0)])
def test_thresholds_refuse(bad):
    with pytest.raises(ValueError):
        ML().logit_thresholds(bad, 3)


def test_thresholds_in_logit_space():
    M = ML()
    assert M.logit_thresholds(0.5, 3) == (0.0, 0.0, 0.0)
    got = M.logit_thresholds((0.3, 0.5, 0.7), 3)
    assert got == tuple(float(v) for v in R.logit_thresholds_np((0.3, 0.5, 0.7), 3))
    assert got[1] == 0.0 and got[0] == float(np.float32(math.log(0.3 / 0.7))) and got[0] < 0 < got[2]


def test_wrong_types_and_shapes_are_refused():
    M = ML()
    g = M.LabelGroups(R.BRATS)
    z, y = torch.zeros(2, 3, 2, 2, 2), torch.zeros(2, 1, 2, 2, 2)
    with pytest.raises(TypeError):
        M.multilabel_loss(z, y, R.BRATS)
    with pytest.raises(TypeError):
        M.multilabel_loss(z, y, g, {"alpha": 1})
    with pytest.raises(ValueError, match="2 channels.*3 groups"):
        M.multilabel_loss(z[:, :2], y, g)
    with pytest.raises(ValueError):
        M.multilabel_loss(z, y[:1], g)
    with pytest.raises(ValueError, match="one weight per group"):
        M.multilabel_loss(z, y, g, M.MultiLabelSpec(group_weights=(1.0, 2.0)))
    with pytest.raises(ValueError, match="one weight per group"):
        M.MultiLabelLoss(g, pos_weight=(1.0,))
    with pytest.raises(RuntimeError, match="GPU"):
        M.decode_groups(z, g)
    with pytest.raises(RuntimeError, match="GPU"):
        M.group_counts(y, y, g)


# ============================================================================================= 2. the tables
def test_brats_tables():
    g = ML().LabelGroups(R.BRATS)
    assert g.R == 3 and g.write == (1, 2, 3) and g.labels == (0, 1, 2, 3)
    assert g.lut.dtype == np.uint8 and g.lut.tolist() == [0, 1, 2, 2, 3, 3, 3, 3]
    m = g.member
    assert m.dtype == np.int32 and m.shape == (256,)
    assert m[:5].tolist() == [256, 256 | 1, 256 | 3, 256 | 7, 0] and not m[4:].any()
    assert np.array_equal(m, R.member_np(R.BRATS)) and np.array_equal(g.lut, R.lut_np(R.BRATS, (1, 2, 3)))


def test_groups_that_are_not_nested_need_write():
    M = ML()
    pair = [(1, 2), (3, 4)]
    with pytest.raises(ValueError, match="write"):
        M.LabelGroups(pair)
    g = M.LabelGroups(pair, write=(1, 3))
    assert g.lut.tolist() == [0, 1, 3, 3] and g.labels == (0, 1, 2, 3, 4)
    assert np.array_equal(g.member, R.member_np(pair))
    # known labels beyond the groups: valid voxels that belong to no group
    h = M.LabelGroups([(2,)], labels=(0, 1, 2))
    assert h.member[:4].tolist() == [256, 256, 257, 0] and h.write == (2,)
    for R_ in (1, 8):
        k = M.LabelGroups(R.GROUPS[R_])
        assert list(k.write) == R.default_write(R.GROUPS[R_])
        assert np.array_equal(k.lut, R.lut_np(R.GROUPS[R_], k.write)) and k.lut.shape == (1 << R_,)
    assert M.LabelGroups(R.GROUPS[8]).lut[0b10000001] == 8 and M.LabelGroups(R.GROUPS[8]).lut[0b00000101] == 3


# ============================================================================================= 3. the restatement itself
@pytest.mark.parametrize("ignore", [None, 255])
def test_reference_is_bce_with_logits_on_the_one_hot_planes(ignore):
    groups = [(1,), (2,)]
    z, y = R.inputs(2, 210, groups, 11, "ignored" if ignore is not None else "plain", ignore)
    o = R.opts(ignore_index=ignore, lambda_region=0.0)
    got, grad = R.multilabel_ref64(z, y, groups, o)
    valid = R.valid_and_targets(y, groups, ignore)[0]
    z64 = z.to(F64).clone().requires_grad_(True)
    planes = torch.stack([(y == 1.0), (y == 2.0)], dim=-1).to(F64)
    want = F.binary_cross_entropy_with_logits(z64[valid], planes[valid], reduction="mean")
    want.backward()
    want = want.detach()
    assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert float((grad - z64.grad).abs().max()) <= 1e-12
    assert bool((grad[~valid] == 0).all())


def test_reference_region_term_is_dice_by_hand():
    groups = [(1, 2), (2,)]
    z = torch.tensor([[[30.0, -30.0], [30.0, 30.0], [-30.0, -30.0], [0.0, 0.0]]])
    y = torch.tensor([[1.0, 2.0, 0.0, 7.0]])                       # the last voxel is unknown: it takes no part
    got, _ = R.multilabel_ref64(z, y, groups, R.opts(lambda_voxel=0.0))
    assert abs(float(got)) < 1e-6                                  # both groups predicted exactly
    got, _ = R.multilabel_ref64(-z, y, groups, R.opts(lambda_voxel=0.0))
    assert abs(float(got) - 1.0) < 1e-5                            # and exactly missed


# ============================================================================================= 4. the CPU path
CPU_CASES = [(Rg, i) for Rg in (1, 3, 8) for i in range(len(R.loss_cases(3)))]


@pytest.mark.parametrize("Rg,i", CPU_CASES)
def test_cpu_path_against_the_reference(Rg, i):
    M = ML()
    name, kind, o = R.loss_cases(Rg)[i]
    groups = R.GROUPS[Rg]
    dims = (5, 6, 7)
    z, y = R.inputs(2, 210, groups, 100 * Rg + i, kind, o["ignore_index"])
    ref = R.MlRef(z, y, groups, o)
    logits = z.reshape(2, *dims, Rg).permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    spec = M.MultiLabelSpec(**o)
    got = M.multilabel_loss(logits, y.reshape(2, 1, *dims), M.LabelGroups(groups), spec)
    (got * 0.37).backward()
    grad = logits.grad.permute(0, 2, 3, 4, 1).reshape(2, 210, Rg)
    want = float(ref.l64)
    assert abs(float(got.detach()) - want) <= R.LOSS_VALUE_BAR * max(1.0, abs(want)), (name, float(got.detach()), want)
    assert bool((grad[~ref.valid] == 0).all()), name
    assert not ref.zero
    assert R.rel_l2(grad, 0.37 * ref.g64) < R.LOSS_L2_BAR, name
    # the module form, labels without the channel axis, float64 logits
    mod = M.MultiLabelLoss(M.LabelGroups(groups), spec)
    got2 = mod(logits.detach().double(), y.reshape(2, *dims).to(torch.int64) if kind in ("plain", "absent") else y.reshape(2, *dims))
    assert abs(float(got2) - want) <= 1e-9 * max(1.0, abs(want)), name


def test_step_loss_uses_the_module():
    from argparse import Namespace
    from mivp_amd import train
    M = ML()
    groups = M.LabelGroups(R.BRATS)
    mod = M.MultiLabelLoss(groups, alpha=0.3, beta=0.7)
    z, y = R.inputs(2, 64, R.BRATS, 3)
    logits, tgt = z.reshape(2, 4, 4, 4, 3).permute(0, 4, 1, 2, 3), y.reshape(2, 1, 4, 4, 4)
    conf = Namespace(training_mode="downstream", seg_loss=mod, include_background=True)
    got = train.step_loss({"downstream": logits}, conf, tgt)
    want, _ = R.multilabel_ref64(z, y, R.BRATS, R.opts(0.3, 0.7))
    assert abs(float(got) - float(want)) <= R.LOSS_VALUE_BAR * max(1.0, abs(float(want)))
    assert "LabelGroups" in repr(mod) and "alpha=0.3" in repr(mod)


# ============================================================================================= 5. scores, header, exports
def test_group_scores_by_hand():
    M = ML()
    s = M.group_scores(np.array([[3, 4, 6], [0, 0, 5], [0, 0, 0], [7, 7, 7]], dtype=np.int64))
    assert s["dice"].dtype == np.float64 and s["iou"].dtype == np.float64
    assert s["dice"][0] == 2 * 3 / 10 and s["iou"][0] == 3 / 7
    assert s["dice"][1] == 0.0 and s["iou"][1] == 0.0              # nothing predicted, something there
    assert math.isnan(s["dice"][2]) and math.isnan(s["iou"][2])    # both sets empty
    assert s["dice"][3] == 1.0 and s["iou"][3] == 1.0
    t = M.group_scores(torch.tensor([[1, 2, 2]]))
    assert t["dice"].tolist() == [0.5] and t["iou"].tolist() == [1 / 3]
    with pytest.raises(ValueError):
        M.group_scores(np.zeros((3, 2)))


def test_header_declares_the_entries_and_the_package_exports_the_names():
    import mivp_amd
    from mivp_amd import _lib
    protos = _lib.parse_header()
    for name, n in (("mivp_multilabel_loss_ws", 2), ("mivp_multilabel_loss", 20), ("mivp_multilabel_loss_grad", 20),
                    ("mivp_multilabel_decode", 11), ("mivp_group_counts", 12)):
        assert name in protos and len(protos[name][1]) == n, name
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    assert "f_r    = w_r [ t_r pi_r (1 - p_r)^gamma (-log p_r) + (1 - t_r) p_r^gamma (-log(1 - p_r)) ]" in text
    for name in ("LabelGroups", "MultiLabelSpec", "MultiLabelLoss", "multilabel_loss", "decode_groups", "group_counts",
                 "group_scores", "evaluate_volume_groups"):
        assert callable(getattr(mivp_amd, name)), name
    P = mivp_amd.inference.SlidingWindowPredictor
    assert callable(P.predict_groups) and callable(P.evaluate_groups)
    assert mivp_amd.inference.evaluate_volume_groups is mivp_amd.multilabel.evaluate_volume_groups
