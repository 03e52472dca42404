"""CPU: the host side of FusedAdamW's gradient-norm clipping and non-finite step skipping.

The constructor's argument checks, the unchanged state_dict / param_groups layout, train.build_optimizer's pass-through,
tests/clip_ref.py against torch.nn.utils.clip_grad_norm_, and the header's declarations.  The kernels are tested in
tests/test_hip_grad_clip.py."""
import math
import os
import re
import sys
from argparse import Namespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as K  # noqa: E402
from conftest import ROOT  # noqa: E402
from mivp_amd import _lib, optim, train  # noqa: E402


def params():
    return [torch.nn.Parameter(torch.zeros(3, 5)), torch.nn.Parameter(torch.zeros(7))]


def test_constructor_takes_and_checks_the_options():
    opt = optim.FusedAdamW(params(), max_grad_norm=1.0, skip_nonfinite=True)       # a TypeError without the feature
    assert opt.max_grad_norm == 1.0 and opt.skip_nonfinite is True
    plain = optim.FusedAdamW(params())
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False
    assert optim.FusedAdamW(params(), max_grad_norm=2).max_grad_norm == 2.0
    for bad in (0, 0.0, -1.0, math.inf, -math.inf, math.nan, "1", True, [1.0], torch.tensor(1.0)):
        with pytest.raises(ValueError, match="max_grad_norm"):
            optim.FusedAdamW(params(), max_grad_norm=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="skip_nonfinite"):
            optim.FusedAdamW(params(), skip_nonfinite=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        plain.max_grad_norm = -3.0
    plain.max_grad_norm = 4.0                                     # nothing is recorded: assignment is allowed
    assert plain.max_grad_norm == 4.0
    with pytest.raises(RuntimeError, match="after the first step"):
        opt.grad_norm
    with pytest.raises(RuntimeError, match="after the first step"):
        opt.clip_stats()


def test_assignment_after_a_recording_raises():
    opt = optim.FusedAdamW(params(), capturable=True, max_grad_norm=1.0)
    opt._graph_params = frozenset()                               # what step() leaves behind while a stream is captured
    with pytest.raises(RuntimeError, match="record"):
        opt.max_grad_norm = 2.0
    with pytest.raises(RuntimeError, match="record"):
        opt.skip_nonfinite = True
    assert opt.max_grad_norm == 1.0 and opt.skip_nonfinite is False


def test_state_dict_and_param_groups_keep_adamw_layout():
    ps = params()
    plain = optim.FusedAdamW(ps, lr=2e-3, weight_decay=0.1)
    clip = optim.FusedAdamW(ps, lr=2e-3, weight_decay=0.1, max_grad_norm=1.0, skip_nonfinite=True)
    ref = torch.optim.AdamW(ps, lr=2e-3, weight_decay=0.1)
    for a, b in zip(plain.param_groups, clip.param_groups):
        assert list(a.keys()) == list(b.keys())
    assert "max_grad_norm" not in clip.defaults and "skip_nonfinite" not in clip.defaults
    sa, sb = plain.state_dict(), clip.state_dict()
    assert sa.keys() == sb.keys() == ref.state_dict().keys()
    assert [g.keys() for g in sa["param_groups"]] == [g.keys() for g in sb["param_groups"]]
    # a checkpoint written without the options (the layout of every earlier one) loads, and leaves the options alone
    for p in ps:
        plain.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.ones_like(p), "exp_avg_sq": torch.ones_like(p)}
    clip.load_state_dict(plain.state_dict())
    assert clip.max_grad_norm == 1.0 and clip.skip_nonfinite is True
    assert all(int(clip.state[p]["step"]) == 3 for p in ps)
    assert set(clip.state_dict()["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}


class _Core(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(4))

    def named_parameters_downstream(self):
        return list(self.named_parameters())


def test_build_optimizer_passes_the_options_through():
    conf = Namespace(training_mode="downstream", lr_downstream=1e-3, weight_decay_downstream=1e-2)
    opt = train.build_optimizer(_Core(), conf)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    conf.max_grad_norm = 12.0
    assert train.build_optimizer(_Core(), conf).max_grad_norm == 12.0
    opt = train.build_optimizer(_Core(), conf, capturable=True, max_grad_norm=3.0, skip_nonfinite=True)
    assert opt.max_grad_norm == 3.0 and opt.skip_nonfinite is True and opt.capturable is True


@pytest.mark.parametrize("max_norm", [0.5, 1e3, 1e9])
def test_clip_ref_agrees_with_torch(max_norm):
    g = K.gen(5)
    shapes = [(3, 5, 7), (1025,), (1,), (2, 1024)]
    ps = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes]
    grads = [torch.randn(s, generator=g, dtype=torch.float64) * 10.0 ** (i - 1) for i, s in enumerate(shapes)]
    for p, gr in zip(ps, grads):
        p.grad = gr.clone()
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    plan = K.plan_ref(K.sumsq64(grads), max_norm)
    assert abs(plan["norm"] - total) <= 1e-12 * total
    assert (plan["coef"] == 1.0) == (max_norm >= total + K.EPS)
    for p, gr in zip(ps, grads):
        want = gr * plan["coef"]
        assert float((p.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert K.plan_ref(K.sumsq64(grads))["coef"] == 1.0


def test_clip_ref_flags_and_counters():
    nan, inf = float("nan"), float("inf")
    assert K.plan_ref(nan, 1.0, True) == dict(sumsq=pytest.approx(nan, nan_ok=True), norm=pytest.approx(nan, nan_ok=True),
                                              coef=pytest.approx(nan, nan_ok=True), nonfinite=1, apply=0)
    assert K.plan_ref(inf, 1.0, False)["apply"] == 1 and K.plan_ref(inf, 1.0, False)["coef"] == 0.0
    assert K.plan_ref(inf, None, True)["coef"] == 1.0
    c = K.Counters()
    for sumsq in (100.0, 0.25, nan, 400.0, 0.01):                  # clipped, not, skipped, clipped, not
        c.update(K.plan_ref(sumsq, 1.0, True))
    assert (c.steps, c.clipped, c.skipped, c.max_norm_seen) == (5, 2, 1, 20.0)
    assert K.SUMSQ_REL == 13 * 2.0 ** -24 and K.NORM_REL == 8.5 * 2.0 ** -24


def test_header_declares_the_entries_and_the_kernel_states_the_same_additions():
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    at = {n: text.index(f"int {n}(") for n in ("mivp_adamw_multi_dev", "mivp_grad_sumsq_multi", "mivp_grad_clip_plan",
                                                "mivp_adamw_multi_clip", "mivp_adamw_multi_clip_dev", "mivp_store_floats")}
    assert list(at.values()) == sorted(at.values())               # after mivp_adamw_multi_dev, in this order
    assert _lib.ABI_VERSION == 18
    assert set(at) <= set(_lib.parse_header())
    src = open(os.path.join(ROOT, "medical-image-segmentation-with-visual-prompts_amd", "csrc", "proto.hip")).read()
    m = re.search(r"constexpr int SUMSQ_ADDS = (\d+) \+ (\d+) \+ (\d+);", src)
    assert m and sum(int(v) for v in m.groups()) == K.SUMSQ_ADDS
