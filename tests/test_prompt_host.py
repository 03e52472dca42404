"""CPU tests of the input-side reference (tests/input_prompt_ref.py) against torch, and of the argument checks of
``prompting.InputPrompt`` / ``PromptedModel`` / ``build_prompt_optimizer`` that need no device.

The restatement is float64 numpy; torch's own float64 ``F.conv3d`` autograd and ``F.interpolate(align_corners=True)`` (forward and
autograd) are the independent side.  Interpolation coordinates are exact rationals in the restatement and float64 products in
torch, so the two agree to a few ulp of float64, not in the bits -- except where the weights are exactly 0 or 1."""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_prompt_ref as R  # noqa: E402

F64 = torch.float64
TOL = 1e-12                                       # float64 sums of at most a few thousand O(1) terms


@pytest.mark.parametrize("B,Cin,dims,C", [(1, 1, (2, 2, 2), 8), (2, 3, (6, 10, 14), 48), (1, 4, (4, 6, 8), 16)])
def test_dgrad_restatement_is_conv3d_autograd(B, Cin, dims, C):
    g = torch.Generator().manual_seed(B + Cin + C)
    x = torch.randn((B, Cin, *dims), generator=g, dtype=F64, requires_grad=True)
    w = torch.randn((C, Cin, 2, 2, 2), generator=g, dtype=F64)
    dz = torch.randn((B, dims[0] // 2, dims[1] // 2, dims[2] // 2, C), generator=g, dtype=F64)
    y = F.conv3d(x, w, stride=2)                                       # [B, C, h, w, d]
    (y.permute(0, 2, 3, 4, 1) * dz).sum().backward()
    got = R.embed_dgrad(dz.numpy(), w.numpy())
    assert got.shape == tuple(x.shape)
    assert float(np.abs(got - x.grad.numpy()).max()) < TOL


CASES = [((2, 2, 2), (4, 6, 8), 1, 2), ((3, 4, 5), (8, 10, 12), 2, 3), ((1, 3, 2), (4, 6, 8), 2, 2), ((3, 1, 1), (5, 4, 6), 1, 1),
         ((2, 3, 1), (2, 3, 1), 1, 2)]


@pytest.mark.parametrize("lattice,roi,Cin,B", CASES)
def test_interpolation_and_transpose_are_torch_align_corners(lattice, roi, Cin, B):
    g = torch.Generator().manual_seed(sum(lattice) + sum(roi))
    P = torch.randn((Cin, *lattice), generator=g, dtype=F64, requires_grad=True)
    gout = torch.randn((B, Cin, *roi), generator=g, dtype=F64)
    up = F.interpolate(P[None], size=roi, mode="trilinear", align_corners=True)[0]
    (up[None] * gout).sum().backward()
    assert float(np.abs(R.interp(P.detach().numpy(), roi) - up.detach().numpy()).max()) < TOL
    assert float(np.abs(R.interp_t(gout.numpy(), lattice) - P.grad.numpy()).max()) < TOL
    # <T p, g> == <p, T^t g>: the two restatements are each other's transpose
    lhs = float((R.interp(P.detach().numpy(), roi)[None] * gout.numpy()).sum())
    rhs = float((P.detach().numpy() * R.interp_t(gout.numpy(), lattice)).sum())
    assert abs(lhs - rhs) < 1e-10 * max(1.0, abs(lhs))


def test_one_node_axis_is_constant_along_it():
    P = np.arange(6, dtype=np.float64).reshape(1, 1, 3, 2)
    up = R.interp(P, (4, 6, 8))
    assert np.array_equal(up, np.broadcast_to(up[:, :1], up.shape))
    assert np.array_equal(R.axis_matrix(5, 1), np.ones((5, 1)))


def test_identity_lattice_has_weights_zero_or_one():
    for n in (1, 2, 7, 96):
        M = R.axis_matrix(n, n)
        assert np.array_equal(M, np.eye(n))
    g = np.random.default_rng(0)
    P = g.standard_normal((2, 3, 4, 5))
    x = g.standard_normal((3, 2, 3, 4, 5))
    assert np.array_equal(R.interp(P, (3, 4, 5)), P)
    assert np.array_equal(R.prompt_fwd(x, P, 1.0), x + P[None])
    assert np.array_equal(R.interp_t(x, (3, 4, 5)), (x[0] + x[1]) + x[2])
    g32 = x.astype(np.float32)
    assert np.array_equal(R.identity_bwd_f32(g32, 1.0), (g32[0] + g32[1]) + g32[2])


def test_axis_rows_sum_to_one_and_nodes_sit_on_the_corners():
    for n, g in ((8, 3), (96, 8), (12, 5), (6, 6), (9, 2)):
        M = R.axis_matrix(n, g)
        assert np.allclose(M.sum(1), 1.0, atol=1e-15) and (M >= 0).all()
        assert M[0, 0] == 1.0 and M[n - 1, g - 1] == 1.0
        assert ((M > 0).sum(1) <= 2).all()


# ---------------------------------------------------------------------------------------------
# argument checks (no device)
# ---------------------------------------------------------------------------------------------
def test_input_prompt_construction_and_checks():
    import mivp_amd  # noqa: F401
    from mivp_amd.prompting import InputPrompt
    p = InputPrompt(2, (8, 10, 12), lattice=(3, 4, 5), scale=0.5)
    assert tuple(p.P.shape) == (2, 3, 4, 5) and p.P.dtype == torch.float32 and p.P.requires_grad
    assert not bool(p.P.detach().any())                               # the identity to start from
    assert p.scale.dtype == torch.float32 and float(p.scale) == 0.5
    assert [n for n, _ in p.named_parameters()] == ["P"]
    full = InputPrompt(1, (4, 6, 8))
    assert full.lattice == full.roi == (4, 6, 8) and tuple(full.P.shape) == (1, 4, 6, 8)
    assert InputPrompt(1, (4, 6, 8), lattice=(1, 6, 1)).lattice == (1, 6, 1)
    p.set_scale(0.25)
    assert float(p.scale) == 0.25
    for bad in (dict(channels=0), dict(channels=True), dict(channels=1.0), dict(roi=(8, 8)), dict(roi=(8, 0, 8)), dict(roi="888"),
                dict(roi=(8, 8, 8.0)), dict(lattice=(9, 8, 8)), dict(lattice=(0, 2, 2)), dict(lattice=(2, 2)), dict(lattice=5),
                dict(scale=float("nan")), dict(scale="1"), dict(scale=True), dict(roi=(4000, 90, 8))):
        kw = dict(channels=1, roi=(8, 8, 8), lattice=(2, 2, 2), scale=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            InputPrompt(**kw)
    with pytest.raises(ValueError):
        p.set_scale(float("inf"))
    for x in (torch.zeros(2, 8, 10, 12), torch.zeros(1, 1, 8, 10, 12), torch.zeros(1, 2, 8, 10, 14),
              torch.zeros(1, 2, 8, 10, 12, dtype=torch.float64), torch.zeros(0, 2, 8, 10, 12), "x"):
        with pytest.raises(ValueError):
            p(x)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        p(torch.zeros(1, 2, 8, 10, 12))                                # no CPU fallback


def test_prompted_model_surface_and_checks():
    import mivp_amd  # noqa: F401
    from mivp_amd import prompting as PR

    class Toy(torch.nn.Module):
        def __init__(self, cin):
            super().__init__()
            self.conf = Namespace(input_channels=cin, training_mode="downstream", lr_prompt_tokens=5e-4, lr_downstream=1e-3,
                                  weight_decay_downstream=0.0)
            self.head = torch.nn.Linear(2, 2)

        def named_parameters_downstream(self):
            return list(self.head.named_parameters())

        def forward(self, x):
            return {"downstream": x}

    prompt = PR.InputPrompt(1, (4, 4, 4), lattice=(2, 2, 2))
    toy = Toy(1)
    w = PR.PromptedModel(toy, prompt)
    assert w.conf is toy.conf
    assert [n for n, _ in w.named_parameters_input_prompt()] == ["prompt.P"] and w.named_parameters_input_prompt()[0][1] is prompt.P
    assert [n for n, _ in w.named_parameters_downstream()] == ["weight", "bias"]          # forwarded to the model
    assert "prompt.P" in dict(w.named_parameters()) and "model.head.weight" in dict(w.named_parameters())
    with pytest.raises(AttributeError):
        w.named_parameters_nonexistent
    with pytest.raises(AttributeError):
        w.something_else
    for model, pr in ((toy, "prompt"), ("model", prompt), (Toy(2), prompt), (w, prompt)):
        with pytest.raises(ValueError):
            PR.PromptedModel(model, pr)
    with pytest.raises(ValueError):
        PR.build_prompt_optimizer(toy, toy.conf)
    for kw in (dict(lr=-1.0), dict(weight_decay=float("nan")), dict(include_downstream=1), dict(capturable="yes")):
        with pytest.raises(ValueError):
            PR.build_prompt_optimizer(w, toy.conf, **kw)
    other = Namespace(**{**vars(toy.conf), "training_mode": "supervised_learning_all"})
    with pytest.raises(ValueError, match="downstream"):
        PR.build_prompt_optimizer(w, other, include_downstream=True)
    for fn in (PR.input_gradient, PR.saliency_map):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            fn(toy, torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4), toy.conf)
    with pytest.raises(ValueError):
        PR.fgsm(toy, torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4), toy.conf, -0.1)


def test_the_new_entries_are_declared_and_the_abi_version_stands():
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib
    protos = _lib.parse_header()
    assert len(protos["mivp_patch_embed_dgrad"][1]) == 5
    assert len(protos["mivp_input_prompt_fwd"][1]) == 13 and len(protos["mivp_input_prompt_bwd"][1]) == 12
    assert _lib.ABI_VERSION == 18
