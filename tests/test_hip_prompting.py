"""GPU tests of the input volume's gradient and the pixel-space prompt at the autograd and model level.

  functional.patch_embed with x.requires_grad (training- and eval-mode BatchNorm): dx against float64 autograd of BN(conv(x)) under
      the E32 rule of tests/input_prompt_ref.py (every element within 8 E32).  The float32 eager torch composition that defines
      E32 stores what the kernels store in bf16 -- the recomputed conv output z and the BatchNorm backward's dz, as dy itself
      arrives in bf16 -- and is float32 everywhere else (the project's err32 restatements round at the storage points in the
      same way, tests/merge_ref.py).  Parameter gradients: the same bits as a call with x.requires_grad == False; launch lists.
  whole model: dL/dx against OracleSwinUnetR (CPU, x.requires_grad_) on the 16^3 toy fixtures, one configuration without
      res blocks and one whose raw-input skip adds a torch-autograd contribution, under the rule of
      test_hip_model._check_all_gradients restated here: rel-L2 error <= max(5e-2, 5 x yardstick), the yardstick being the larger
      of the oracle's and the kernels' own change of that gradient under 2^-9 relative input noise; cosine > 0.9 where the
      yardstick is below 0.2; finite and non-zero.
  PromptedModel (downstream mode, backbone not stepped): an eager train_step moves P and no other parameter; P.grad against the
      oracle's dL/dx' composed with the float64 T^t under the same rule; a GraphedStep recorded once and replayed on new x, y
      and a new set_scale value equals the eager step in the bits.
  saliency_map / fgsm: shapes, dtypes, eps = 0, and the loss after a small step."""
import copy
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_prompt_ref as R  # noqa: E402
from conftest import load_fixture, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def r16(t):
    return t.to(BF16).to(F32)


def round_weights(sd):
    """As tests/test_hip_model.py: GEMM / conv operands rounded to bf16 on both sides, so the comparison isolates arithmetic."""
    out = {}
    for k, v in sd.items():
        if v.is_floating_point() and v.dim() >= 2 and not k.startswith("prompt_tokens") and ".pe." not in k \
                and not k.startswith("input_layer.0"):
            out[k] = r16(v)
        else:
            out[k] = v.clone()
    return out


def toy(tag):
    fx = load_fixture(f"unetr_{tag}")
    conf = Namespace(**fx.meta["conf"])
    conf.include_background = True
    conf.lr_downstream, conf.weight_decay_downstream, conf.lr_prompt_tokens = 1e-3, 0.0, 5e-3
    return fx, conf, round_weights(fx["sd"])


def product_model(conf, sd):
    from mivp_amd.swin_unetr import SwinUnetR
    model = SwinUnetR(conf)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train()


def labels(shape, seed=3):
    return torch.randint(0, 2, (shape[0], 1, *shape[2:]), generator=torch.Generator().manual_seed(seed)).float()


def check_gradient(name, g, w, yard):
    """The rule of test_hip_model._check_all_gradients for one tensor; g the kernels' gradient, w the oracle's."""
    g, w = g.detach().cpu().to(F32), w.detach().cpu().to(F32)
    assert bool(torch.isfinite(g).all()), name
    assert float(g.norm()) > 0 and float(w.norm()) > 1e-6, (name, float(g.norm()), float(w.norm()))
    cos = float(F.cosine_similarity(g.reshape(-1), w.reshape(-1), dim=0))
    e = rel_l2(g, w)
    print(f"[input grad] {name}: rel-L2 error {e:.3e}, cosine {cos:.4f}, yardstick {yard:.3e}, bar {max(5e-2, 5.0 * yard):.3e}")
    assert not (yard < 0.2 and cos < 0.9), (name, e, cos, yard)
    assert e <= max(5e-2, 5.0 * yard), (name, e, cos, yard)


class LaunchLog:
    """Names of the C-ABI entries called while active (ops and prompting look ``_lib.call`` up at every call)."""

    def __enter__(self):
        from mivp_amd import _lib
        self._lib, self._call, self.names = _lib, _lib.call, []

        def call(name, *args):
            self.names.append(name)
            return self._call(name, *args)

        _lib.call = call
        return self

    def __exit__(self, *exc):
        self._lib.call = self._call


# =============================================================================================
# functional.patch_embed
# =============================================================================================
def embed_modules(Cin, Cc, seed, frozen):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv3d(Cin, Cc, 2, 2)
    bn = torch.nn.BatchNorm3d(Cc)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.4)
        conv.bias.copy_(torch.randn(Cc, generator=g) * 0.1)
        bn.weight.copy_(1.0 + 0.2 * torch.randn(Cc, generator=g))
        bn.bias.copy_(0.1 * torch.randn(Cc, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(Cc, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(Cc, generator=g))
    if frozen:
        for p in list(conv.parameters()) + list(bn.parameters()):
            p.requires_grad_(False)
    return conv, bn


def embed_references(x, conv, bn, gout, training):
    """(float64 autograd dx, the float32 composition with bf16 storage of z and dz); gout [B,h,w,d,C]."""
    w, b, ga, be = (t.detach().cpu() for t in (conv.weight, conv.bias, bn.weight, bn.bias))
    rm, rv = bn.running_mean.detach().cpu(), bn.running_var.detach().cpu()
    x64 = x.to(F64).requires_grad_(True)
    y = F.batch_norm(F.conv3d(x64, w.to(F64), b.to(F64), stride=2), rm.to(F64).clone(), rv.to(F64).clone(), ga.to(F64), be.to(F64),
                     training, 0.1, bn.eps)
    (y.permute(0, 2, 3, 4, 1) * gout.to(F64)).sum().backward()
    z = F.conv3d(x, w, b, stride=2)                                        # float32 from here on
    red, shp = (0, 2, 3, 4), (1, -1, 1, 1, 1)
    if training:
        mean, var = z.mean(red), z.var(red, unbiased=False)
    else:
        mean, var = rm, rv
    rstd = torch.rsqrt(var + bn.eps)
    zb = r16(z)                                                            # the recomputed conv output as stored
    gz = gout.permute(0, 4, 1, 2, 3).to(F32)
    xhat = (zb - mean.view(shp)) * rstd.view(shp)
    if training:
        n = z.numel() // z.shape[1]
        dz = (ga * rstd).view(shp) * (gz - gz.sum(red).view(shp) / n - xhat * (gz * xhat).sum(red).view(shp) / n)
    else:
        dz = (ga * rstd).view(shp) * gz
    dx32 = F.conv_transpose3d(r16(dz), w, stride=2)                        # dz as stored
    return x64.grad, dx32


EMBED = [(1, 48, (8, 12, 10), 2), (2, 16, (6, 4, 10), 3)]


@pytest.mark.parametrize("training", [True, False], ids=["train_bn", "eval_bn"])
@pytest.mark.parametrize("frozen", [False, True], ids=["trainable", "frozen"])
@pytest.mark.parametrize("Cin,Cc,dims,B", EMBED, ids=[f"Cin{c[0]}_C{c[1]}_{'x'.join(map(str, c[2]))}_B{c[3]}" for c in EMBED])
def test_patch_embed_input_gradient(Cin, Cc, dims, B, frozen, training):
    import mivp_amd  # noqa: F401
    from mivp_amd import functional as Fn
    g = torch.Generator().manual_seed(Cin + Cc + B)
    x = torch.rand((B, Cin, *dims), generator=g)
    gout = r16(torch.randn((B, dims[0] // 2, dims[1] // 2, dims[2] // 2, Cc), generator=g))

    def run(x_grad):
        conv, bn = embed_modules(Cin, Cc, 11, frozen)
        conv, bn = conv.to(DEV), bn.to(DEV)
        bn.train(training)
        xd = x.to(DEV).requires_grad_(x_grad)
        with LaunchLog() as log:
            y = Fn.patch_embed(None, conv, bn, xd)
            Fn.flush_counters()
            if y.requires_grad:
                (y.float() * gout.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return conv, bn, xd, y, log.names

    conv, bn, xd, y, names = run(True)
    assert y.dtype == BF16 and xd.grad is not None and xd.grad.dtype == F32 and xd.grad.shape == xd.shape
    ref_conv, ref_bn = embed_modules(Cin, Cc, 11, frozen)
    ref_bn.train(training)
    dx64, dx32 = embed_references(x, ref_conv, ref_bn, gout, training)
    what = f"patch_embed dx Cin={Cin} C={Cc} dims={dims} B={B} frozen={frozen} training={training}"
    R.check_err32(xd.grad.cpu().numpy(), dx64.numpy(), dx32.numpy(), what, "bchwd")
    # launches: one dgrad; a frozen encoder skips the im2col, the TN GEMM and the column sum
    assert names.count("mivp_patch_embed_dgrad") == 1
    assert ("mivp_patch_im2col" in names) == (not frozen) and ("mivp_gemm_tn" in names) == (not frozen)
    # the path without an input gradient: the same parameter bits, the launches it always had
    conv0, bn0, x0, y0, names0 = run(False)
    assert torch.equal(y0, y) and x0.grad is None
    assert "mivp_patch_embed_dgrad" not in names0
    if frozen:
        assert not y0.requires_grad and all(p.grad is None for p in list(conv.parameters()) + list(bn.parameters()))
        assert names0 == [n for n in names0 if n in ("mivp_patch_embed", "mivp_bn_finalize")]       # forward only
    else:
        assert [n for n in names if n != "mivp_patch_embed_dgrad"] == names0                         # one launch added, none moved
        for (k, p), (_, q) in zip(list(conv.named_parameters()) + list(bn.named_parameters()),
                                  list(conv0.named_parameters()) + list(bn0.named_parameters())):
            assert p.grad is not None and torch.equal(p.grad, q.grad), f"{what}: {k}.grad changed its bits with x.requires_grad"
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        assert torch.equal(getattr(bn, k), getattr(bn0, k)), k


# =============================================================================================
# whole model
# =============================================================================================
@pytest.mark.parametrize("tag", ["downstream_e1d1", "downstream_e1d1_simple"])
def test_model_input_gradient_against_the_oracle(tag):
    import mivp_amd  # noqa: F401
    from oracle.unetr_ref import OracleSwinUnetR
    fx, conf, sd = toy(tag)
    assert conf.unetr_res_block == ("simple" if tag.endswith("simple") else "none")
    x, gout = fx["in"]["x"], fx["in"]["gout"]
    xp = x * (1 + 2.0 ** -9 * torch.randn(x.shape, generator=torch.Generator().manual_seed(1)))

    def oracle(xx):
        xg = xx.clone().requires_grad_(True)
        want, _ = OracleSwinUnetR(conf, {k: v.clone() for k, v in sd.items()})(xg, training=True)
        (want["downstream"] * gout).sum().backward()
        return xg.grad

    def product(xx):
        model = product_model(conf, sd)
        xg = xx.to(DEV).requires_grad_(True)
        with LaunchLog() as log:
            (model(xg)["downstream"] * gout.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert log.names.count("mivp_patch_embed_dgrad") == 1
        return xg.grad.cpu()

    w, wp, g, gp = oracle(x), oracle(xp), product(x), product(xp)
    assert g.shape == x.shape and g.dtype == F32
    check_gradient(f"{tag} dL/dx", g, w, max(rel_l2(wp, w), rel_l2(gp, g)))
    # the default path (x without a gradient) launches neither new kernel
    model = product_model(conf, sd)
    with LaunchLog() as log:
        (model(x.to(DEV))["downstream"] * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert not [n for n in log.names if n in ("mivp_patch_embed_dgrad", "mivp_input_prompt_fwd", "mivp_input_prompt_bwd")]


# =============================================================================================
# PromptedModel
# =============================================================================================
LATTICE, SCALE = (4, 4, 4), 0.5


def prompted(conf, sd, P0):
    from mivp_amd import prompting as PR
    prompt = PR.InputPrompt(conf.input_channels, (16, 16, 16), lattice=LATTICE, scale=SCALE)
    with torch.no_grad():
        prompt.P.copy_(P0)
    return PR.PromptedModel(product_model(conf, sd), prompt.to(DEV))


def test_prompted_model_step_and_prompt_gradient_against_the_oracle():
    import mivp_amd  # noqa: F401
    from mivp_amd import prompting as PR, train
    from oracle.unetr_ref import OracleSwinUnetR
    fx, conf, sd = toy("downstream_e1d1")
    x = fx["in"]["x"]
    y = labels(x.shape)
    P0 = 0.05 * torch.randn((1, *LATTICE), generator=torch.Generator().manual_seed(2))
    xp = x * (1 + 2.0 ** -9 * torch.randn(x.shape, generator=torch.Generator().manual_seed(1)))

    def oracle(xx):
        xin = torch.from_numpy(R.prompt_fwd(xx.numpy(), P0.numpy(), SCALE)).to(F32).requires_grad_(True)
        out, _ = OracleSwinUnetR(conf, {k: v.clone() for k, v in sd.items()})(xin, training=True)
        train.dice_focal_loss(out["downstream"], y, True, 4.0).backward()
        return torch.from_numpy(R.prompt_bwd(xin.grad.numpy(), LATTICE, SCALE))

    def product(xx):
        wrapper = prompted(conf, sd, P0)
        opt = PR.build_prompt_optimizer(wrapper, conf, lr=1e-2)
        before = {k: v.detach().clone() for k, v in wrapper.model.named_parameters()}
        with LaunchLog() as log:
            loss = train.train_step(wrapper, opt, conf, xx.to(DEV), y.to(DEV))
        torch.cuda.synchronize()
        return wrapper, before, loss, log.names

    wrapper, before, loss, names = product(x)
    assert bool(torch.isfinite(loss)) and names.count("mivp_input_prompt_fwd") == 1 and names.count("mivp_input_prompt_bwd") == 1
    assert names.count("mivp_patch_embed_dgrad") == 1
    assert [k for k, _ in wrapper.named_parameters_input_prompt()] == ["prompt.P"]
    assert not torch.equal(wrapper.prompt.P.detach().cpu(), P0), "the step did not move P"
    changed = [k for k, v in wrapper.model.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert changed == [], f"parameters outside the optimizer changed their bits: {changed[:4]}"
    g = wrapper.prompt.P.grad
    assert g is not None and g.shape == (1, *LATTICE) and g.dtype == F32
    wrapper_p, _, _, _ = product(xp)
    w, wp = oracle(x), oracle(xp)
    check_gradient("P.grad", g, w, max(rel_l2(wp, w), rel_l2(wrapper_p.prompt.P.grad, g)))


def test_graphed_prompt_step_equals_the_eager_step():
    """Two eager warm-up steps + one replay on a new batch and a new scale against three eager steps: the same bits."""
    import mivp_amd  # noqa: F401
    from mivp_amd import prompting as PR, train
    fx, conf, sd = toy("downstream_e1d1")
    x0 = fx["in"]["x"]
    y0 = labels(x0.shape)
    x1 = torch.rand(x0.shape, generator=torch.Generator().manual_seed(8))
    y1 = labels(x0.shape, seed=9)
    P0 = 0.05 * torch.randn((1, *LATTICE), generator=torch.Generator().manual_seed(2))
    ref = prompted(conf, sd, P0)
    own = copy.deepcopy(ref)
    o_ref = PR.build_prompt_optimizer(ref, conf, lr=1e-2, include_downstream=True)
    o_own = PR.build_prompt_optimizer(own, conf, lr=1e-2, include_downstream=True, capturable=True)
    assert len(o_ref.param_groups) == 2 and o_ref.param_groups[0]["params"][0] is ref.prompt.P
    x, y = x0.to(DEV).clone(), y0.to(DEV).clone()
    for _ in range(2):
        train.train_step(ref, o_ref, conf, x, y)
    ref.prompt.set_scale(0.25)
    l_ref = float(train.train_step(ref, o_ref, conf, x1.to(DEV), y1.to(DEV)))
    step = train.graphed_train_step(own, o_own, conf, x, y, warmup=2)
    x.copy_(x1.to(DEV)); y.copy_(y1.to(DEV))
    own.prompt.set_scale(0.25)
    l_own = float(step())
    torch.cuda.synchronize()
    print(f"[graph prompt] eager loss {l_ref!r}, replayed {l_own!r}")
    assert l_own == l_ref
    assert torch.equal(own.prompt.P.detach(), ref.prompt.P.detach())
    a, b = dict(ref.state_dict()), dict(own.state_dict())
    assert [k for k in a if not torch.equal(a[k], b[k])] == []


# =============================================================================================
# saliency_map / fgsm
# =============================================================================================
def test_saliency_and_fgsm():
    import mivp_amd  # noqa: F401
    from mivp_amd import prompting as PR, train
    from oracle.unetr_ref import OracleSwinUnetR
    fx, conf, sd = toy("downstream_e1d1_simple")
    x, y = fx["in"]["x"].to(DEV), labels(fx["in"]["x"].shape).to(DEV)
    model = product_model(conf, sd)
    g = PR.input_gradient(model, x, y, conf)
    assert g.shape == x.shape and g.dtype == F32 and g.is_cuda and not g.requires_grad
    assert all(p.grad is None for p in model.parameters()) and not x.requires_grad
    sal = PR.saliency_map(model, x, y, conf)
    assert sal.shape == (x.shape[0], *x.shape[2:]) and sal.dtype == F32 and sal.is_cuda
    assert bool((sal >= 0).all()) and float(sal.max()) > 0 and bool(torch.isfinite(sal).all())
    same = PR.fgsm(model, x, y, conf, 0.0)
    assert same.data_ptr() != x.data_ptr() and torch.equal(same.view(torch.int32), x.view(torch.int32))
    eps = 1e-2
    adv = PR.fgsm(model, x, y, conf, eps)
    assert adv.shape == x.shape and adv.dtype == x.dtype and float((adv - x).abs().max()) <= eps + 2.0 ** -22   # |x| < 2: two float32 roundings

    def oracle_loss(xx):
        sd64 = {k: (v.to(F64) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        out, _ = OracleSwinUnetR(conf, sd64)(xx, training=True)
        return train.dice_focal_loss(out["downstream"], y.cpu().to(F64), True, 4.0)

    x64 = x.cpu().to(F64).requires_grad_(True)
    l0 = oracle_loss(x64)
    l0.backward()
    rise = float(oracle_loss((x64 + eps * x64.grad.sign()).detach())) - float(l0)
    with torch.no_grad():
        before = float(train.step_loss(model(x), conf, y))
        after = float(train.step_loss(model(adv), conf, y))
    print(f"[fgsm] eps {eps}: loss {before!r} -> {after!r}; the float64 oracle's own step changes its loss by {rise:.3e}")
    if rise <= 0:
        print("[fgsm] the oracle's float64 step does not raise the loss on this fixture: the loss comparison is not asserted")
    else:
        assert after >= before, (before, after, rise)
