"""GPU: the phase-1 multi-view step (csrc/multiview.hip through mivp_amd.multiview).

Views are compared bit for bit with torch.rot90 + mask; the reconstruction / mutual terms and the heads with fp32 torch
autograd (and the reference's ContrastivePairLoss fixtures); the whole step with the reference's MultiViewTrainer run for
one step (tests/golden/gen_golden_multiview.py), under the bars of the existing model tests: loss components within
2.5e-2 (16^3 toy volumes) or 1.25x the distance between two HIP runs whose inputs differ by 2^-9 relative noise, and
every trainable gradient pointing the same way (cosine > 0.9 where it is stable) and within max(5e-2, 5 x yardstick)
rel-L2, the yardstick being the HIP path's own gradient movement under that input noise (the rule of
test_hip_model._check_all_gradients, restated here)."""
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_fixture, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
PERMS = {0: (0, 1, 3, 2, 4), 1: (0, 1, 4, 3, 2), 2: (0, 1, 2, 4, 3)}


def _mv():
    import mivp_amd  # noqa: F401
    from mivp_amd import multiview
    return multiview


def views_torch(x, rot, keep):
    out = torch.stack([torch.rot90(x[b], int(rot[b]), (1, 2)) for b in range(x.shape[0])])
    return out * keep.to(out.device, out.dtype)


def con_loss_torch(z_i, z_j, temp=0.5):
    bs = z_i.shape[0]
    z = torch.cat([F.normalize(z_i, dim=1), F.normalize(z_j, dim=1)])
    sim = F.cosine_similarity(z.unsqueeze(1), z.unsqueeze(0), dim=2)
    pos = torch.exp(torch.cat([torch.diag(sim, bs), torch.diag(sim, -bs)]) / temp)
    neg = (~torch.eye(2 * bs, dtype=torch.bool, device=z.device)).to(z.dtype) * torch.exp(sim / temp)
    return torch.sum(-torch.log(pos / torch.sum(neg, dim=1))) / (2 * bs)


def _draws(mv, B, dims, mshape, ratio, rot_i, rot_j, perm, seed=0):
    d = mv.draw_views(np.random.RandomState(seed), B, dims, mshape, ratio, perm is not None)
    d.rot_i, d.rot_j = np.asarray(rot_i, dtype=np.int64), np.asarray(rot_j, dtype=np.int64)
    d.perm = perm
    return d


def _conf(**kw):
    c = dict(use_reconstruction=False, use_rotation_prediction=False, use_contrastive_learning=False,
             use_mutual_learning=False, weight_rec=0.2, weight_rot=0.5, weight_con=0.3)
    c.update(kw)
    return Namespace(**c)


# ------------------------------------------------------------------------------------------------ 1. views
@pytest.mark.parametrize("B,C,dims,mutual", [(4, 1, (96, 96, 96), True), (2, 1, (128, 128, 8), False),
                                             (4, 4, (32, 32, 32), True), (4, 1, (20, 20, 6), False)])
def test_views_bit_exact(B, C, dims, mutual):
    mv = _mv()
    x = torch.rand(B, C, *dims, generator=torch.Generator().manual_seed(1)).to(DEV)
    rot_i, rot_j = [k % 4 for k in range(B)], [(3 - k) % 4 for k in range(B)]       # all four codes in each view
    for perm in ((0, 1, 2) if mutual else (None,)):
        d = _draws(mv, B, dims, (2, 2, 2), 0.2, rot_i, rot_j, perm, seed=B + C)
        slot = mv.ViewSlot(B, dims, (2, 2, 2), 0.2, mutual, DEV)
        slot.load(d)
        xi, xj, xk = mv.make_views(x, slot)
        torch.cuda.synchronize()
        ki, kj = d.keep_voxels("i"), d.keep_voxels("j")
        wi, wj = views_torch(x, rot_i, ki), views_torch(x, rot_j, kj)
        assert torch.equal(xi, wi) and torch.equal(xj, wj)
        assert not xi.requires_grad
        if mutual:
            assert torch.equal(xk, wi.permute(*PERMS[perm]).contiguous()), perm
        else:
            assert xk is None


# ------------------------------------------------------------------------------------------------ 2. rec / mut
@pytest.mark.parametrize("perm", [0, 1, 2])
def test_reconstruction_and_mutual_terms(perm):
    mv = _mv()
    B, dims, ratio = 4, (96, 96, 96), 0.2
    g = torch.Generator().manual_seed(perm)
    x = torch.rand(B, 1, *dims, generator=g).to(DEV)
    d = _draws(mv, B, dims, (2, 2, 2), ratio, [0, 1, 2, 3], [3, 2, 1, 0], perm, seed=perm)
    slot = mv.ViewSlot(B, dims, (2, 2, 2), ratio, True, DEV)
    slot.load(d)
    xi, xj, _ = mv.make_views(x, slot)
    recs = [torch.randn(B, 1, *dims, generator=g).to(DEV).requires_grad_(True) for _ in range(3)]
    conf = _conf(use_reconstruction=True, use_mutual_learning=True)

    def hip():
        for r in recs:
            r.grad = None
        total, vec = mv.multiview_loss({"reconstruction": recs[0]}, {"reconstruction": recs[1]},
                                       {"reconstruction": recs[2]}, slot, conf, xi, xj)
        total.backward()
        torch.cuda.synchronize()
        return vec.clone(), [r.grad.clone() for r in recs]

    vec, grads = hip()
    vec2, grads2 = hip()
    assert torch.equal(vec, vec2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    ki, kj = d.keep_voxels("i").to(DEV).float(), d.keep_voxels("j").to(DEV).float()
    for r in recs:
        r.grad = None
    rec = F.mse_loss(torch.cat([recs[0] * ki, recs[1] * kj]), torch.cat([xi * ki, xj * kj])) / (1 - ratio)
    mut = F.mse_loss(recs[2].permute(*PERMS[perm]).contiguous() * ki, recs[0] * ki) / (1 - ratio)
    (0.2 * rec + mut).backward()
    assert abs(float(vec[0]) - float(rec)) <= 1e-6 * float(rec)
    assert abs(float(vec[3]) - float(mut)) <= 1e-6 * float(mut)
    assert abs(float(vec[4]) - float(0.2 * rec + mut)) <= 1e-6 * float(0.2 * rec + mut)
    assert float(vec[1]) == 0.0 and float(vec[2]) == 0.0
    for a, r in zip(grads, recs):
        assert rel_l2(a, r.grad) < 1e-6


# ------------------------------------------------------------------------------------------------ 3. heads
@pytest.mark.parametrize("tag", ["a", "b"])
def test_contrastive_pair_loss_matches_reference(tag):
    mv = _mv()
    fx = load_fixture(f"mv_contrastive_{tag}")
    zi = fx["in"]["z_i"].to(DEV).requires_grad_(True)
    zj = fx["in"]["z_j"].to(DEV).requires_grad_(True)
    m = mv.ContrastivePairLoss(fx.meta["bs"]).to(DEV)
    assert set(dict(m.named_buffers())) == {"temp", "neg_mask"}
    loss = m(zi, zj)
    loss.backward()
    torch.cuda.synchronize()
    want = float(fx["out"]["loss"])
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert rel_l2(zi.grad, fx["grad"]["z_i"]) < 1e-5
    assert rel_l2(zj.grad, fx["grad"]["z_j"]) < 1e-5


@pytest.mark.parametrize("B", [2, 14])
def test_heads_match_torch_autograd(B):
    mv = _mv()
    dims = (8, 8, 8)
    g = torch.Generator().manual_seed(B)
    d = _draws(mv, B, dims, (2, 2, 2), 0.2, [k % 4 for k in range(B)], [(k + 1) % 4 for k in range(B)], None)
    slot = mv.ViewSlot(B, dims, (2, 2, 2), 0.2, False, DEV)
    slot.load(d)
    leaves = [torch.randn(B, 4, generator=g), torch.randn(B, 4, generator=g), torch.randn(B, 512, generator=g),
              torch.randn(B, 512, generator=g)]
    leaves = [t.to(DEV).requires_grad_(True) for t in leaves]
    conf = _conf(use_rotation_prediction=True, use_contrastive_learning=True)
    total, vec = mv.multiview_loss({"rotation_prediction": leaves[0], "contrastive_coding": leaves[2]},
                                   {"rotation_prediction": leaves[1], "contrastive_coding": leaves[3]}, None, slot, conf,
                                   None, None)
    total.backward()
    torch.cuda.synchronize()
    got = [t.grad.clone() for t in leaves]
    for t in leaves:
        t.grad = None
    tgt = torch.tensor(np.concatenate([d.rot_i, d.rot_j]), device=DEV)
    rot = F.cross_entropy(torch.cat([leaves[0], leaves[1]]), tgt)
    con = con_loss_torch(leaves[2], leaves[3])
    (0.5 * rot + 0.3 * con).backward()
    assert abs(float(vec[1]) - float(rot)) <= 1e-5 * float(rot)
    assert abs(float(vec[2]) - float(con)) <= 1e-5 * float(con)
    assert abs(float(vec[4]) - float(0.5 * rot + 0.3 * con)) <= 1e-5 * float(0.5 * rot + 0.3 * con)
    for a, t in zip(got, leaves):
        assert rel_l2(a, t.grad) < 1e-5


def test_heads_limits_raise():
    mv = _mv()
    with pytest.raises(ValueError):
        mv.ContrastivePairLoss(33)(torch.randn(33, 8, device=DEV), torch.randn(33, 8, device=DEV))
    with pytest.raises(ValueError):
        mv.ContrastivePairLoss(2)(torch.randn(2, 1025, device=DEV), torch.randn(2, 1025, device=DEV))


# ------------------------------------------------------------------------------------------------ 4. full step
def _fixture_draws(mv, fx, conf):
    d, m = fx["draws"], tuple(conf.masking_shape)
    ki = d["keep_i"].bool().numpy()[::m[0], ::m[1], ::m[2]]
    kj = d["keep_j"].bool().numpy()[::m[0], ::m[1], ::m[2]]
    return mv.ViewDraws(d["rot_i"].numpy().astype(np.int64), d["rot_j"].numpy().astype(np.int64), ki.copy(), kj.copy(),
                        fx.meta["perm"] if conf.use_mutual_learning else None, tuple(conf.roi_size), m,
                        float(conf.masking_ratio))


def _hip_step(mv, conf, sd, x, draws):
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    model = SwinUnetR(conf)
    model.load_state_dict(sd, strict=True)
    model.to(DEV).train()
    opt = train.build_optimizer(model, conf)
    slot = mv.make_slot(conf, x.to(DEV))
    slot.load(draws)
    vec = mv.multiview_forward_backward(model, opt, conf, x.to(DEV).contiguous(), slot)
    torch.cuda.synchronize()
    return model, vec.cpu()


@pytest.mark.parametrize("tag", ["rrc", "mut"])
def test_full_step_matches_reference_trainer(tag):
    mv = _mv()
    fx = load_fixture(f"mv_step_{tag}")
    conf = Namespace(**fx.meta["conf"])
    sd = dict(fx["sd"])
    x = fx["in"]["x"]
    draws = _fixture_draws(mv, fx, conf)
    # the fixture's draws are the reference's own (its keep maps at patch resolution reproduce the voxel maps)
    assert torch.equal(draws.keep_voxels("i"), fx["draws"]["keep_i"].bool())
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(1))
    model, vec = _hip_step(mv, conf, sd, x, draws)
    model_p, vec_p = _hip_step(mv, conf, sd, x * (1 + 2.0 ** -9 * noise), draws)
    names = ["rec", "rot", "con", "mut", "tot"]
    for i, k in enumerate(names):
        if k not in fx["loss"]:
            assert float(vec[i]) == 0.0, k
            continue
        want = float(fx["loss"][k])
        self_noise = abs(float(vec_p[i]) - float(vec[i])) / abs(want)
        assert abs(float(vec[i]) - want) / abs(want) < max(2.5e-2, 1.25 * self_noise), (k, float(vec[i]), want)
    params, params_p = dict(model.named_parameters()), dict(model_p.named_parameters())
    bad = {}
    for k in fx.meta["trainable"]:
        w = fx["grad"][k]
        g = params[k].grad
        assert g is not None, k
        assert torch.isfinite(g).all(), k
        sib = fx["grad"].get(k.replace(".bias", ".weight")) if k.endswith(".bias") else None
        scale = float(sib.norm()) if sib is not None else 1.0
        if float(w.norm()) < 1e-6 or (sib is not None and float(w.norm()) < 1e-4 * scale):
            assert float(g.norm()) < 2e-2 * max(scale, 1e-3), (k, float(g.norm()), scale)
            continue
        g = g.cpu()
        cos = float(F.cosine_similarity(g.reshape(-1), w.reshape(-1), dim=0))
        yard = rel_l2(params_p[k].grad.cpu(), g)
        e = rel_l2(g, w)
        if (yard < 0.2 and cos < 0.9) or e > max(5e-2, 5.0 * yard):
            bad[k] = (e, cos, yard)
    assert not bad, bad
    # the patch-embed BatchNorm ran once per forward (two or three), as the reference's
    msd = model.state_dict()
    for k, v in fx["after"].items():
        if v.is_floating_point():
            assert rel_l2(msd[k].cpu(), v) < 2e-2, k
        else:
            assert int(msd[k]) == int(v), k


# ------------------------------------------------------------------------------------------------ 5. graphed step
def test_graphed_step_equals_eager_steps():
    mv = _mv()
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    fx = load_fixture("mv_step_rrc")
    conf = Namespace(**fx.meta["conf"])
    x = fx["in"]["x"].to(DEV).contiguous()
    seq = [mv.draw_views(np.random.RandomState(100 + s), 2, conf.roi_size, conf.masking_shape, conf.masking_ratio, False)
           for s in range(6)]

    def fresh():
        m = SwinUnetR(conf)
        m.load_state_dict(dict(fx["sd"]), strict=True)
        m.to(DEV).train()
        o = train.build_optimizer(m, conf, capturable=True)
        return m, o, train.build_scheduler(o, conf)

    m_e, o_e, s_e = fresh()
    slot = mv.make_slot(conf, x)
    eager = []
    for s in range(5):
        eager.append(mv.multiview_step(m_e, o_e, s_e, conf, x, seq[s], slot=slot).clone())
    torch.cuda.synchronize()
    m_g, o_g, s_g = fresh()
    it = iter(seq)
    step = mv.graphed_multiview_step(m_g, o_g, s_g, conf, x, lambda: next(it), warmup=2)
    for s in range(2, 5):
        out = step()
        torch.cuda.synchronize()
        assert torch.equal(out.clone(), eager[s]), (s, out, eager[s])  # loss components read after the replay
    pe, pg = dict(m_e.named_parameters()), dict(m_g.named_parameters())
    assert all(torch.equal(pe[k], pg[k]) for k in pe)
    # a refresh with new draws changes the recorded views
    before = step.views["x_i"].clone()
    step()
    torch.cuda.synchronize()
    after = step.views["x_i"].clone()
    assert not torch.equal(before, after)
    ki = seq[5].keep_voxels("i")
    assert torch.equal(after, views_torch(x, seq[5].rot_i, ki))


# ------------------------------------------------------------------------------------------------ 6. input checks
def test_input_checks_raise_before_launch():
    mv = _mv()
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    fx = load_fixture("mv_step_rrc")
    conf = Namespace(**fx.meta["conf"])
    model = SwinUnetR(conf).to(DEV).train()
    opt = train.build_optimizer(model, conf)
    good = mv.draw_views(np.random.RandomState(0), 2, (16, 16, 16), (2, 2, 2), 0.2, False)
    with pytest.raises(ValueError):                                     # H != W
        mv.multiview_step(model, opt, None, conf, torch.rand(2, 1, 16, 8, 16, device=DEV), good)
    with pytest.raises(ValueError):                                     # roi_size != spatial dims
        c2 = Namespace(**vars(conf))
        c2.roi_size = [32, 32, 32]
        mv.multiview_step(model, opt, None, c2, torch.rand(2, 1, 16, 16, 16, device=DEV), good)
    with pytest.raises(ValueError):                                     # mutual on a non-cube
        c3 = Namespace(**vars(conf))
        c3.use_mutual_learning, c3.roi_size = True, [16, 16, 8]
        mv.multiview_step(model, opt, None, c3, torch.rand(2, 1, 16, 16, 8, device=DEV), good)
    assert all(p.grad is None for p in model.parameters())
