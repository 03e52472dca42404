"""Host side of the phase-1 multi-view step (mivp_amd.multiview, train.build_optimizer / build_scheduler for
``self_supervised_learning_encoder``): the draws against the reference's own random_rotate / random_mask /
random_permute, the keep-bit packing, the optimizer partition and schedule of multi_view.py:57-85, and a pure-torch
restatement of the four loss terms pinned to the reference's values (the oracle the GPU tests use)."""
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_fixture, rel_l2


# ------------------------------------------------------------------------------------------------ pure-torch oracle
def views_torch(x, rot, keep):
    """mask(rot90(x[b], rot[b], (H, W))) with one keep pattern [H, W, D] (bool, True = visible) for the batch."""
    out = torch.stack([torch.rot90(x[b], int(rot[b]), (1, 2)) for b in range(x.shape[0])])
    return out * keep.to(out.dtype)


PERMS = {0: (0, 1, 3, 2, 4), 1: (0, 1, 4, 3, 2), 2: (0, 1, 2, 4, 3)}


def rec_loss_torch(rec_i, rec_j, x_i, x_j, keep_i, keep_j, ratio):
    ki, kj = keep_i.to(rec_i.dtype), keep_j.to(rec_i.dtype)
    return F.mse_loss(torch.cat([rec_i * ki, rec_j * kj]), torch.cat([x_i * ki, x_j * kj])) / (1 - ratio)


def rot_loss_torch(rot_i, rot_j, k_i, k_j):
    return F.cross_entropy(torch.cat([rot_i, rot_j]), torch.cat([torch.as_tensor(k_i), torch.as_tensor(k_j)]).long())


def con_loss_torch(z_i, z_j, temp=0.5):
    bs = z_i.shape[0]
    z = torch.cat([F.normalize(z_i, dim=1), F.normalize(z_j, dim=1)])
    sim = F.cosine_similarity(z.unsqueeze(1), z.unsqueeze(0), dim=2)
    pos = torch.exp(torch.cat([torch.diag(sim, bs), torch.diag(sim, -bs)]) / temp)
    neg = (~torch.eye(2 * bs, dtype=torch.bool)).to(z.dtype) * torch.exp(sim / temp)
    return torch.sum(-torch.log(pos / torch.sum(neg, dim=1))) / (2 * bs)


def mut_loss_torch(rec_i, rec_k, perm, keep_i, ratio):
    ki = keep_i.to(rec_i.dtype)
    return F.mse_loss(rec_k.permute(*PERMS[perm]).contiguous() * ki, rec_i * ki) / (1 - ratio)


# ------------------------------------------------------------------------------------------------ draws
def _mv():
    import mivp_amd  # noqa: F401
    from mivp_amd import multiview
    return multiview


def test_draw_views_reproduces_reference_draws():
    mv = _mv()
    fx = load_fixture("mv_draws")
    assert len(fx.meta["cases"]) >= 4
    for n, c in enumerate(fx.meta["cases"]):
        d = mv.draw_views(np.random.RandomState(c["seed"]), c["B"], c["roi"], c["masking_shape"], c["ratio"], c["mutual"])
        g = fx[f"c{n}"]
        assert np.array_equal(d.rot_i, g["rot_i"].numpy()), n
        assert np.array_equal(d.rot_j, g["rot_j"].numpy()), n
        assert torch.equal(d.keep_voxels("i"), g["keep_i"].bool()), n
        assert torch.equal(d.keep_voxels("j"), g["keep_j"].bool()), n
        assert d.perm == c["perm"], n


def test_draw_views_matches_global_stream_order():
    """np.random.seed(s) + the global calls == RandomState(s): the trainer's seeding carries over."""
    mv = _mv()
    a = mv.draw_views(np.random.RandomState(5), 3, (8, 8, 8), (2, 2, 2), 0.2, True)
    b = mv.draw_views(np.random.RandomState(5), 3, (8, 8, 8), (2, 2, 2), 0.2, True)
    assert np.array_equal(a.rot_i, b.rot_i) and np.array_equal(a.keep_j, b.keep_j) and a.perm == b.perm
    n = 64
    assert a.keep_i.sum() == round(n * 0.8) and a.keep_j.sum() == round(n * 0.8)


@pytest.mark.parametrize("grid", [(8, 8, 8), (64, 64, 4), (3, 5, 7), (1, 1, 1), (4, 4, 2)])
def test_keep_bits_round_trip(grid):
    mv = _mv()
    rs = np.random.RandomState(sum(grid))
    keep = rs.rand(*grid) < 0.7
    words = mv.pack_keep(keep)
    assert words.dtype == np.int32 and words.size == (keep.size + 31) // 32
    assert np.array_equal(mv.unpack_keep(words, grid), keep)
    flat = keep.reshape(-1)
    w = words.view(np.uint32)
    for p in (0, flat.size // 3, flat.size - 1):
        assert bool((w[p >> 5] >> (p & 31)) & 1) == bool(flat[p])


@pytest.mark.parametrize("dims,mshape,mutual", [((16, 8, 8), (2, 2, 2), False), ((16, 16, 9), (2, 2, 2), False),
                                                ((16, 16, 8), (2, 2, 2), True)])
def test_draw_views_rejects_bad_shapes(dims, mshape, mutual):
    mv = _mv()
    with pytest.raises(ValueError):
        mv.draw_views(np.random.RandomState(0), 2, dims, mshape, 0.2, mutual)


# ------------------------------------------------------------------------------------------------ optimizer / schedule
def _ssl_conf(ep):
    from mivp_amd import train
    fx = load_fixture("mv_step_rrc")
    conf = Namespace(**fx.meta["conf"])
    conf.use_encoder_prompting = ep
    conf.lr_multi_view, conf.weight_decay_multi_view = 5e-4, 0.1
    conf.lr_prompt_tokens, conf.weight_decay_prompt_tokens = 1e-3, 0.05
    return conf, train, fx


@pytest.mark.parametrize("ep", [True, False])
def test_build_optimizer_multi_view_groups(ep):
    import mivp_amd  # noqa: F401
    from mivp_amd.swin_unetr import SwinUnetR
    conf, train, fx = _ssl_conf(ep)
    model = SwinUnetR(conf)
    opt = train.build_optimizer(model, conf)
    names = {id(p): n for n, p in model.named_parameters()}
    assert len(opt.param_groups) == (2 if ep else 1)
    g0 = opt.param_groups[0]
    assert (g0["lr"], g0["weight_decay"]) == (5e-4, 0.1)
    want0 = fx.meta["param_order_encoder"]
    if not ep:
        want0 = [n for n in want0 if not n.startswith("prompt_tokens")]
    assert [names[id(p)] for p in g0["params"]] == want0
    assert any(n.startswith("extra_heads.reconstruction") for n in want0)
    assert any(n.startswith("extra_heads.contrastive_coding") for n in want0)
    if ep:
        g1 = opt.param_groups[1]
        assert (g1["lr"], g1["weight_decay"]) == (1e-3, 0.05)
        assert [names[id(p)] for p in g1["params"]] == fx.meta["param_order_prompt"]
    # every trainable parameter of the reference's step is in exactly one group
    got = sorted(names[id(p)] for g in opt.param_groups for p in g["params"])
    assert len(got) == len(set(got))
    if ep:
        assert got == sorted(fx.meta["trainable"])


def test_multi_view_schedule_lrs():
    """WarmupCosineSchedule(warmup_steps_multi_view, t_total_multi_view), stepped once per step, on both groups."""
    conf, train, _ = _ssl_conf(True)
    from mivp_amd.swin_unetr import SwinUnetR
    conf.warmup_steps_multi_view, conf.t_total_multi_view = 10, 30
    conf.lr_prompt_tokens = 1e-3
    model = SwinUnetR(conf)
    opt = train.build_optimizer(model, conf)
    sched = train.build_scheduler(opt, conf)
    lrs = []
    for _ in range(40):
        lrs.append([g["lr"] for g in opt.param_groups])
        sched.step()
    want = load_fixture("utils_metrics_schedule")["sched"]["lrs"]      # the reference's schedule, base lrs 5e-4 / 1e-3
    assert torch.allclose(torch.tensor(lrs, dtype=torch.float64), want, rtol=1e-12, atol=0)


def test_ssl_encoder_step_loss_points_to_multiview():
    from mivp_amd import train
    conf, _, _ = train.make_conf("ssl_enc")
    with pytest.raises(ValueError, match="multiview"):
        train.step_loss({}, conf, None)


def test_ssl_enc_workload_is_the_yml_phase1_setting():
    from mivp_amd import train
    conf, size, batch = train.make_conf("ssl_enc")
    assert (size, batch, conf.input_channels) == (96, 4, 1)
    assert conf.use_reconstruction and conf.use_rotation_prediction and conf.use_contrastive_learning
    assert not conf.use_mutual_learning
    assert list(conf.roi_size) == [96, 96, 96] and list(conf.masking_shape) == [2, 2, 2] and conf.masking_ratio == 0.2
    assert (conf.weight_rec, conf.weight_rot, conf.weight_con) == (0.2, 0.5, 0.3)
    assert conf.batch_size_multi_view * conf.num_samples_multi_view == 14


# ------------------------------------------------------------------------------------------------ the loss oracle
@pytest.mark.parametrize("tag", ["a", "b"])
def test_torch_contrastive_restatement_matches_reference(tag):
    fx = load_fixture(f"mv_contrastive_{tag}")
    zi = fx["in"]["z_i"].clone().requires_grad_(True)
    zj = fx["in"]["z_j"].clone().requires_grad_(True)
    loss = con_loss_torch(zi, zj)
    loss.backward()
    assert abs(float(loss) - float(fx["out"]["loss"])) <= 1e-6 * abs(float(fx["out"]["loss"]))
    assert rel_l2(zi.grad, fx["grad"]["z_i"]) < 1e-6
    assert rel_l2(zj.grad, fx["grad"]["z_j"]) < 1e-6


@pytest.mark.parametrize("tag", ["rrc", "mut"])
def test_torch_loss_restatement_matches_reference_step(tag):
    fx = load_fixture(f"mv_step_{tag}")
    conf = Namespace(**fx.meta["conf"])
    x, d = fx["in"]["x"], fx["draws"]
    ki, kj = d["keep_i"].bool(), d["keep_j"].bool()
    x_i, x_j = views_torch(x, d["rot_i"], ki), views_torch(x, d["rot_j"], kj)
    oi, oj = fx["out_i"], fx["out_j"]
    r = conf.masking_ratio
    got = {"rec": rec_loss_torch(oi["reconstruction"], oj["reconstruction"], x_i, x_j, ki, kj, r),
           "rot": rot_loss_torch(oi["rotation_prediction"], oj["rotation_prediction"], d["rot_i"], d["rot_j"]),
           "con": con_loss_torch(oi["contrastive_coding"], oj["contrastive_coding"])}
    if conf.use_mutual_learning:
        got["mut"] = mut_loss_torch(oi["reconstruction"], fx["out_k"]["reconstruction"], fx.meta["perm"], ki, r)
    got["tot"] = conf.weight_rec * got["rec"] + conf.weight_rot * got["rot"] + conf.weight_con * got["con"] \
        + got.get("mut", 0.0)
    assert set(got) == set(fx["loss"])
    for k, v in got.items():
        want = float(fx["loss"][k])
        assert abs(float(v) - want) <= 1e-6 * abs(want), (k, float(v), want)
