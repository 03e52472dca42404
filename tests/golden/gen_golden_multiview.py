#!/usr/bin/env python3
"""Generate the phase-1 (multi-view) golden fixtures under tests/golden/ from the REFERENCE's own code.

Reuses gen_golden.py's import boundary (``_import_reference``: the synthetic parent package, the MONAI stand-in for the
two swin_unetr files) plus an empty ``cv2`` placeholder (utils.py imports it for its PNG viewers only) and an empty
``torchinfo.summary`` stand-in (multi_view.py logs a model summary).  The proxy heads are stock torch layers, so no new
stand-in boundary is involved.  Only DATA is written.

  mv_draws.npz            random_rotate / random_mask / random_permute (utils.py:267-350) under np.random.seed(s), in the
                          trainer's order (rotate i, rotate j, mask i, mask j, permute), for several seeds, batches and roi
                          shapes, 128x128x8 included
  mv_contrastive_{a,b}    ContrastivePairLoss (losses/contrastive_pair_loss.py): z_i, z_j, loss, both gradients; a: B = 2,
                          dim 32 with a nearly parallel pair; b: B = 14, dim 512
  mv_step_{rrc,mut}       MultiViewTrainer.self_supervised_learning (multi_view.py:96-176) driven for ONE step on a
                          one-batch loader: the reference SwinUnetR in self_supervised_learning_encoder mode, 16^3, B = 2,
                          dropout 0, GEMM weights rounded to bf16 first (the HIP model's operand precision).  The trainer's
                          own loop draws the views and computes the losses; AdamW.step is wrapped to record every trainable
                          gradient (and the BatchNorm running statistics after the step's forwards), then stops the run
                          before the update.  rrc: reconstruction + rotation + contrastive, encoder prompting on;
                          mut: the same plus the mutual term, prompting off.  The head outputs of every
                          forward are stored too (out_i / out_j / out_k), so the loss formulas can be checked on their own.

Usage:  python tests/golden/gen_golden_multiview.py
"""
import os
import sys
import types
from argparse import Namespace

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from gen_golden import _import_reference, _randomize, _save, tiny_conf  # noqa: E402

PERM_SHAPES = {(3, 2, 4): 0, (4, 3, 2): 1, (2, 4, 3): 2}     # random_permute's codes, told apart on a 2x3x4 probe


def _placeholders():
    if "cv2" not in sys.modules:
        try:
            import cv2  # noqa: F401
        except ImportError:
            sys.modules["cv2"] = types.ModuleType("cv2")
    if "torchinfo" not in sys.modules:
        try:
            import torchinfo  # noqa: F401
        except ImportError:
            ti = types.ModuleType("torchinfo")
            ti.summary = lambda model, *a, **k: ""
            sys.modules["torchinfo"] = ti


def _perm_code(fn):
    return PERM_SHAPES[tuple(fn(torch.zeros(1, 1, 2, 3, 4)).shape[2:])]


def _round_bf16(sd):
    out = {}
    for k, v in sd.items():
        if v.is_floating_point() and v.dim() >= 2 and not k.startswith("prompt_tokens") and ".pe." not in k \
                and not k.startswith("input_layer.0"):
            out[k] = v.to(torch.bfloat16).to(torch.float32)
        else:
            out[k] = v.clone()
    return out


def gen_draws(U):
    cases = [(0, 2, (16, 16, 16), (2, 2, 2), 0.2, True), (1, 4, (96, 96, 96), (2, 2, 2), 0.2, True),
             (2, 14, (128, 128, 8), (2, 2, 2), 0.2, False), (3, 3, (32, 32, 16), (4, 4, 2), 0.35, False),
             (7, 2, (24, 24, 24), (4, 2, 6), 0.5, True)]
    arrays, meta = {}, {"cases": []}
    for n, (seed, B, roi, ms, ratio, mutual) in enumerate(cases):
        np.random.seed(seed)
        x = torch.zeros(B, 1, *roi)
        x_i, k_i = U.random_rotate(x)
        x_j, k_j = U.random_rotate(x)
        x_i, m_i = U.random_mask(x_i, list(roi), list(ms), ratio)
        x_j, m_j = U.random_mask(x_j, list(roi), list(ms), ratio)
        arrays[f"c{n}/rot_i"] = k_i
        arrays[f"c{n}/rot_j"] = k_j
        arrays[f"c{n}/keep_i"] = m_i.numpy().astype(np.uint8)
        arrays[f"c{n}/keep_j"] = m_j.numpy().astype(np.uint8)
        perm = None
        if mutual:
            _, fn = U.random_permute(x_i)
            perm = _perm_code(fn)
        meta["cases"].append({"seed": seed, "B": B, "roi": list(roi), "masking_shape": list(ms), "ratio": ratio,
                              "mutual": mutual, "perm": perm})
    _save("mv_draws", arrays, meta)


def gen_contrastive(CPL):
    for tag, B, dim, seed in [("a", 2, 32, 3), ("b", 14, 512, 4)]:
        g = torch.Generator().manual_seed(seed)
        zi = torch.randn(B, dim, generator=g)
        zj = torch.randn(B, dim, generator=g)
        if tag == "a":
            zj[0] = zi[0] * 1.7 + 1e-3 * torch.randn(dim, generator=g)      # a nearly parallel positive pair
        else:
            zj = 0.6 * zi + 0.8 * zj                                         # correlated pairs, as trained codes are
        zi.requires_grad_(True)
        zj.requires_grad_(True)
        loss = CPL(B)(zi, zj)
        loss.backward()
        _save(f"mv_contrastive_{tag}", {"in/z_i": zi, "in/z_j": zj, "out/loss": loss.reshape(1), "grad/z_i": zi.grad,
                                        "grad/z_j": zj.grad}, {"bs": B, "dim": dim, "temp": 0.5})


class _Stop(Exception):
    pass


class _Loader(list):
    def __init__(self, items):
        super().__init__(items)
        self.dataset = list(items)


def gen_step(su, mv, tag, ep, mutual, seed):
    torch.manual_seed(40 + seed)
    conf = tiny_conf("self_supervised_learning_encoder", ep, False)
    conf.use_reconstruction = conf.use_rotation_prediction = conf.use_contrastive_learning = True
    conf.use_mutual_learning = mutual
    conf.contrastive_coding_dim = 32
    hp = Namespace(**vars(conf), gpu=0, roi_size=[16, 16, 16], masking_shape=[2, 2, 2], masking_ratio=0.2,
                   weight_rec=0.2, weight_rot=0.5, weight_con=0.3, max_epochs_multi_view=0, lr_multi_view=5e-4,
                   weight_decay_multi_view=0.1, num_samples_multi_view=1, batch_size_multi_view=2,
                   warmup_steps_multi_view=100, t_total_multi_view=4000, lr_prompt_tokens=5e-4,
                   weight_decay_prompt_tokens=0.1, load_ckpt_backbone=False, summary_dir="-", view=False,
                   save_ckpt_backbone=False)
    model = su.SwinUnetR(hp)
    _randomize(model, torch.Generator().manual_seed(8 + seed))
    model.load_state_dict(_round_bf16(model.state_dict()))
    sd_before = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.rand(2, 1, 16, 16, 16, generator=torch.Generator().manual_seed(60 + seed))

    rec = {}
    orig = {n: getattr(mv, n) for n in ("random_rotate", "random_mask", "random_permute")}

    def w_rotate(t):
        out = orig["random_rotate"](t)
        rec.setdefault("rot", []).append(out[1].clone())
        return out

    def w_mask(t, *a):
        out = orig["random_mask"](t, *a)
        rec.setdefault("keep", []).append(out[1].clone())
        return out

    def w_permute(t):
        out = orig["random_permute"](t)
        rec["perm"] = _perm_code(out[1])
        return out

    trainer = mv.MultiViewTrainer(hp, lambda h: model, _Loader([{"image": x, "name": ["v0"]}]), _Loader([]),
                                  types.SimpleNamespace(info=lambda *a, **k: None),
                                  types.SimpleNamespace(add_scalar=lambda *a, **k: None))
    trainer.device = torch.device("cpu")
    losses = {}
    conf_losses = trainer.configure_losses

    def w_configure_losses():
        out = conf_losses()
        losses["avg"] = out[1]
        return out
    trainer.configure_losses = w_configure_losses
    grads, after = {}, {}

    def w_step(self_opt, *a, **k):
        for n, q in model.named_parameters():
            if q.requires_grad:
                grads[n] = q.grad.clone() if q.grad is not None else torch.zeros_like(q)
        for n, v in model.state_dict().items():
            if "running_" in n or "num_batches" in n:
                after[n] = v.clone()
        raise _Stop()

    calls = []
    model.register_forward_hook(lambda m, inp, out: calls.append({k: v.detach().clone() for k, v in out.items()
                                                                  if k != "out_vit"}))
    old_step = torch.optim.AdamW.step
    for n in orig:
        setattr(mv, n, {"random_rotate": w_rotate, "random_mask": w_mask, "random_permute": w_permute}[n])
    torch.optim.AdamW.step = w_step
    np.random.seed(seed)
    try:
        trainer.self_supervised_learning()
        raise RuntimeError("the trainer finished without reaching the optimizer step")
    except _Stop:
        pass
    finally:
        torch.optim.AdamW.step = old_step
        for n, f in orig.items():
            setattr(mv, n, f)
    avg = losses["avg"]
    arrays = {f"sd/{k}": v for k, v in sd_before.items()}
    arrays.update({"in/x": x, "draws/rot_i": rec["rot"][0], "draws/rot_j": rec["rot"][1],
                   "draws/keep_i": rec["keep"][0].numpy().astype(np.uint8),
                   "draws/keep_j": rec["keep"][1].numpy().astype(np.uint8)})
    for name in ("rec", "rot", "con", "mut", "tot"):
        if name in avg:
            arrays[f"loss/{name}"] = avg[name][-1].detach().reshape(1)
    for k, v in grads.items():
        arrays[f"grad/{k}"] = v
    for view, out in zip("ijk", calls):
        for k, v in out.items():
            arrays[f"out_{view}/{k}"] = v
    for k, v in after.items():
        arrays[f"after/{k}"] = v
    meta = {"conf": {k: v for k, v in vars(hp).items()}, "trainable": sorted(grads), "seed": seed,
            "perm": rec.get("perm"),
            "param_order_encoder": [n for n, _ in _named(model, model.named_parameters_encoder())],
            "note": "MONAI stand-in used: parity unpinned at the MONAI boundary; weights bf16-rounded before the step"}
    if ep:
        meta["param_order_prompt"] = [n for n, _ in _named(model, model.named_parameters_prompt_tokens_encoder())]
    _save(f"mv_step_{tag}", arrays, meta)


def _named(model, plist):
    ids = {id(q): k for k, q in model.named_parameters()}
    return [(ids[id(q)], q) for _, q in plist]


if __name__ == "__main__":
    torch.set_num_threads(8)
    sb, down, wa, rpe, ub, su = _import_reference()
    _placeholders()
    from refmodules import utils as U
    from refmodules.losses import contrastive_pair_loss as cpl
    from refmodules import multi_view as mv
    gen_draws(U)
    gen_contrastive(cpl.ContrastivePairLoss)
    gen_step(su, mv, "rrc", True, False, 1)
    gen_step(su, mv, "mut", False, True, 2)
