"""Pixel-space visual prompts and the input volume's gradient.

``InputPrompt`` learns an additive perturbation of the INPUT of a frozen model (Bahng et al., "Exploring Visual Prompts for
Adapting Large-Scale Models"): ``x' = x + scale * T(P)`` with one f32 parameter ``P [Cin, gh, gw, gd]`` -- a coarse lattice
that ``T`` interpolates trilinearly to the roi under torch's ``align_corners=True`` rule (a low-frequency prompt), or, with
``lattice=None``, one value per voxel (the full-resolution prompt; every interpolation weight is then exactly 0 or 1).  Both
directions are one HIP launch each (csrc/input_prompt.hip): the forward streams ``x`` and evaluates ``T`` on the fly, the
backward gathers ``dP`` per lattice node in a fixed order (no atomics: equal calls give equal bits).  ``dL/dx'`` itself comes from
the patch embedding's data gradient (csrc/norm_embed.hip) plus, in the res-block configurations, torch autograd through the
raw-input skip.

``PromptedModel`` puts a prompt in front of a model; ``build_prompt_optimizer`` builds the ``FusedAdamW`` over it;
``train.train_step`` / ``train.GraphedStep`` run on the wrapper as they do on the model.  ``input_gradient`` /
``saliency_map`` / ``fgsm`` are the other three uses of ``dL/dx``.  Everything stays on the device.

Out of scope: test-time adaptation loops, frequency-domain prompts, padding-frame prompts, prompts on the students /
teacher step."""
from __future__ import annotations

from argparse import Namespace
from typing import Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib as L
from ._host import check_at_least, check_finite, check_flag, check_gpu, check_int_from

MAX_AXES_SUM = 4096          # H + W + D the kernels' per-axis tables take (csrc/input_prompt.hip)


def _three(name: str, v, lo: int = 1) -> Tuple[int, int, int]:
    try:
        vals = None if isinstance(v, (str, bytes)) else tuple(v)
    except TypeError:
        vals = None
    if vals is None or len(vals) != 3:
        raise ValueError(f"{name} must be three integers, got {v!r}")
    return tuple(check_int_from(f"{name}[{a}]", s, lo) for a, s in enumerate(vals))


class _InputPromptFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, P, scale):
        B, cin, H, W, D = x.shape
        xc = x.contiguous()
        Pc = P.detach().contiguous()
        y = torch.empty_like(xc)
        L.call("mivp_input_prompt_fwd", L.ptr(xc), L.ptr(Pc), L.ptr(scale), B, cin, H, W, D, Pc.shape[1], Pc.shape[2],
               Pc.shape[3], L.ptr(y), L.stream())
        ctx.save_for_backward(scale)
        ctx.lattice = tuple(Pc.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        (scale,) = ctx.saved_tensors
        dP = None
        if ctx.needs_input_grad[1]:
            g = dy.contiguous()
            B, cin, H, W, D = g.shape
            dP = torch.empty(ctx.lattice, dtype=torch.float32, device=g.device)
            L.call("mivp_input_prompt_bwd", L.ptr(g), L.ptr(scale), B, cin, H, W, D, ctx.lattice[1], ctx.lattice[2],
                   ctx.lattice[3], L.ptr(dP), L.stream())
        return (dy if ctx.needs_input_grad[0] else None), dP, None     # dx = dx': passed through untouched


class InputPrompt(nn.Module):
    """``x' = x + scale * T(P)`` on f32 ``[B, channels, *roi]`` GPU volumes; ``P`` starts at zero (the identity).

    ``lattice=(gh, gw, gd)``: nodes per axis, ``1 <= g <= roi``; a one-node axis is constant along it; ``None`` is the roi
    itself.  ``scale`` lives in a device float: ``set_scale`` is a stream-ordered copy, legal between the replays of a
    recorded step, so a schedule needs no re-recording."""

    def __init__(self, channels: int, roi: Sequence[int], lattice: Optional[Sequence[int]] = None, scale: float = 1.0):
        super().__init__()
        self.channels = check_int_from("channels", channels, 1)
        self.roi = _three("roi", roi)
        if sum(self.roi) > MAX_AXES_SUM:
            raise ValueError(f"roi {self.roi}: the sum of the three sizes must be at most {MAX_AXES_SUM}")
        self.lattice = self.roi if lattice is None else _three("lattice", lattice)
        for a in range(3):
            if self.lattice[a] > self.roi[a]:
                raise ValueError(f"lattice {self.lattice} has more nodes than the roi {self.roi} has voxels on axis {a}")
        self.P = nn.Parameter(torch.zeros((self.channels, *self.lattice), dtype=torch.float32))
        self.register_buffer("scale", torch.tensor([check_finite("scale", scale)], dtype=torch.float32))

    def set_scale(self, value: float) -> None:
        v = check_finite("scale", value)
        if self.scale.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("InputPrompt.set_scale inside a recording: a recording must not freeze today's scale into the "
                               "graph; call it between replays")
        self.scale.copy_(torch.tensor([v], dtype=torch.float32))

    def check_input(self, x) -> None:
        if not isinstance(x, torch.Tensor) or x.dim() != 5:
            raise ValueError(f"InputPrompt takes [B, {self.channels}, *{self.roi}] volumes, got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        if x.shape[1] != self.channels or tuple(x.shape[2:]) != self.roi:
            raise ValueError(f"InputPrompt was built for [B, {self.channels}, *{self.roi}], got {tuple(x.shape)}")
        if x.shape[0] < 1 or x.numel() >= 2 ** 31:
            raise ValueError(f"InputPrompt: {x.numel()} elements; the kernels take between 1 and 2^31 - 1")
        if x.dtype != torch.float32:
            raise ValueError(f"InputPrompt takes float32 volumes (what the model reads), got {x.dtype}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self.check_input(x)
        check_gpu("the input volume", x)
        if self.P.device != x.device:
            raise RuntimeError(f"InputPrompt is on {self.P.device}, the input on {x.device}")
        return _InputPromptFn.apply(x, self.P, self.scale)

    def extra_repr(self) -> str:
        return f"channels={self.channels}, roi={self.roi}, lattice={self.lattice}"


class PromptedModel(nn.Module):
    """``forward(x) = model(prompt(x))``.  The model's ``named_parameters_*`` partitions are forwarded (so
    ``train.build_optimizer(wrapper, conf)`` still builds the model's own optimizer) and ``named_parameters_input_prompt``
    is added; ``conf`` is the model's."""

    def __init__(self, model: nn.Module, prompt: InputPrompt):
        super().__init__()
        if not isinstance(model, nn.Module):
            raise ValueError(f"model must be an nn.Module, got {type(model).__name__}")
        if isinstance(model, PromptedModel):
            raise ValueError("model is a PromptedModel already: one prompt per model")
        if not isinstance(prompt, InputPrompt):
            raise ValueError(f"prompt must be an InputPrompt, got {type(prompt).__name__}")
        conf = getattr(model, "conf", None)
        cin = getattr(conf, "input_channels", None)
        if cin is not None and int(cin) != prompt.channels:
            raise ValueError(f"the prompt has {prompt.channels} channels, the model reads {cin}")
        self.model = model
        self.prompt = prompt

    @property
    def conf(self):
        return self.model.conf

    def forward(self, x):
        return self.model(self.prompt(x))

    def named_parameters_input_prompt(self):
        return [("prompt.P", self.prompt.P)]

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name.startswith("named_parameters_"):
                return getattr(super().__getattr__("model"), name)
            raise


def build_prompt_optimizer(wrapper: PromptedModel, conf: Namespace, lr: Optional[float] = None, weight_decay: float = 0.0,
                           include_downstream: bool = False, capturable: bool = False, max_grad_norm=None,
                           skip_nonfinite: bool = False):
    """``FusedAdamW`` over the pixel-space prompt (``lr`` defaults to ``conf.lr_prompt_tokens``), with
    ``include_downstream`` together with the model's ``downstream`` partition (prompt tokens and the segmentation head) at
    ``conf.lr_downstream`` / ``conf.weight_decay_downstream`` as a second group."""
    from .optim import FusedAdamW
    if not isinstance(wrapper, PromptedModel):
        raise ValueError(f"build_prompt_optimizer takes a PromptedModel, got {type(wrapper).__name__}")
    lr = float(conf.lr_prompt_tokens) if lr is None else check_at_least("lr", lr, 0.0)
    wd = check_at_least("weight_decay", weight_decay, 0.0)
    groups = [{"params": [p for _, p in wrapper.named_parameters_input_prompt()], "lr": lr, "weight_decay": wd}]
    if check_flag("include_downstream", include_downstream):
        if conf.training_mode != "downstream":
            raise ValueError(f"include_downstream needs training_mode 'downstream', the configuration has {conf.training_mode!r}")
        groups.append({"params": [p for _, p in wrapper.named_parameters_downstream()], "lr": float(conf.lr_downstream),
                       "weight_decay": float(conf.weight_decay_downstream)})
    if max_grad_norm is None:
        max_grad_norm = getattr(conf, "max_grad_norm", None)
    return FusedAdamW(groups, lr=lr, weight_decay=wd, capturable=check_flag("capturable", capturable),
                      max_grad_norm=max_grad_norm, skip_nonfinite=check_flag("skip_nonfinite", skip_nonfinite))


def _check_volume(x):
    check_gpu("x", x)
    if x.dim() != 5 or not x.is_floating_point():
        raise ValueError(f"x must be a floating-point [B, C, H, W, D] volume, got {x.dtype} {tuple(x.shape)}")


def input_gradient(model: nn.Module, x: torch.Tensor, y: torch.Tensor, conf: Namespace) -> torch.Tensor:
    """``dL/dx`` of ``train.step_loss(model(x), conf, y)``, f32 in the shape of ``x``.  The model runs in the mode it is in
    (a model in ``train()`` updates its BatchNorm statistics as any forward does); no parameter's ``.grad`` is touched."""
    from . import train
    _check_volume(x)
    xg = x.detach().requires_grad_(True)
    with torch.enable_grad():
        loss = train.step_loss(model(xg), conf, y)
        (g,) = torch.autograd.grad(loss, xg, grad_outputs=train.unit_grad(loss))
    return g.float()


def saliency_map(model: nn.Module, x: torch.Tensor, y: torch.Tensor, conf: Namespace) -> torch.Tensor:
    """Channel-wise maximum of ``|dL/dx|``: f32 ``[B, H, W, D]``."""
    return input_gradient(model, x, y, conf).abs().amax(dim=1)


def fgsm(model: nn.Module, x: torch.Tensor, y: torch.Tensor, conf: Namespace, eps: float) -> torch.Tensor:
    """One fast-gradient-sign step ``x + eps * sign(dL/dx)`` (Goodfellow et al.); ``eps == 0`` returns a copy of ``x``."""
    eps = check_at_least("eps", eps, 0.0)
    _check_volume(x)
    if eps == 0.0:
        return x.detach().clone()
    return x.detach() + eps * input_gradient(model, x, y, conf).sign().to(x.dtype)
