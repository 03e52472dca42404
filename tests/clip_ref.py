"""Float64 reference of FusedAdamW's gradient-norm plan (test helper, not a test module).

Written from the comments of ``k_grad_sumsq_multi`` / ``k_grad_clip_plan`` (csrc/proto.hip) and of
``torch.nn.utils.clip_grad_norm_``; nothing here shares code with the package.  The AdamW side of the tests comes from
tests/loss_optim_ref.py, re-exported below.

  sumsq      sum of g*g over every element of every gradient
  norm       sqrt(sumsq)
  coef       min(1, max_norm / (norm + 1e-6)), a NaN kept; exactly 1 without a max_norm
  nonfinite  sumsq is not finite; apply = not (skip_nonfinite and nonfinite)
  counters   steps += 1; clipped += apply and f32(coef) < 1; skipped += not apply; max_norm_seen over finite norms

Bounds (derived, not measured).  The kernel adds the products of a chunk in f32 in a fixed tree whose longest path has
SUMSQ_ADDS additions (the kernel's comment states the same number), and the chunk sums in float64.  Every term is
non-negative, so nothing cancels: each product carries one rounding and each addition on its path one more, and the
relative error of a chunk sum, and of the sum of the chunk sums, is (SUMSQ_ADDS + 1) * 2^-24 to first order (a contracted
multiply-add drops a rounding; the float64 additions are 2^-29 of this).  The square root halves a relative error; the
float64 root, its rounding to f32 and the comparison against a float64 value account for 2 * 2^-24 more.  Products that
underflow (|g| < 2^-63) are outside these bounds; no case has one."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_optim_ref import (ADAM_GROUPS, LADDER_SHAPES, U32, AdamState, adam_case, adam_hyper_row,  # noqa: E402,F401
                            adam_many_case, adamw_ref64, assert_equal_located, assert_within_located, gen)

SUMSQ_ADDS = 12                                   # 3 in a thread, 6 across the lanes of a wave, 3 over the four waves
SUMSQ_REL = (SUMSQ_ADDS + 1) * U32
NORM_REL = 0.5 * SUMSQ_REL + 2.0 * U32
EPS = 1e-6


def sumsq64(grads):
    """Sum of squares of every element of ``grads`` (tensors; None entries are skipped) in float64."""
    return float(sum(float((g.detach().to(torch.float64).cpu() ** 2).sum()) for g in grads if g is not None))


def coef64(norm, max_norm):
    if max_norm is None:
        return 1.0
    c = max_norm / (norm + EPS)
    return c if (c < 1.0 or c != c) else 1.0


def plan_ref(sumsq, max_norm=None, skip_nonfinite=False):
    nonfinite = not math.isfinite(sumsq)
    norm = math.sqrt(sumsq) if sumsq == sumsq else float("nan")
    return dict(sumsq=sumsq, norm=norm, coef=coef64(norm, max_norm), nonfinite=int(nonfinite),
                apply=int(not (skip_nonfinite and nonfinite)))


class Counters:
    """The running values of the record."""

    def __init__(self):
        self.steps = self.clipped = self.skipped = 0
        self.max_norm_seen = 0.0

    def update(self, plan):
        self.steps += 1
        coef32 = float(np.float32(plan["coef"]))
        self.clipped += int(bool(plan["apply"]) and coef32 < 1.0)
        self.skipped += int(not plan["apply"])
        if not plan["nonfinite"]:
            self.max_norm_seen = max(self.max_norm_seen, float(np.float32(plan["norm"])))
        return self


def ulps32(got, want64):
    """|got - want| in units of the f32 spacing at f32(want)."""
    w = np.float32(want64)
    return abs(float(got) - float(want64)) / float(np.spacing(np.abs(w)))


def integer_grads(shapes, seed, amax=15):
    """Integer-valued f32 gradients with |g| <= amax: a chunk's sum of squares stays below 2^24, so f32 adds exactly."""
    g = gen(seed)
    assert 1024 * amax * amax < 2 ** 24
    return [torch.randint(-amax, amax + 1, tuple(s), generator=g).to(torch.float32) for s in shapes]
