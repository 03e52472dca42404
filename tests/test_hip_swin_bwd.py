"""GPU parity of the Swin-block and patch-merge BACKWARD kernels against autograd over the oracle.

Gradients flow through several bf16 rounding points (dO, dt1, dq/dk/dv, dS, dx), so the tolerance is
looser than forward: rel-L2 <= 1.5e-2 for dx (bf16 tensor), <= 1.5e-2 for the fp32 prompt / prompt-bias
gradients (they are sums over every window of bf16-rounded products).

PRIMARY bar (round 2): the same comparison against the rounding-aware oracle (``emulate_bf16=True``, straight-through
gradient through each rounding): forward storage rounding is then common to both sides and what remains is the backward
path's own bf16 storage (dO, dt1, dS, dq / dk / dv, dx): rel-L2 <= TIGHT_BWD for dx and the prompt gradients."""
import pytest
import torch

from conftest import load_fixture, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIGHT_FWD = 2e-3
TIGHT_BWD = 5e-3


def r16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _rounded_state(sd):
    out = {}
    for k, v in sd.items():
        if v.is_floating_point() and v.dim() == 2 and ("to_" in k or "proj.weight" in k or k.endswith("mlp.weight")
                                                       or "reduction" in k):
            out[k] = r16(v)
        else:
            out[k] = v.clone()
    return out


def _run_block(sd, x, prm, gout, window, shift, heads, need_dx=True, emulate=False):
    import mivp_amd
    from mivp_amd import swin_ops
    from oracle import swin_ref as S
    n_prompt = 0 if prm is None else prm.shape[0]
    sdo = {k: v.clone() for k, v in sd.items()}
    tok_keys = [k for k in sdo if "weights_token" in k or "enc_token" in k] if n_prompt else []
    for k in tok_keys:
        sdo[k].requires_grad_(True)
    xo = x.clone().requires_grad_(True)
    po = prm.clone().requires_grad_(True) if prm is not None else None
    want = S.swin_block(xo, po, sdo, "", window, shift, heads, emulate_bf16=emulate)
    want.backward(gout)
    w = swin_ops.weights_from_state(sd, "", heads, 64, 0, torch.device(DEV), need_bwd=True)
    ts = None
    leafs = {}
    if n_prompt:
        for k in tok_keys:
            leafs[k] = sd[k].clone().to(DEV).requires_grad_(True)
        ts = (leafs["pe.weights_token"] @ leafs["pe.enc_token.0"].t())[:, :n_prompt] * (64 ** -0.5)
    xc = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    pd = None if prm is None else prm.to(DEV)
    y, saved = swin_ops.swin_block_forward(xc, pd, w, ts, window, shift, save=True)
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    dx, dprompt, dts = swin_ops.swin_block_backward(saved, w, pd, dy, need_dx, n_prompt > 0)
    torch.cuda.synchronize()
    res = {"y": (rel_l2(y.float().cpu().permute(0, 4, 1, 2, 3), want), None)}
    if need_dx:
        res["dx"] = (rel_l2(dx.float().cpu().permute(0, 4, 1, 2, 3), xo.grad), None)
    if n_prompt:
        res["dprompt"] = (rel_l2(dprompt.cpu(), po.grad), None)
        ts.backward(dts)
        for k in tok_keys:
            res["d" + k] = (rel_l2(leafs[k].grad.cpu(), sdo[k].grad), None)
    return res


BLOCKS = ["nopad_noshift", "nopad_shift", "nopad_shift_prompt", "oddpad_shift_prompt",
          "evenpad_noshift_prompt", "smalldim_shift", "smalldim_pad_prompt", "w442_shift_prompt"]


@pytest.mark.parametrize("tag", BLOCKS)
def test_block_backward_golden_shapes(tag):
    fx = load_fixture(f"block_{tag}")
    m = fx.meta
    sd = _rounded_state(fx["sd"])
    res = _run_block(sd, r16(fx["in"]["x"]), fx["in"].get("prompt"), r16(fx["in"]["gout"]), m["window"], m["shift"],
                     m["heads"])
    assert res["y"][0] < 6e-3
    for k, (err, _) in res.items():
        assert err < 1.5e-2, (tag, k, err)
    tight = _run_block(sd, r16(fx["in"]["x"]), fx["in"].get("prompt"), r16(fx["in"]["gout"]), m["window"], m["shift"],
                       m["heads"], emulate=True)
    print(f"[tight] block_{tag} backward vs rounding-aware oracle:", {k: f"{v[0]:.2e}" for k, v in tight.items()})
    assert tight["y"][0] < TIGHT_FWD
    for k, (err, _) in tight.items():
        assert err < TIGHT_BWD, (tag, k, err)


@pytest.mark.parametrize("window,dims,C,heads,n_prompt,shift,need_dx", [
    ((7, 7, 7), (14, 14, 14), 48, 4, 64, (3, 3, 3), True),
    ((7, 7, 7), (14, 14, 14), 48, 4, 64, (0, 0, 0), False),   # first prompted block: prompt gradients only
    ((7, 7, 7), (12, 12, 24), 96, 8, 64, (3, 3, 3), True),
    ((7, 7, 7), (6, 6, 24), 192, 16, 64, (3, 3, 3), True),
    ((7, 7, 7), (12, 12, 24), 96, 4, 0, (3, 3, 3), True),       # decoder, hd 24, no prompts
    ((7, 7, 7), (6, 6, 24), 192, 4, 64, (3, 3, 3), True),       # decoder with prompts, hd 48 (chunked LDS)
    ((7, 7, 7), (12, 12, 24), 96, 4, 0, (0, 0, 0), True),       # hd 24 un-shifted: the dq pass at two workgroups per CU
    ((7, 7, 7), (6, 6, 24), 192, 4, 0, (3, 3, 3), True),        # hd 48 without prompts: 22 key tiles, two per wave in the shifted dkv pass
    ((7, 7, 7), (6, 6, 24), 192, 4, 0, (0, 0, 0), True),        # ... three per wave (one workgroup per window and head) un-shifted
    ((8, 8, 4), (16, 16, 8), 48, 4, 64, (4, 4, 2), True),
    ((2, 4, 4), (2, 4, 4), 128, 16, 0, (0, 0, 0), True),        # one 32-slot window: the 16-token backward kernels with eight channel tiles
    ((2, 4, 4), (2, 4, 4), 64, 16, 0, (0, 0, 0), True),         # ... with four
    ((2, 4, 4), (2, 4, 4), 384, 32, 0, (0, 0, 0), True),        # C = 384: the column-split / row-image backward kernels with 24 channel tiles
    ((2, 2, 4), (2, 2, 4), 96, 8, 0, (0, 0, 0), True),          # one 16-slot window: the 16-token backward kernels with six channel tiles
    ((2, 2, 4), (2, 2, 4), 192, 16, 0, (0, 0, 0), True),        # ... with twelve
])
def test_block_backward_real_sizes(window, dims, C, heads, n_prompt, shift, need_dx):
    from oracle.unetr_ref import _block_state
    gen = torch.Generator().manual_seed(2)
    sd = {}
    _block_state(sd, "", C, heads, list(window), 64, max(n_prompt, 1), n_prompt > 0, gen)
    for k in list(sd):
        if "norm.weight" in k:
            sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=gen)
        if "norm.bias" in k or k.endswith("proj.bias") or k.endswith("mlp.bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=gen)
    sd = _rounded_state(sd)
    x = r16(torch.randn(1, C, *dims, generator=gen))
    prm = 0.5 * torch.randn(n_prompt, C, generator=gen) if n_prompt else None
    gout = r16(torch.randn(1, C, *dims, generator=gen))
    res = _run_block(sd, x, prm, gout, window, shift, heads, need_dx)
    for k, (err, _) in res.items():
        assert err < 1.5e-2, (k, err)
    tight = _run_block(sd, x, prm, gout, window, shift, heads, need_dx, emulate=True)
    print(f"[tight] C={C} heads={heads} dims={dims} backward vs rounding-aware oracle:", {k: f"{v[0]:.2e}" for k, v in tight.items()})
    assert tight["y"][0] < TIGHT_FWD
    for k, (err, _) in tight.items():
        assert err < TIGHT_BWD, (k, err)


WEIGHT_KEYS = {"ln1_w": "attn_norm.weight", "ln1_b": "attn_norm.bias", "wq": "attn.to_q.weight", "wk": "attn.to_k.weight",
               "wv": "attn.to_v.weight", "wproj": "attn.proj.weight", "bproj": "attn.proj.bias", "ln2_w": "mlp_norm.weight",
               "ln2_b": "mlp_norm.bias", "wmlp": "mlp.weight", "bmlp": "mlp.bias"}


def _run_block_weight_grads(sd, x, prm, gout, window, shift, heads):
    """All parameter gradients of one block (the *_all / *_decoder training modes) vs autograd over the oracle."""
    import mivp_amd
    from mivp_amd import swin_ops
    from oracle import swin_ref as S
    n_prompt = 0 if prm is None else prm.shape[0]
    sdo = {k: v.clone() for k, v in sd.items()}
    for k, v in sdo.items():
        if v.is_floating_point() and (n_prompt or "token" not in k):
            v.requires_grad_(True)
    xo = x.clone().requires_grad_(True)
    po = prm.clone().requires_grad_(True) if prm is not None else None
    S.swin_block(xo, po, sdo, "", window, shift, heads).backward(gout)

    w = swin_ops.weights_from_state(sd, "", heads, 64, 0, torch.device(DEV), need_bwd=True)
    leafs = {k: sd[k].clone().to(DEV).requires_grad_(True) for k in sd if k.startswith("pe.") and sd[k].is_floating_point()}
    scale = 64 ** -0.5
    tabs = [(leafs[f"pe.weights_content_{a}"] @ leafs[f"pe.enc_content_{a}"].t()) * (scale / 3.0) for a in "hwd"]
    ts = None
    if n_prompt:
        ts = (leafs["pe.weights_token"] @ leafs["pe.enc_token.0"].t())[:, :n_prompt] * scale
    xc = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    pd = None if prm is None else prm.to(DEV)
    y, saved = swin_ops.swin_block_forward(xc, pd, w, ts, window, shift, save=True)
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    dx, dprompt, dts, wg = swin_ops.swin_block_backward(saved, w, pd, dy, True, n_prompt > 0, need_w=True)
    torch.cuda.synchronize()
    res = {"dx": rel_l2(dx.float().cpu().permute(0, 4, 1, 2, 3), xo.grad)}
    for short, key in WEIGHT_KEYS.items():
        assert torch.isfinite(wg[short]).all(), short
        res[key] = rel_l2(wg[short].cpu().reshape(sdo[key].shape), sdo[key].grad)
    torch.autograd.backward(tabs + ([ts] if n_prompt else []), [wg["t_h"], wg["t_w"], wg["t_d"]] + ([dts] if n_prompt else []))
    for k, leaf in leafs.items():
        if sdo[k].grad is not None:
            res[k] = rel_l2(leaf.grad.cpu(), sdo[k].grad)
    if n_prompt:
        res["dprompt"] = rel_l2(dprompt.cpu(), po.grad)
    return res


@pytest.mark.parametrize("tag", BLOCKS)
def test_block_weight_gradients_golden_shapes(tag):
    """Tolerance 1.5e-2 rel-L2 as for dx: the operands of every weight-gradient product are bf16-rounded
    activations / activation gradients; the sums themselves are fp32.  The relative-position table gradients get
    3e-2: they are signed sums of dS over a handful of windows in these toy shapes, and every softmax row of dS sums
    to zero, so the bf16 rounding of q / k / dO upstream is amplified by the cancellation (measured 0.2-1.7e-2)."""
    fx = load_fixture(f"block_{tag}")
    m = fx.meta
    sd = _rounded_state(fx["sd"])
    res = _run_block_weight_grads(sd, r16(fx["in"]["x"]), fx["in"].get("prompt"), r16(fx["in"]["gout"]), m["window"],
                                  m["shift"], m["heads"])
    for k, err in res.items():
        assert err < (3e-2 if "content" in k else 1.5e-2), (tag, k, err)


@pytest.mark.parametrize("window,dims,C,heads,n_prompt,shift", [
    ((7, 7, 7), (14, 14, 14), 48, 4, 64, (3, 3, 3)),
    ((7, 7, 7), (12, 12, 24), 96, 8, 0, (0, 0, 0)),
    ((7, 7, 7), (6, 6, 24), 192, 4, 64, (3, 3, 3)),       # decoder with prompts, hd 48
    ((8, 8, 4), (16, 16, 8), 48, 4, 64, (4, 4, 2)),
])
def test_block_weight_gradients_real_sizes(window, dims, C, heads, n_prompt, shift):
    from oracle.unetr_ref import _block_state
    gen = torch.Generator().manual_seed(5)
    sd = {}
    _block_state(sd, "", C, heads, list(window), 64, max(n_prompt, 1), n_prompt > 0, gen)
    for k in list(sd):
        if "norm.weight" in k:
            sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=gen)
        if "norm.bias" in k or k.endswith("proj.bias") or k.endswith("mlp.bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=gen)
    sd = _rounded_state(sd)
    x = r16(torch.randn(2, C, *dims, generator=gen))
    prm = 0.5 * torch.randn(n_prompt, C, generator=gen) if n_prompt else None
    gout = r16(torch.randn(2, C, *dims, generator=gen))
    res = _run_block_weight_grads(sd, x, prm, gout, window, shift, heads)
    for k, err in res.items():
        assert err < 1.5e-2, (k, err)


@pytest.mark.parametrize("tag,p_attn,p_proj", [("oddpad_shift_prompt", 0.1, 0.1), ("nopad_shift", 0.25, 0.0),
                                               ("w442_shift_prompt", 0.0, 0.3)])
def test_block_dropout_matches_oracle_under_the_same_masks(tag, p_attn, p_proj):
    """attn_drop / proj_drop (window_attention.py:57,60): the kernels draw their masks from a counter hash, so the
    random stream cannot equal nn.Dropout's; instead the masks the kernels used are exported through
    mivp_dropout_masks and handed to the oracle, after which forward, dx, prompt and weight gradients must agree as
    in the dropout-free tests.  The drop rate itself is checked against p."""
    import ctypes as C
    import mivp_amd
    from mivp_amd import swin_ops, _lib as L
    from oracle import swin_ref as S
    fx = load_fixture(f"block_{tag}")
    m = fx.meta
    window, shift, heads = m["window"], m["shift"], m["heads"]
    sd = _rounded_state(fx["sd"])
    x, prm, gout = r16(fx["in"]["x"]), fx["in"].get("prompt"), r16(fx["in"]["gout"])
    n_prompt = 0 if prm is None else prm.shape[0]
    w = swin_ops.weights_from_state(sd, "", heads, 64, 0, torch.device(DEV), need_bwd=True)
    ts = None
    if n_prompt:
        ts = ((sd["pe.weights_token"] @ sd["pe.enc_token.0"].t())[:, :n_prompt] * (64 ** -0.5)).to(DEV)
    xc = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    pd = None if prm is None else prm.to(DEV)
    y, saved = swin_ops.swin_block_forward(xc, pd, w, ts, window, shift, save=True, dropout=(p_attn, p_proj, 1234, 987))
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    dx, dprompt, dts, wg = swin_ops.swin_block_backward(saved, w, pd, dy, True, n_prompt > 0, need_w=True)
    d = saved.desc
    B, P, Nq, Nqp, Nkp, Cc = d.B, d.P, d.Nq, d.Nqp, d.Nkp, d.C
    ak = torch.empty((B * P * heads, Nqp, Nkp), dtype=torch.uint8, device=DEV)
    pk = torch.empty((B * P * Nqp, Cc), dtype=torch.uint8, device=DEV)
    L.call("mivp_dropout_masks", C.byref(d), L.ptr(ak), L.ptr(pk), L.stream())
    torch.cuda.synchronize()
    ak = ak.cpu().view(B, P, heads, Nqp, Nkp).float()
    cols = list(range(Nq)) + list(range(Nqp, Nqp + n_prompt))            # oracle key order: window slots, then prompts
    attn_keep = ak[:, :, :, :Nq][..., cols] * float(d.attn_drop_scale)
    proj_keep = pk.cpu().view(B, P, Nqp, Cc)[:, :, :Nq].float() * float(d.proj_drop_scale)
    if p_attn:
        assert abs(1.0 - float(ak.mean()) - p_attn) < 0.02
    if p_proj:
        assert abs(1.0 - float(pk.float().mean()) - p_proj) < 0.03
    sdo = {k: v.clone() for k, v in sd.items()}
    for k, v in sdo.items():
        if v.is_floating_point() and "pe." not in k:
            v.requires_grad_(True)
    xo = x.clone().requires_grad_(True)
    po = prm.clone().requires_grad_(True) if prm is not None else None
    want = S.swin_block(xo, po, sdo, "", window, shift, heads, 64, attn_keep if p_attn else None,
                        proj_keep if p_proj else None)
    want.backward(gout)
    assert rel_l2(y.float().cpu().permute(0, 4, 1, 2, 3), want.detach()) < 6e-3
    assert rel_l2(dx.float().cpu().permute(0, 4, 1, 2, 3), xo.grad) < 1.5e-2
    if n_prompt:
        assert rel_l2(dprompt.cpu(), po.grad) < 1.5e-2
    for short, key in WEIGHT_KEYS.items():
        assert rel_l2(wg[short].cpu().reshape(sdo[key].shape), sdo[key].grad) < 1.5e-2, key
    # without the masks the oracle must NOT agree (the test would be vacuous if dropout were a no-op)
    plain = S.swin_block(x, prm, sd, "", window, shift, heads)
    assert rel_l2(y.float().cpu().permute(0, 4, 1, 2, 3), plain) > 2e-2


@pytest.mark.parametrize("dims,C,heads,shift,p_attn,p_proj", [
    ((14, 14, 14), 48, 4, (3, 3, 3), 0.0, 0.2),      # C = 48: proj dropout in the row-image proj + MLP pair (forward and backward)
    ((12, 12, 24), 96, 4, (0, 0, 0), 0.1, 0.1),      # C = 96, head_dim 24: + attention dropout in the two-pass backward (shared pair hashes)
    ((14, 14, 14), 48, 4, (3, 3, 3), 0.15, 0.0),     # fused backward with dropout at two workgroups per CU, shifted windows
])
def test_block_dropout_real_sizes_under_exported_masks(dims, C, heads, shift, p_attn, p_proj):
    """The same check as test_block_dropout_matches_oracle_under_the_same_masks at model widths, data gradients only: these are
    the shapes that take the row-image token kernels and the one-pass / two-workgroup attention backward (round 3: proj dropout
    inside k_proj_mlp_fwd_wide / k_proj_mlp_bwd_wide, pair hashes shared between adjacent lanes in the backward kernels)."""
    import ctypes as C_
    import mivp_amd  # noqa: F401
    from mivp_amd import swin_ops, _lib as L
    from oracle import swin_ref as S
    from oracle.unetr_ref import _block_state
    window = (7, 7, 7)
    gen = torch.Generator().manual_seed(7)
    sd = {}
    _block_state(sd, "", C, heads, list(window), 64, 1, False, gen)
    for k in list(sd):
        if "norm.weight" in k:
            sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=gen)
        if "norm.bias" in k or k.endswith("proj.bias") or k.endswith("mlp.bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=gen)
    sd = _rounded_state(sd)
    x = r16(torch.randn(1, C, *dims, generator=gen))
    gout = r16(torch.randn(1, C, *dims, generator=gen))
    w = swin_ops.weights_from_state(sd, "", heads, 64, 0, torch.device(DEV), need_bwd=True)
    xc = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    y, saved = swin_ops.swin_block_forward(xc, None, w, None, window, shift, save=True, dropout=(p_attn, p_proj, 4321, 789))
    dx, _, _ = swin_ops.swin_block_backward(saved, w, None, dy, True, False)
    d = saved.desc
    B, P, Nq, Nqp, Nkp, Cc = d.B, d.P, d.Nq, d.Nqp, d.Nkp, d.C
    ak = torch.empty((B * P * heads, Nqp, Nkp), dtype=torch.uint8, device=DEV)
    pk = torch.empty((B * P * Nqp, Cc), dtype=torch.uint8, device=DEV)
    L.call("mivp_dropout_masks", C_.byref(d), L.ptr(ak), L.ptr(pk), L.stream())
    torch.cuda.synchronize()
    attn_keep = ak.cpu().view(B, P, heads, Nqp, Nkp).float()[:, :, :, :Nq, :Nq] * float(d.attn_drop_scale)
    proj_keep = pk.cpu().view(B, P, Nqp, Cc)[:, :, :Nq].float() * float(d.proj_drop_scale)
    if p_attn:
        assert abs(1.0 - float(ak.float().mean()) - p_attn) < 0.01
    if p_proj:
        assert abs(1.0 - float(pk.float().mean()) - p_proj) < 0.01
    xo = x.clone().requires_grad_(True)
    want = S.swin_block(xo, None, sd, "", window, shift, heads, 64, attn_keep if p_attn else None, proj_keep if p_proj else None)
    want.backward(gout)
    e_y = rel_l2(y.float().cpu().permute(0, 4, 1, 2, 3), want.detach())
    e_dx = rel_l2(dx.float().cpu().permute(0, 4, 1, 2, 3), xo.grad)
    print(f"[dropout real sizes] C={C} shift={shift} p=({p_attn}, {p_proj}): y {e_y:.2e} dx {e_dx:.2e}")
    assert e_y < 6e-3 and e_dx < 1.5e-2
    plain = S.swin_block(x, None, sd, "", window, shift, heads)
    assert rel_l2(y.float().cpu().permute(0, 4, 1, 2, 3), plain) > 3 * e_y   # dropout was not a no-op (attention dropout alone moves y by ~0.8 %)


def test_dropout_epoch_word_moves_the_masks():
    """mivp.h ``MivpSwinDesc.seed_epoch`` (ABI 12): the dropout kernels fold a device-resident epoch word into their seeds, so
    a recorded graph (frozen descriptor) draws new masks per replay.  Exported masks: NULL == word 0; different words give
    different masks at the same keep rate; forward + backward under a non-zero word still agree with the oracle under the
    exported masks (the same check as above, on one fixture)."""
    import ctypes as C
    import mivp_amd  # noqa: F401
    from mivp_amd import swin_ops, _lib as L
    from oracle import swin_ref as S
    fx = load_fixture("block_oddpad_shift_prompt")
    m = fx.meta
    window, shift, heads = m["window"], m["shift"], m["heads"]
    sd = _rounded_state(fx["sd"])
    x, prm, gout = r16(fx["in"]["x"]), fx["in"].get("prompt"), r16(fx["in"]["gout"])
    n_prompt = prm.shape[0]
    w = swin_ops.weights_from_state(sd, "", heads, 64, 0, torch.device(DEV), need_bwd=True)
    ts = ((sd["pe.weights_token"] @ sd["pe.enc_token.0"].t())[:, :n_prompt] * (64 ** -0.5)).to(DEV)
    xc = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    pd = prm.to(DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    p_attn, p_proj = 0.2, 0.2

    def run(epoch_ptr, value):
        word.fill_(value)
        y, saved = swin_ops.swin_block_forward(xc, pd, w, ts, window, shift, save=True, dropout=(p_attn, p_proj, 1234, 987, epoch_ptr))
        dx, dprompt, dts = swin_ops.swin_block_backward(saved, w, pd, dy, True, True)
        d = saved.desc
        ak = torch.empty((d.B * d.P * heads, d.Nqp, d.Nkp), dtype=torch.uint8, device=DEV)
        pk = torch.empty((d.B * d.P * d.Nqp, d.C), dtype=torch.uint8, device=DEV)
        L.call("mivp_dropout_masks", C.byref(d), L.ptr(ak), L.ptr(pk), L.stream())
        torch.cuda.synchronize()
        return y.float().cpu(), dx.float().cpu(), dprompt.cpu(), ak.cpu(), pk.cpu(), d

    y_n, dx_n, dp_n, ak_n, pk_n, _ = run(None, 0)
    y_0, dx_0, dp_0, ak_0, pk_0, _ = run(word.data_ptr(), 0)
    y_5, dx_5, dp_5, ak_5, pk_5, d5 = run(word.data_ptr(), 5)
    assert torch.equal(ak_n, ak_0) and torch.equal(pk_n, pk_0) and torch.equal(y_n, y_0) and torch.equal(dx_n, dx_0)
    assert not torch.equal(ak_0, ak_5) and not torch.equal(pk_0, pk_5) and not torch.equal(y_0, y_5)
    for ak, pk in ((ak_0, pk_0), (ak_5, pk_5)):
        assert abs(1.0 - float(ak.float().mean()) - p_attn) < 0.02 and abs(1.0 - float(pk.float().mean()) - p_proj) < 0.03
    # masks of the two epochs are independent: they agree about as often as independent draws would (keep^2 + drop^2)
    agree = float((ak_0 == ak_5).float().mean())
    assert abs(agree - ((1 - p_attn) ** 2 + p_attn ** 2)) < 0.02, agree
    # forward / backward under epoch 5 against the oracle with THOSE masks
    B, P, Nq, Nqp, Nkp, Cc = d5.B, d5.P, d5.Nq, d5.Nqp, d5.Nkp, d5.C
    cols = list(range(Nq)) + list(range(Nqp, Nqp + n_prompt))
    attn_keep = ak_5.view(B, P, heads, Nqp, Nkp).float()[:, :, :, :Nq][..., cols] * float(d5.attn_drop_scale)
    proj_keep = pk_5.view(B, P, Nqp, Cc)[:, :, :Nq].float() * float(d5.proj_drop_scale)
    xo = x.clone().requires_grad_(True)
    po = prm.clone().requires_grad_(True)
    want = S.swin_block(xo, po, sd, "", window, shift, heads, 64, attn_keep, proj_keep)
    want.backward(gout)
    assert rel_l2(y_5.permute(0, 4, 1, 2, 3), want.detach()) < 6e-3
    assert rel_l2(dx_5.permute(0, 4, 1, 2, 3), xo.grad) < 1.5e-2
    assert rel_l2(dp_5, po.grad) < 1.5e-2


@pytest.mark.parametrize("tag", ["even_T", "odd_T", "even_F", "odd_F"])
def test_patch_merge_backward_golden(tag):
    import mivp_amd
    from mivp_amd import ops
    from oracle import swin_ref as S
    fx = load_fixture(f"merge_{tag}")
    sd = _rounded_state(fx["sd"])
    x = r16(fx["in"]["x"]).requires_grad_(True)
    want = S.patch_merge(x, sd, "", fx.meta["merge_last_dim"])
    g = r16(fx["in"]["gout"])
    want.backward(g)
    xc = x.detach().permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    dy = g.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    w = sd["reduction.weight"]
    dx = ops.patch_merge_backward(dy, xc, sd["norm.weight"].to(DEV), sd["norm.bias"].to(DEV),
                                  w.t().contiguous().to(DEV, torch.bfloat16), fx.meta["merge_last_dim"])
    torch.cuda.synchronize()
    assert rel_l2(dx.float().cpu().permute(0, 4, 1, 2, 3), x.grad) < 1e-2


@pytest.mark.parametrize("C,dims,last", [(48, (8, 8, 8), True), (192, (4, 6, 5), False)])
def test_patch_merge_backward_real_channels(C, dims, last):
    import mivp_amd
    from mivp_amd import ops
    from oracle import swin_ref as S
    g = torch.Generator().manual_seed(C)
    k = 8 if last else 4
    sd = {"norm.weight": (1 + 0.2 * torch.randn(k * C, generator=g)).requires_grad_(True),
          "norm.bias": (0.1 * torch.randn(k * C, generator=g)).requires_grad_(True),
          "reduction.weight": r16(torch.randn(2 * C, k * C, generator=g) / (k * C) ** 0.5).requires_grad_(True)}
    x = r16(torch.randn(2, C, *dims, generator=g)).requires_grad_(True)
    want = S.patch_merge(x, sd, "", last)
    gout = r16(torch.randn(want.shape, generator=g))
    want.backward(gout)
    xc = x.detach().permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    w_t = sd["reduction.weight"].detach().t().contiguous().to(DEV, torch.bfloat16)
    ln_w, ln_b = sd["norm.weight"].detach().to(DEV), sd["norm.bias"].detach().to(DEV)
    dx = ops.patch_merge_backward(dy, xc, ln_w, ln_b, w_t, last)
    torch.cuda.synchronize()
    assert rel_l2(dx.float().cpu().permute(0, 4, 1, 2, 3), x.grad) < 1e-2
    # weight-gradient mode: same dx, plus the parameters' gradients (bf16 operands, fp32 sums: 6e-3)
    dx2, dw, dgamma, dbeta = ops.patch_merge_backward(dy, xc, ln_w, ln_b, w_t, last, need_w=True)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx)
    assert rel_l2(dw.cpu(), sd["reduction.weight"].grad) < 6e-3
    assert rel_l2(dgamma.cpu(), sd["norm.weight"].grad) < 6e-3
    assert rel_l2(dbeta.cpu(), sd["norm.bias"].grad) < 6e-3


@pytest.mark.parametrize("window,dims,C,heads,n_prompt,shift,dropout", [
    ((7, 7, 7), (14, 14, 14), 48, 4, 64, (3, 3, 3), None),            # cut and uncut windows, prompts (26 key tiles)
    ((7, 7, 7), (14, 14, 14), 48, 4, 0, (0, 0, 0), None),             # decoder stage 2: no prompts (22 key tiles)
    ((7, 7, 7), (12, 12, 24), 96, 8, 64, (3, 3, 3), None),
    ((7, 7, 7), (6, 6, 24), 192, 16, 64, (3, 3, 3), (0.1, 0.1, 123, 456)),
    ((8, 8, 4), (16, 16, 8), 48, 4, 64, (4, 4, 2), None),             # 256-token windows: 20 key tiles
    ((5, 5, 3), (10, 10, 6), 48, 4, 16, (2, 2, 1), None),             # 75 queries -> 5 query tiles: the phantom sixth tile
    ((3, 3, 2), (6, 6, 4), 16, 4, 8, (1, 1, 1), (0.2, 0.0, 9, 10)),   # head_dim 4, tiny windows
])
def test_one_pass_backward_equals_two_pass(window, dims, C, heads, n_prompt, shift, dropout):
    """csrc/swin_bwd_fused.hip against the dq-owner + dkv-owner pair it replaces (swin_bwd.hip), same inputs: both form the
    same products with fp32 accumulation and round dS / P to bf16 at the same points, so dq / dk / dv (through dx) and the
    prompt gradients agree to summation-order noise -- a wrong tile, lane map or mask would be an O(1) difference."""
    import mivp_amd
    from mivp_amd import swin_ops
    from oracle.unetr_ref import _block_state
    gen = torch.Generator().manual_seed(3)
    sd = {}
    _block_state(sd, "", C, heads, list(window), 64, max(n_prompt, 1), n_prompt > 0, gen)
    sd = _rounded_state(sd)
    x = r16(torch.randn(2, C, *dims, generator=gen))
    prm = 0.5 * torch.randn(n_prompt, C, generator=gen) if n_prompt else None
    gout = r16(torch.randn(2, C, *dims, generator=gen))
    w = swin_ops.weights_from_state(sd, "", heads, 64, n_prompt, torch.device(DEV), need_bwd=True)
    xc = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    pd = None if prm is None else prm.to(DEV)
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    res = []
    for fused in (True, False):
        swin_ops.USE_FUSED_ATTN_BWD = fused
        try:
            y, saved = swin_ops.swin_block_forward(xc, pd, w, None, window, shift, save=True, dropout=dropout)
            if fused:
                import ctypes
                from mivp_amd import _lib as L
                assert L.lib().mivp_win_attn_bwd_fused_supported(ctypes.byref(saved.desc)) == 1
            res.append(swin_ops.swin_block_backward(saved, w, pd, dy, True, n_prompt > 0))
        finally:
            swin_ops.USE_FUSED_ATTN_BWD = True
    torch.cuda.synchronize()
    (dx1, dp1, dt1), (dx2, dp2, dt2) = res
    assert torch.isfinite(dx1.float()).all()
    e = rel_l2(dx1.float().cpu(), dx2.float().cpu())
    assert e < 2.5e-3, ("dx", e)                                # two bf16 roundings of nearly equal f32 values
    if n_prompt:
        assert rel_l2(dp1.cpu(), dp2.cpu()) < 1e-3 and rel_l2(dt1.cpu(), dt2.cpu()) < 1e-3, \
            (rel_l2(dp1.cpu(), dp2.cpu()), rel_l2(dt1.cpu(), dt2.cpu()))


@pytest.mark.parametrize("window,dims,C,heads,n_prompt,shift,dropout", [
    ((7, 7, 7), (24, 24, 24), 48, 4, 64, (0, 0, 0), None),            # cfg2's first prompted block (padded windows)
    ((7, 7, 7), (14, 14, 14), 48, 4, 64, (3, 3, 3), (0.1, 0.0, 5, 6)),
    ((4, 4, 4), (8, 8, 8), 32, 2, 16, (0, 0, 0), None),               # one prompt tile: eight query parts
    ((5, 5, 3), (10, 10, 6), 48, 4, 30, (2, 2, 1), None),             # 30 prompts -> two prompt tiles, the second ragged
])
def test_prompt_only_backward_equals_two_pass(window, dims, C, heads, n_prompt, shift, dropout):
    """mivp_win_attn_bwd_prompt (first prompted block behind a frozen stem: need_dx False) against mivp_win_attn_delta + the
    prompt-only mode of mivp_win_attn_bwd_dkv: same products, same bf16 rounding points of dS / P."""
    import ctypes
    import mivp_amd
    from mivp_amd import swin_ops, _lib as L
    from oracle.unetr_ref import _block_state
    gen = torch.Generator().manual_seed(4)
    sd = {}
    _block_state(sd, "", C, heads, list(window), 64, n_prompt, True, gen)
    sd = _rounded_state(sd)
    x = r16(torch.randn(2, C, *dims, generator=gen))
    prm = 0.5 * torch.randn(n_prompt, C, generator=gen)
    gout = r16(torch.randn(2, C, *dims, generator=gen))
    w = swin_ops.weights_from_state(sd, "", heads, 64, n_prompt, torch.device(DEV), need_bwd=True)
    xc = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    pd = prm.to(DEV)
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)
    res = []
    for fused in (True, False):
        swin_ops.USE_FUSED_ATTN_BWD = fused
        try:
            y, saved = swin_ops.swin_block_forward(xc, pd, w, None, window, shift, save=True, dropout=dropout)
            if fused:
                assert L.lib().mivp_win_attn_bwd_prompt_supported(ctypes.byref(saved.desc)) == 1
            res.append(swin_ops.swin_block_backward(saved, w, pd, dy, False, True))
        finally:
            swin_ops.USE_FUSED_ATTN_BWD = True
    torch.cuda.synchronize()
    (dx1, dp1, dt1), (dx2, dp2, dt2) = res
    assert dx1 is None and dx2 is None
    assert torch.isfinite(dp1).all() and torch.isfinite(dt1).all()
    assert rel_l2(dp1.cpu(), dp2.cpu()) < 1e-3 and rel_l2(dt1.cpu(), dt2.cpu()) < 1e-3, \
        (rel_l2(dp1.cpu(), dp2.cpu()), rel_l2(dt1.cpu(), dt2.cpu()))
