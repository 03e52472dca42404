"""CPU: the float64 references of tests/prompt_ref.py pinned against torch.autograd and against the property the bias
augmentation rests on, so that the GPU tests of test_hip_prompt_path.py compare the kernels with something checked."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_ref as R  # noqa: E402

F64 = torch.float64
WINDOWS = [(7, 7, 7), (8, 8, 4), (5, 5, 3), (3, 3, 2), (2, 3, 5)]


def _tables(g, heads, window, n_prompt):
    tabs = [torch.randn((heads, 2 * w - 1), generator=g, dtype=F64) * 0.3 for w in window]
    ts = torch.randn((heads, n_prompt), generator=g, dtype=F64) * 0.3
    return tabs, ts


def test_bf16_rne_is_the_hardware_rounding():
    g = R.gen(1)
    x = torch.randn(20000, generator=g, dtype=torch.float32) * torch.exp2(torch.randint(-20, 20, (20000,), generator=g).float())
    ties = torch.tensor([1.00390625, 1.01171875, -3.0078125, 257.0, 0.0, -0.0, 1.0, -43264.0], dtype=torch.float32)
    x = torch.cat([x, ties])                                         # f32 inputs: torch's f32 -> bf16 is one rounding too
    assert torch.equal(R.bf16_rne(x.double()), x.bfloat16().double())
    # one rounding, not two: 1 + 2^-8 + 2^-40 lies above the tie and must round up; through f32 it would fall on the tie
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=F64)
    assert float(R.bf16_rne(v)) == 1.0 + 2.0 ** -7
    assert float(R.PAD_BIAS) == float(R.bf16_rne(torch.tensor([-30000.0 * R.LOG2E], dtype=F64)))


def test_interval_rule_accepts_a_neighbour_only_across_a_boundary():
    ref = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -30, 1.25], dtype=F64)     # the first sits just below a tie
    b = torch.full_like(ref, 2.0 ** -20)
    R.assert_rounds_from_interval(torch.tensor([1.0, 1.25]).bfloat16(), ref, b)
    R.assert_rounds_from_interval(torch.tensor([1.0078125, 1.25]).bfloat16(), ref, b)
    for wrong in ([1.015625, 1.25], [1.0, 1.2578125], [float("nan"), 1.25]):
        with pytest.raises(AssertionError):
            R.assert_rounds_from_interval(torch.tensor(wrong).bfloat16(), ref, b)


@pytest.mark.parametrize("heads,n_p,e", [(4, 64, 64), (8, 30, 64), (2, 1, 5), (3, 7, 33)])
def test_token_score_adjoints_against_autograd(heads, n_p, e):
    g = R.gen(heads * 1000 + n_p)
    W = torch.randn((heads, e), generator=g, dtype=F64).requires_grad_(True)
    E = torch.randn((n_p, e), generator=g, dtype=F64).requires_grad_(True)
    dts = torch.randn((heads, n_p), generator=g, dtype=F64)
    scale = e ** -0.5
    ts = R.token_scores(W, E, scale)
    assert ts.shape == (heads, n_p)
    Wl, El = W.detach().tolist(), E.detach().tolist()
    for h in range(heads):
        for t in range(0, n_p, max(1, n_p // 3)):
            assert float(ts[h, t].detach()) == pytest.approx(scale * sum(Wl[h][k] * El[t][k] for k in range(e)), rel=1e-12)
    ts.backward(dts)
    dW, dE = R.token_scores_grads(dts, W.detach(), E.detach(), scale)
    torch.testing.assert_close(dW, W.grad, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(dE, E.grad, rtol=1e-12, atol=1e-14)
    b_ts, b_w, b_e = R.token_scores_bounds(dts, W.detach(), E.detach(), scale)
    assert b_ts.shape == ts.shape and b_w.shape == dW.shape and b_e.shape == dE.shape
    assert bool((b_ts > 0).all()) and bool((b_w > 0).all()) and bool((b_e > 0).all())


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n_prompt", [0, 5])
def test_augmentation_identity_on_every_pair(window, n_prompt):
    """<qa[n], ka[h][m]> / log2(e) == T_h[k0-i0+w0-1] + T_w[..] + T_d[..] for every valid (query, key) pair, un-rounded."""
    heads = 3
    (t_h, t_w, t_d), ts = _tables(R.gen(sum(window) + n_prompt), heads, window, n_prompt)
    d = R.aug_dims(window, n_prompt)
    qa = R.relbias_qa(window, n_prompt)
    ka, b = R.relbias_ka(t_h, t_w, t_d, ts, window, n_prompt)
    assert qa.shape == (d["Nqp"], d["augp"]) and ka.shape == (heads, d["Nkp"], d["augp"]) and b.shape == ka.shape
    # the bias itself, slot by slot from the formula (independent of relbias_full's index arithmetic)
    w0, w1, w2 = window
    want = torch.zeros((heads, d["Nq"], d["Nq"] + n_prompt), dtype=F64)
    for n in range(d["Nq"]):
        i0, i1, i2 = n // (w1 * w2), (n // w2) % w1, n % w2
        for m in range(d["Nq"]):
            k0, k1, k2 = m // (w1 * w2), (m // w2) % w1, m % w2
            want[:, n, m] = t_h[:, k0 - i0 + w0 - 1] + t_w[:, k1 - i1 + w1 - 1] + t_d[:, k2 - i2 + w2 - 1]
        want[:, n, d["Nq"]:] = ts
    full = R.relbias_full(t_h, t_w, t_d, ts, window)
    torch.testing.assert_close(full, want, rtol=0, atol=1e-15)
    got = R.bias_from_aug(qa, ka, window, n_prompt)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-14)
    # layout: pad query rows and pad columns are zero; every padding key row carries PAD_BIAS in the w0 columns only
    assert not bool(qa[d["Nq"]:].any()) and not bool(qa[:, d["aug"]:].any()) and not bool(ka[:, :, d["aug"]:].any())
    assert bool((qa[:d["Nq"], :w0].sum(1) == 1).all())               # the i0 one-hot always holds a one
    pad = torch.cat([torch.arange(d["Nq"], d["Nqp"]), torch.arange(d["Nqp"] + n_prompt, d["Nkp"])])
    assert bool((ka[:, pad, :w0] == R.PAD_BIAS).all()) and not bool(ka[:, pad, w0:].any())
    assert not bool(ka[:, d["Nqp"]:d["Nqp"] + n_prompt, w0:].any())
    assert not bool(b[:, pad].any())


@pytest.mark.parametrize("window", WINDOWS)
def test_relbias_adjoint_against_autograd(window):
    heads, n_prompt = 2, 8
    g = R.gen(7 + sum(window))
    (t_h, t_w, t_d), ts = _tables(g, heads, window, n_prompt)
    d = R.aug_dims(window, n_prompt)
    dka = torch.randn((heads, d["Nkp"], 32), generator=g, dtype=F64)
    leaves = [t.clone().requires_grad_(True) for t in (t_h, t_w, t_d)]
    val, _ = R.relbias_ka_terms(*leaves, window)                     # = ka / log2(e) on the rows and columns that count
    (val * dka[:, :d["Nq"], :d["aug"]]).sum().backward()
    got = R.relbias_grad(dka, window)
    for a, leaf in zip(got, leaves):
        torch.testing.assert_close(a, leaf.grad, rtol=1e-12, atol=1e-13)
    # the integer form used by the exact GPU test is the same function
    dki = torch.randint(-8, 9, dka.shape, generator=g)
    for a, bq in zip(R.relbias_grad(dki, window), R.relbias_grad(dki.to(F64), window)):
        assert a.dtype == torch.int64 and torch.equal(a.to(F64), bq)
    # and the gradient through the full bias agrees: d bias / d tables pulled back through qa
    leaves2 = [t.clone().requires_grad_(True) for t in (t_h, t_w, t_d)]
    full = R.relbias_full(*leaves2, None, window)                    # [heads, Nq, Nq]
    dS = torch.randn(full.shape, generator=g, dtype=F64)
    (full * dS).sum().backward()
    qa = R.relbias_qa(window)
    dka2 = torch.zeros((heads, d["Nkp"], 32), dtype=F64)
    dka2[:, :d["Nq"], :d["augp"]] = dS.transpose(1, 2) @ qa[:d["Nq"]]
    for a, leaf in zip(R.relbias_grad(dka2, window), leaves2):
        torch.testing.assert_close(a, leaf.grad, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("Cc,heads,n_p", [(16, 4, 8), (48, 4, 5), (96, 8, 3)])
def test_prompt_kv_map_and_its_gradient(Cc, heads, n_p):
    g = R.gen(Cc + n_p)
    prompt = torch.randn((n_p, Cc), generator=g, dtype=F64)
    ln_w = 1.0 + 0.2 * torch.randn(Cc, generator=g, dtype=F64)
    ln_b = 0.1 * torch.randn(Cc, generator=g, dtype=F64)
    wqkv = R.bf16_rne(torch.randn((3 * Cc, Cc), generator=g, dtype=F64) * Cc ** -0.5)
    Npp, eps, hd = R.round_up(n_p, 16), 1e-6, Cc // heads
    yln, kp, vp, bk, bv = R.prompt_kv(prompt, ln_w, ln_b, wqkv, heads, Npp, eps)
    torch.testing.assert_close(yln, torch.nn.functional.layer_norm(prompt, (Cc,), ln_w, ln_b, eps), rtol=1e-12, atol=1e-13)
    assert kp.shape == vp.shape == bk.shape == bv.shape == (heads, Npp, hd)
    assert not bool(kp[:, n_p:].any()) and not bool(vp[:, n_p:].any())
    y16 = yln.float().bfloat16().double()
    for (h, t, j) in [(0, 0, 0), (heads - 1, n_p - 1, hd - 1), (1, n_p // 2, 1)]:
        assert float(kp[h, t, j]) == pytest.approx(R.LOG2E * float(y16[t] @ wqkv[Cc + h * hd + j]), rel=1e-12)
        assert float(vp[h, t, j]) == pytest.approx(float(y16[t] @ wqkv[2 * Cc + h * hd + j]), rel=1e-12)
    assert bool((kp.abs() <= bk / (Cc * R.U32) + 1e-300).all())      # b is C u times the absolute-value form
    # head split / merge are inverse relayouts
    rows = torch.randn((n_p, Cc), generator=g, dtype=F64)
    assert torch.equal(R.head_merge(R.head_split(rows, heads, Npp), n_p), rows)
    # gradient against autograd of the smooth map with SHARED gamma / beta: the per-row terms must sum to it
    dkp = torch.randn((heads, Npp, hd), generator=g, dtype=F64)
    dvp = torch.randn((heads, Npp, hd), generator=g, dtype=F64)
    p = prompt.clone().requires_grad_(True)
    gam, bet = ln_w.clone().requires_grad_(True), ln_b.clone().requires_grad_(True)
    K, V = R.prompt_kv_smooth(p, gam, bet, wqkv, heads, eps)
    ((dkp[:, :n_p] * K).sum() + (dvp[:, :n_p] * V).sum()).backward()
    dprompt, wg_ln = R.prompt_kv_bwd(dkp, dvp, prompt, ln_w, ln_b, wqkv, heads, eps)
    torch.testing.assert_close(dprompt, p.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(wg_ln[0].sum(0), bet.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(wg_ln[1].sum(0), gam.grad, rtol=1e-11, atol=1e-13)
    # the closed forms the header states: dbeta row = dK Wk + dV Wv, dgamma row = that times the normalised row
    dy = R.head_merge(dkp, n_p) @ wqkv[Cc:2 * Cc] + R.head_merge(dvp, n_p) @ wqkv[2 * Cc:]
    xh = (yln - ln_b) / ln_w
    torch.testing.assert_close(wg_ln[0], dy, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(wg_ln[1], dy * xh, rtol=1e-10, atol=1e-12)
    # the f32 evaluation is the same function at lower precision
    d32, w32 = R.prompt_kv_bwd(dkp, dvp, prompt, ln_w, ln_b, wqkv, heads, eps, dtype=torch.float32)
    assert d32.dtype == torch.float32 and 0 < R.rel_max_err(d32, dprompt) < 1e-4 and R.rel_max_err(w32, wg_ln) < 1e-4


def test_reduce_rows_references():
    g = R.gen(3)
    x = R.draw(g, (65, 33), range(-2047, 2048))
    s, a = R.reduce_rows_int(x)
    assert s.dtype == torch.int64 and torch.equal(s.to(F64), x.sum(0)) and bool((a.to(F64) == x.abs().sum(0)).all())
    assert int(a.max()) < 2 ** 24
    r, b = R.reduce_rows_bound(x)
    assert torch.equal(r, x.sum(0)) and bool((b == 64 * R.U32 * x.abs().sum(0)).all())
    z, bz = R.reduce_rows_bound(torch.zeros((0, 5), dtype=F64))
    assert not bool(z.any()) and not bool(bz.any())
