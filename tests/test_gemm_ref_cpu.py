"""tests/gemm_ref.py against torch in fp64, its yardsticks, and how far a wrong kernel would sit from it.

reference() restates include/vqa_hip.h; here it must equal F.linear / torch.bmm / F.conv2d / the autograd
weight gradient of F.conv2d / F.gelu / tanh to 1e-12 of the normaliser, so the GPU parity test compares
the kernels with what torch computes in fp64 and not with a private formula.

test_mistakes_are_visible: each of the 25 deliberate mistakes of gemm_ref.MISTAKES, applied to model(),
must exceed its group's bound by at least 2x on a case of the GPU tables.  Least ratio measured: 257
(gelu_tanh: the tanh form of GELU differs from the erf form by up to 4.7e-4); then scale_batch at 1.9e3 (an
e4m3 scale not moved by its batch stride) and c16_trunc at 5.2e3 (a truncating bf16 store); every other
mistake sits more than 6e4 bounds away, and a read through the wrong pitch or stride lands in NaN padding.
Nothing here runs a kernel."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as gr

TOL = 1e-12


def _rel(got, c, key="c32"):
    return float((np.abs(got - gr.reference(c)[key]) / gr.normaliser(c)).max())


def _plain_epilogue(c, I, z, prod):
    """The epilogue from torch ops, for cases without mask / dropout."""
    v = c.alpha * prod
    if c.bias:
        v = v + I.bias[I.bias_off + z * I.stride_bias:][:c.n].double()
    for r in (I.res32 if c.res32 else None, I.res16 if c.res16 else None):
        if r is not None:
            v = v + torch.as_strided(r, (c.m, c.n), (I.ldres, 1), z * I.stride_res).double()
    if c.act:
        v = (torch.relu, F.gelu, torch.tanh)[c.act - 1](v)
    return v + c.beta * I.old[z].double() if c.beta else v


def _ab(c, I, z):
    a = torch.as_strided(I.a, (c.k, c.m) if c.at else (c.m, c.k), (I.lda, 1), z * I.stride_a).double()
    b = torch.as_strided(I.b, (c.k, c.n) if c.bt else (c.n, c.k), (I.ldb, 1), z * I.stride_b).double()
    return (a.T if c.at else a), (b.T if c.bt else b)          # A [m, k], W [n, k]


PLAIN = [c for c in gr.table("plain") + gr.EXT if not (c.mask or c.p)]


def test_reference_equals_linear_and_bmm():
    seen = set()
    for c in PLAIN:
        key = (c.at, c.bt, c.m, c.n, c.k > 64, c.bias, c.res32, c.res16, c.act, c.beta, c.batch)
        if key in seen:
            continue
        seen.add(key)
        I = gr.build(c)
        if c.batch > 1:
            A, W = zip(*[_ab(c, I, z) for z in range(c.batch)])
            prod = torch.bmm(torch.stack(A), torch.stack(W).transpose(1, 2))
        else:
            A, W = _ab(c, I, 0)
            prod = F.linear(A, W)[None]
        got = torch.stack([_plain_epilogue(c, I, z, prod[z]) for z in range(c.batch)]).numpy()
        assert _rel(got, c) <= TOL, gr.name(c)
    assert len(seen) > 40 and {2, 3} <= {k[8] for k in seen}  # GELU and tanh among them


def _nchw(c, I, which):
    g = c.geom
    return (I.a if which == "a" else I.b)[:g[0] * g[1] * g[2] * g[3]].double().view(g[0], g[1], g[2], g[3]).permute(0, 3, 1, 2)


@pytest.mark.parametrize("c", gr.CONV + gr.PATCH, ids=gr.name)
def test_reference_equals_conv2d(c):
    I, g = gr.build(c), c.geom
    w = torch.as_strided(I.b, (c.n, c.k), (I.ldb, 1)).double()
    if c.conv == 2:                                             # [Cout][C/64][3][3][64] -> [Cout][C][3][3]
        w = w.view(c.n, g[3] // 64, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(c.n, g[3], 3, 3)
    else:                                                       # [Cout][kh][kw][C]
        w = w.view(c.n, g[6], g[7], g[3]).permute(0, 3, 1, 2)
    y = F.conv2d(_nchw(c, I, "a"), w, stride=g[8], padding=g[9])
    assert y.shape[2:] == (g[4], g[5])
    got = _plain_epilogue(c, I, 0, y.permute(0, 2, 3, 1).reshape(c.m, c.n)).numpy()[None]
    assert _rel(got, c) <= TOL


@pytest.mark.parametrize("c", gr.BCONV + tuple(s for s in gr.SPLITK if s.bconv and s.splitk == 2), ids=gr.name)
def test_reference_equals_conv2d_weight_gradient(c):
    """b_conv: dW[co, (kh, kw, c)] = sum over the output pixels of dY x the input under the tap."""
    I, g = gr.build(c), c.geom
    for z in range(c.batch):
        x = I.b[z * I.stride_b:][:g[0] * g[1] * g[2] * g[3]].double().view(g[0], g[1], g[2], g[3]).permute(0, 3, 1, 2)
        dy = torch.as_strided(I.a, (c.k, c.m), (I.lda, 1), z * I.stride_a).double()          # [(img, oh, ow), co]
        w = torch.zeros(c.m, g[3], g[6], g[7], dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, w, stride=g[8], padding=g[9])
        y.backward(dy.view(g[0], g[4], g[5], c.m).permute(0, 3, 1, 2))
        dw = w.grad.permute(0, 2, 3, 1).reshape(c.m, c.n)
        A, B, _, _ = gr.operands(c, I, z)
        assert float((np.abs(A @ B - dw.numpy()) / (np.abs(A) @ np.abs(B) + 1e-300)).max()) <= TOL


def test_reference_masked_dropout_epilogue_by_hand():
    """mask and dropout from the documented law, element by element on a few rows: k = [mask > 0] *
    multiplier of element (z*m + row)*n + col, or row*n + col at site + z*drop_site_stride."""
    from oracle import vqa_oracle as orc
    for c in gr.BATCH[:2] + (gr.EPI[11],):
        I, ref = gr.build(c), gr.reference(c)
        for z in range(c.batch):
            A, W = _ab(c, I, z)
            for row in (0, c.m // 2, c.m - 1):
                for col in (0, 1, c.n - 1):
                    e = (row * c.n + col) if c.dsite else ((z * c.m + row) * c.n + col)
                    kf = float(orc.dropout_multiplier_np(c.p, gr.SEED, gr.COUNTER, gr.SITE + z * c.dsite, e + 1)[e])
                    if c.mask:
                        kf *= float(I.mask16[z * I.stride_res + row * I.ldmask + col] > 0)
                    v = c.alpha * float(A[row] @ W[col])
                    v += float(I.bias[z * I.stride_bias + col]) if c.bias else 0.0
                    v *= kf
                    v += float(I.res32[z * I.stride_res + row * I.ldres + col]) if c.res32 else 0.0
                    v += float(I.res16[z * I.stride_res + row * I.ldres + col]) if c.res16 else 0.0
                    v += c.beta * float(I.old[z, row, col]) if c.beta else 0.0
                    assert abs(v - ref["c32"][z, row, col]) <= 1e-11 * gr.normaliser(c)[z, row, col]


def test_reference_fp8_equals_dequantised_linear():
    for c in gr.FP8:
        I = gr.build(c)
        for z in range(c.batch):
            a = torch.as_strided(I.a, (c.m, c.k), (I.lda, 1), z * I.stride_a).view(torch.float8_e4m3fn).double()
            b = torch.as_strided(I.b, (c.n, c.k), (I.ldb, 1), z * I.stride_b).view(torch.float8_e4m3fn).double()
            a = a * I.scale_a[z * I.stride_scale_a:][:c.m].double()[:, None]
            b = b * I.scale_b[z * I.stride_scale_b:][:c.n].double()[:, None]
            got = _plain_epilogue(c, I, z, F.linear(a, b)).numpy()
            assert float((np.abs(got - gr.reference(c)["c32"][z]) / gr.normaliser(c)[z]).max()) <= TOL
            # the quantised rows decode to within e4m3's half ulp (2^-4) of their source
            assert float(((a - I.src_a[z].double()).abs() / I.src_a[z].double().abs().amax(1, keepdim=True)).max()) <= 2.0 ** -4


def test_tables_hold_what_the_checks_need():
    """Padding is NaN, the pitches differ, masks contain +0, -0 and negatives, every path is in a table."""
    for g in gr.GROUPS:
        for c in gr.table(g):
            I = gr.build(c)
            assert len({I.ldres, I.ldmask, I.ldc32, I.ldc16}) == 4 and min(I.ldres, I.ldmask, I.ldc32, I.ldc16) > c.n
            if not (c.conv or c.fp8):
                assert I.lda > (c.m if c.at else c.k) and bool(torch.isnan(I.a.float()).any())
            if not (c.bconv or c.fp8):
                assert I.ldb > (c.n if c.bt else c.k) and bool(torch.isnan(I.b.float()).any())
            if c.mask:
                mk = torch.as_strided(I.mask16, (c.m, c.n), (I.ldmask, 1))
                bits = mk.view(torch.int16)
                assert bool((bits == 0).any()) and bool((bits == -32768).any()) and bool((mk < 0).any())
                assert bool(torch.isnan(I.mask16.float()).any())
            assert gr.vec(c) == (c.n % 8 == 0 and not c.scalar)
    cf = [(c.geom[3] % 64 == 0, c.geom[3] * c.geom[7] == 64) for c in gr.CONV]
    assert sum(a for a, _ in cf) >= 3 and sum(b for _, b in cf) >= 3 and sum(not a and not b for a, b in cf) >= 4
    assert any(c.geom[1] != c.geom[2] for c in gr.CONV) and any(c.geom[6] != c.geom[7] for c in gr.CONV)
    assert any(len(gr.slices(c)) == 3 and c.splitk == 5 for c in gr.SPLITK)               # splitk > the k-tiles
    assert any(len(gr.slices(c)) == 1 for c in gr.SPLITK)                                  # one k-tile: no split


def test_yardsticks_are_of_rounding_size():
    for g in gr.GROUPS:
        y = gr.yardstick(g)
        print(g, f"yardstick {y:.3e} bound {gr.bound(g):.3e}")
        # fp32 rounding, 2^-24, times a few; e4m3: the MFMA cuts products 2^-13 below their group's largest
        assert 2.0 ** -26 < y < (2.0 ** -13 if g == "fp8" else 2.0 ** -21), (g, y)
        assert gr.bound(g) == max(4 * y, 2.0 ** -22)
    # the fp32 restatements of the activations alone, |v| <= 8
    v = np.linspace(-8, 8, 200001)
    gelu = 0.5 * v * (1 + torch.erf(torch.from_numpy(v / math.sqrt(2))).numpy())
    assert np.abs(gr._act(v.astype(np.float32), 2, np.float32, None) - gelu).max() < 7e-7
    assert np.abs(gr._act(v.astype(np.float32), 3, np.float32, None) - np.tanh(v)).max() < 1.3e-7


def _candidates(mistake):
    """Up to four cases per group that the mistake can show on, smallest first."""
    out = []
    for g in gr.GROUPS:
        cs = sorted((c for c in gr.table(g) if gr.MISTAKES[mistake](c)), key=lambda c: c.m * c.n * c.k * c.batch)
        out += cs[:4]
    return out


@pytest.mark.parametrize("mistake", sorted(gr.MISTAKES))
def test_mistakes_are_visible(mistake):
    cs = _candidates(mistake)
    assert cs, mistake
    best = max(gr.error(c, gr.model(c, wrong=mistake)) / gr.bound(c.group) for c in cs)
    print(mistake, f"{best:.3g} bounds")
    assert best >= 2.0, (mistake, best)


def test_model_without_a_mistake_is_within_every_bound():
    for g in gr.GROUPS:
        for c in gr.table(g)[:6]:
            assert gr.error(c, gr.model(c)) <= gr.yardstick(g)


def test_fdiv_is_exact_below_2_24():
    """gemm_common.h fdiv (the b_conv loader's split of k into image / row / column) in numpy float32
    against //: every a < 2^24 for every divisor oh*ow and ow the tables and the engines use."""
    divs = sorted({d for oh, ow in gr.FDIV_MAPS for d in (oh * ow, ow)})
    for lo in range(0, 1 << 24, 1 << 22):
        a = np.arange(lo, lo + (1 << 22), dtype=np.int64)
        for d in divs:
            assert np.array_equal(gr.fdiv(a, d), a // d), d
