"""tests/norm_ref.py is the fp64 reference of tests/test_norm_reduce_gpu.py.  Here, on the CPU:
it equals torch.autograd of the two norms; the fp32 yardstick it defines is of rounding size; and
every mistake a kernel could plausibly make moves the reference at least 100 times further than the
bound the GPU test allows (4 x yardstick), so that bound separates right from wrong without a wrong
kernel ever being run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as nr
from oracle import vqa_oracle as orc

SEED, COUNTER = 9, 2
NORM_BWD_ROWS = 8            # rows per block of the backward kernels today (the GPU test reads it)


def _mult(p, site, rows, D, width=None):
    """Multipliers [rows, D] of a site; width != D: the mask a kernel with the wrong row pitch
    `width` would apply (element row * width + col)."""
    width = width or D
    flat = torch.from_numpy(orc.dropout_multiplier(p, SEED, COUNTER, site, rows * width + D))
    idx = torch.arange(rows)[:, None] * width + torch.arange(D)[None, :]
    return flat[idx]


@pytest.mark.parametrize("D", nr.WIDTHS)
@pytest.mark.parametrize("dres", [False, True])
def test_reference_equals_autograd_in_fp64(D, dres):
    rows = 37
    c = {k: v.double() for k, v in nr.make_inputs(D, rows).items()}
    m_dy, m32, m16 = (_mult(0.1, s, rows, D).double() for s in (40, 41, 42))
    dr = c["dres"] if dres else None
    # RMSNorm: out = drop_dy(w * x * rsqrt(mean(x^2) + eps)); the masks on dx as multiplications
    x, w = c["x"].clone().requires_grad_(True), c["w"].clone().requires_grad_(True)
    y = w * x * torch.rsqrt((x * x).mean(-1, keepdim=True) + nr.RMS_EPS) * m_dy
    y.backward(c["dy"])
    full = x.grad if dr is None else x.grad + dr
    dx32, dx16, dw = nr.rms_bwd(c["x"], nr.rms_stats(c["x"]), c["w"], c["dy"], dr, m_dy, m32, m16)
    for got, want in ((dx32, full * m32), (dx16, full * m16), (dw, w.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # LayerNorm: dres only in dx32, the mask only on the branch gradient
    x, g, b = (c[k].clone().requires_grad_(True) for k in ("x", "w", "b"))
    F.layer_norm(x, (D,), g, b, nr.LN_EPS).backward(c["dy"])
    mean, rstd = nr.ln_stats(c["x"])
    dx32, dx16, dg, db, ds = nr.ln_bwd(c["x"], mean, rstd, c["w"], c["dy"], dr, m16)
    for got, want in ((dx32, x.grad if dr is None else x.grad + dr), (dx16, x.grad * m16), (dg, g.grad),
                      (db, b.grad), (ds, (x.grad * m16).sum(0))):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_yardstick_is_of_rounding_size():
    y = nr.yardstick()
    print("yardstick", y, "bounds", nr.bound("dx"), nr.bound("colsum"))
    # a handful of fp32 roundings: above the floor, far below anything a formula error gives
    for kind in ("dx", "colsum"):
        assert 2.0 ** -26 <= y[kind] <= 2.0 ** -20, (kind, y[kind])
        assert nr.bound(kind) == max(4 * y[kind], 2.0 ** -22)


def _mutant_effects(D, rows):
    """{mutant: (kind, effect)}: how far each wrong variant moves its output from the fp64
    reference at one case, in the GPU test's own metrics."""
    c = nr.make_inputs(D, rows)
    x, w, dy, dres = c["x"], c["w"], c["dy"], c["dres"]
    rs, mu, lrs = nr.fp32_stats(c)
    m_dy, m32, m16 = (_mult(0.1, s, rows, D) for s in (40, 41, 42))
    out = {}
    r_ref = nr.rms_bwd(x, rs, w, dy, dres, m_dy, m32, m16)
    l_ref = nr.ln_bwd(x, mu, lrs, w, dy, dres, m16)
    r_plain = nr.rms_bwd(x, rs, w, dy, None, None, None, None)
    l_plain = nr.ln_bwd(x, mu, lrs, w, dy, None, None)
    r_terms = nr.rms_terms(x, rs, dy, m_dy)
    l_terms = nr.ln_terms(x, mu, lrs, w, dy, m16)

    def dx(name, got, ref):
        out[name] = ("dx", min(out.get(name, ("dx", np.inf))[1], nr.rel_rows(got, ref)))

    def cs(name, got, ref, terms):
        out[name] = ("colsum", min(out.get(name, ("colsum", np.inf))[1], nr.rel_cols(got, ref, terms)))

    for wrong in ("div+", "div-", "no_cx"):
        if wrong == "div-" and D == 256:
            continue                                       # a zero divisor: not a quiet mistake
        dx("rms " + wrong, nr.rms_bwd(x, rs, w, dy, None, None, None, None, wrong=wrong)[0], r_plain[0])
        dx("ln " + wrong, nr.ln_bwd(x, mu, lrs, w, dy, None, None, wrong=wrong)[0], l_plain[0])
    if rows > 1:
        nxt = lambda t: torch.roll(t, -1)
        dx("rms rstd of next row", nr.rms_bwd(x, nxt(rs), w, dy, None, None, None, None)[0], r_plain[0])
        dx("ln rstd of next row", nr.ln_bwd(x, mu, nxt(lrs), w, dy, None, None)[0], l_plain[0])
    # column sums that lose their last row, or their last block of rows
    for name, keep in (("last row missing", rows - 1), ("last block missing", (rows - 1) // NORM_BWD_ROWS * NORM_BWD_ROWS)):
        cs("rms dw " + name, r_terms[:keep].sum(0), r_ref[2], r_terms)
        for k, kn in enumerate(("dgamma", "dbeta", "dsum")):
            summands = l_ref[1] if kn == "dsum" else l_terms[k]      # dsum sums the masked branch gradient
            cs(f"ln {kn} {name}", summands[:keep].sum(0), l_ref[2 + k], l_terms[k])
    if D != 768 and rows > 1:
        b_dy, b32, b16 = (_mult(0.1, s, rows, D, width=768) for s in (40, 41, 42))
        dx("rms dx32 mask pitch 768", nr.rms_bwd(x, rs, w, dy, dres, m_dy, b32, m16)[0], r_ref[0])
        dx("rms dx16 mask pitch 768", nr.rms_bwd(x, rs, w, dy, dres, m_dy, m32, b16)[1], r_ref[1])
        dx("rms dy mask pitch 768", nr.rms_bwd(x, rs, w, dy, dres, b_dy, m32, m16)[0], r_ref[0])
        cs("rms dw dy mask pitch 768", nr.rms_bwd(x, rs, w, dy, dres, b_dy, m32, m16)[2], r_ref[2], r_terms)
        bad = nr.ln_bwd(x, mu, lrs, w, dy, dres, b16)
        dx("ln dx16 mask pitch 768", bad[1], l_ref[1])
        cs("ln dsum mask pitch 768", bad[4], l_ref[4], l_terms[2])
    swapped = nr.rms_bwd(x, rs, w, dy, dres, m_dy, m16, m32)
    dx("rms dx32 takes the dx16 mask", swapped[0], r_ref[0])
    dx("rms dx16 takes the dx32 mask", swapped[1], r_ref[1])
    bad = nr.ln_bwd(x, mu, lrs, w, dy, dres, m16, wrong="dres_in_branch")
    dx("ln dres also in dx16", bad[1], l_ref[1])
    cs("ln dres also in dsum", bad[4], l_ref[4], l_terms[2])
    return out


def test_every_mutant_sits_100_bounds_away():
    worst = {}
    for D in nr.WIDTHS:
        for rows in nr.ROWS:
            for name, (kind, eff) in _mutant_effects(D, rows).items():
                if eff < worst.get(name, (kind, np.inf, None))[1]:
                    worst[name] = (kind, eff, (D, rows))
    assert len(worst) >= 25
    for name, (kind, eff, case) in sorted(worst.items(), key=lambda kv: kv[1][1]):
        print(f"{name:34s} {kind:6s} least effect {eff:.3e} at D, rows = {case}  ({eff / nr.bound(kind):.0f} bounds)")
    for name, (kind, eff, case) in worst.items():
        assert eff >= 100 * nr.bound(kind), (name, eff, nr.bound(kind), case)


def test_integer_sums_are_exact_in_any_fp32_order():
    """The exact tests of the column reductions use integers in [-8, 8]: over the largest row
    count any of them uses (1024: the 32 x 32 pairs of the relative-position map, were they all of
    one bucket), sum |x| < 2^24, so every partial sum of every summation order is an integer fp32
    represents exactly."""
    assert 8 * 1024 < 2 ** 24
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-8, 9, (1024, 16), generator=g)
    exact = x.sum(0)
    for order in (x.float().sum(0), x.float().flip(0).cumsum(0)[-1], x.to(torch.bfloat16).float().sum(0)):
        assert torch.equal(order, exact.float())
    assert torch.equal(x.to(torch.bfloat16).long(), x)      # exact in bf16 too
