"""Plain torch restatement of the row-norm backward kernels (csrc/norms.hip), written from the
formulas of include/vqa_hip.h and not from autograd.  Every function takes a dtype: float64 gives
the reference of tests/test_norm_reduce_gpu.py, float32 the yardstick (what a different but
equally long fp32 evaluation of the same formulas loses against fp64).

The statistics (rstd, mean) are ARGUMENTS: the backward's contract is "given rstd / mean", so the
GPU test passes the forward kernel's own fp32 values and a wrong forward can neither hide in the
backward's error nor be blamed on it.  rms_stats / ln_stats give them in any dtype.

Masks are multiplier tensors [rows, D] (oracle.vqa_oracle.dropout_multiplier over rows * D
elements, element row * D + col), None = no dropout.

`wrong=` applies one deliberate mistake to the formula; tests/test_norm_ref_cpu.py measures with
it how far a wrong kernel would sit from the reference (no wrong kernel is ever run)."""
import functools

import torch

WIDTHS = (256, 512, 768, 1024)                 # the four NV instantiations of the backward kernels
ROWS = (1, 5, 13, 37, 136, 264)                # tests/test_norm_reduce_gpu.py says why these
RMS_EPS, LN_EPS = 1e-6, 1e-5
FLOOR = 2.0 ** -22                             # no bound is below a quarter ulp of the normaliser
FACTOR = 4.0                                   # bound = FACTOR * yardstick (test_norm_reduce_gpu.py)


def _c(t, dtype):
    return None if t is None else t.to(dtype)


def make_inputs(D, rows, seed=0):
    """fp32 CPU inputs of one case: x = 2 randn + 0.5 with one row scaled by 1/1024 (eps matters
    there) and one by 64, gains 1 + 0.1 randn, a bias, dy and dres randn."""
    g = torch.Generator().manual_seed(10007 * seed + 31 * D + rows)
    x = 2 * torch.randn(rows, D, generator=g) + 0.5
    x[rows // 3] *= 1.0 / 1024
    x[(2 * rows) // 3] *= 64.0
    w = 1 + 0.1 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    dres = torch.randn(rows, D, generator=g)
    return dict(x=x, w=w, b=b, dy=dy, dres=dres)


def rms_stats(x, eps=RMS_EPS, dtype=torch.float64):
    x = x.to(dtype)
    return torch.rsqrt((x * x).mean(-1) + eps)


def ln_stats(x, eps=LN_EPS, dtype=torch.float64):
    x = x.to(dtype)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean, torch.rsqrt(var + eps)


def rms_terms(x, rstd, dy, m_dy, dtype=torch.float64):
    """[rows, D] summands of dw: (masked dy) * x * rstd."""
    x, rstd, dy, m_dy = (_c(t, dtype) for t in (x, rstd, dy, m_dy))
    d = dy if m_dy is None else dy * m_dy
    return d * x * rstd[:, None]


def rms_bwd(x, rstd, w, dy, dres, m_dy, m_dx32, m_dx16, dtype=torch.float64, wrong=None):
    """T5LayerNorm backward: y = w * x * rstd.  Returns (dx32, the value dx16 rounds, dw).
    g = w * drop_dy(dy);  dx = rstd * g - rstd^3 / D * x * sum(g * x)  (+ dres, in BOTH outputs);
    each output times its own mask;  dw = column sums of drop_dy(dy) * x * rstd."""
    x, rstd, w, dy, dres, m_dy, m_dx32, m_dx16 = (_c(t, dtype) for t in (x, rstd, w, dy, dres, m_dy, m_dx32, m_dx16))
    D = x.shape[1]
    div = {"div+": D + 256, "div-": D - 256}.get(wrong, D)
    d = dy if m_dy is None else dy * m_dy
    g = w * d
    r = rstd[:, None]
    c = r * r * r * (g * x).sum(-1, keepdim=True) / div
    full = r * g if wrong == "no_cx" else r * g - c * x
    if dres is not None:
        full = full + dres
    dx32 = full if m_dx32 is None else full * m_dx32
    dx16 = full if m_dx16 is None else full * m_dx16
    return dx32, dx16, (d * x * r).sum(0)


def ln_terms(x, mean, rstd, gamma, dy, m_dx16, dtype=torch.float64):
    """[rows, D] summands of dgamma and dbeta, and the magnitudes behind dsum's summands.  A dsum
    summand is itself a computed difference rstd * (g - mean(g) - xh * mean(g * xh)) that can
    cancel to nearly nothing while carrying the rounding of its three parts, so a column's
    normaliser sums |rstd g| + |rstd mean(g)| + |rstd xh mean(g xh)| (times the mask), not the
    |difference|: at one row the latter would ask a cancelled element for full relative accuracy."""
    x, mean, rstd, gamma, dy, m_dx16 = (_c(t, dtype) for t in (x, mean, rstd, gamma, dy, m_dx16))
    D = x.shape[1]
    r = rstd[:, None]
    xh = (x - mean[:, None]) * r
    g = gamma * dy
    s1, s2 = g.sum(-1, keepdim=True) / D, (g * xh).sum(-1, keepdim=True) / D
    mag = (r * g).abs() + (r * s1).abs() + (r * xh * s2).abs()
    return dy * xh, dy, mag if m_dx16 is None else mag * m_dx16


def ln_bwd(x, mean, rstd, gamma, dy, dres, m_dx16, dtype=torch.float64, wrong=None):
    """nn.LayerNorm backward.  Returns (dx32, the value dx16 rounds, dgamma, dbeta, dsum).
    xh = (x - mean) * rstd, g = gamma * dy;  dx = rstd * (g - mean(g) - xh * mean(g * xh));
    dres is added into dx32 ONLY; dx16 is dx times its mask; dsum = column sums of that masked
    branch gradient; dgamma = column sums of dy * xh, dbeta of dy."""
    x, mean, rstd, gamma, dy, dres, m_dx16 = (_c(t, dtype) for t in (x, mean, rstd, gamma, dy, dres, m_dx16))
    D = x.shape[1]
    div = {"div+": D + 256, "div-": D - 256}.get(wrong, D)
    r = rstd[:, None]
    xh = (x - mean[:, None]) * r
    g = gamma * dy
    s1 = g.sum(-1, keepdim=True) / div
    s2 = (g * xh).sum(-1, keepdim=True) / div
    o = r * (g - s1) if wrong == "no_cx" else r * (g - s1 - xh * s2)
    dx32 = o if dres is None else o + dres
    branch = dx32 if wrong == "dres_in_branch" else o
    dx16 = branch if m_dx16 is None else branch * m_dx16
    return dx32, dx16, (dy * xh).sum(0), dy.sum(0), dx16.sum(0)


def rel_rows(got, ref):
    """Largest error of a dx, each row relative to that row's max |ref| (float)."""
    ref = ref.double()
    norm = ref.abs().amax(-1).clamp_min(1e-300)
    return float(((got.double() - ref).abs().amax(-1) / norm).max())


def rel_cols(got, ref, terms):
    """Largest error of a column sum relative to the column's sum_r |term| (float)."""
    norm = terms.double().abs().sum(0).clamp_min(1e-300)
    return float(((got.double() - ref.double()).abs() / norm).max())


def fp32_stats(case):
    """The fp64 statistics of a case rounded to fp32: what a correct forward hands the backward."""
    x = case["x"]
    mean, rstd = ln_stats(x)
    return rms_stats(x).float(), mean.float(), rstd.float()


def fp32_errors(D, rows, dres):
    """Errors of the fp32 evaluation of both references against the fp64 one at one case, no masks:
    {"dx": ..., "colsum": ...}."""
    c = make_inputs(D, rows)
    rs, mu, lrs = fp32_stats(c)
    dr = c["dres"] if dres else None
    a64 = rms_bwd(c["x"], rs, c["w"], c["dy"], dr, None, None, None)
    a32 = rms_bwd(c["x"], rs, c["w"], c["dy"], dr, None, None, None, dtype=torch.float32)
    l64 = ln_bwd(c["x"], mu, lrs, c["w"], c["dy"], dr, None)
    l32 = ln_bwd(c["x"], mu, lrs, c["w"], c["dy"], dr, None, dtype=torch.float32)
    tg, tb, ts = ln_terms(c["x"], mu, lrs, c["w"], c["dy"], None)
    dx = max(rel_rows(a32[0], a64[0]), rel_rows(l32[0], l64[0]), rel_rows(l32[1], l64[1]))
    cs = max(rel_cols(a32[2], a64[2], rms_terms(c["x"], rs, c["dy"], None)),
             rel_cols(l32[2], l64[2], tg), rel_cols(l32[3], l64[3], tb), rel_cols(l32[4], l64[4], ts))
    return {"dx": dx, "colsum": cs}


@functools.lru_cache(maxsize=None)
def yardstick():
    """Per output kind, the largest fp32-against-fp64 error over all (D, rows) cases, with and
    without dres: {"dx": ..., "colsum": ...}.  CPU only; nothing of a kernel enters it."""
    out = {"dx": 0.0, "colsum": 0.0}
    for D in WIDTHS:
        for rows in ROWS:
            for dres in (False, True):
                e = fp32_errors(D, rows, dres)
                out = {k: max(out[k], e[k]) for k in out}
    return out


def bound(kind):
    """Relative bound of a kernel output of `kind` against the fp64 reference."""
    return max(FACTOR * yardstick()[kind], FLOOR)
