"""Plain numpy / torch-CPU restatement of vqa_gemm (csrc/gemm.hip, gemm_fp8.hip, conv_patch.inl), written
from the contract of include/vqa_hip.h: every operand is read from its flat buffer through its own
leading dimension and batch stride, exactly as the header states it.

  build(case)        the flat input buffers of a case (every padded element NaN) and the descriptor fields.
  reference(case)    the contract in fp64: what tests/test_gemm_parity_gpu.py compares the kernels with.
  model(case)        the same chain in fp32: 16-deep steps summed by fp32 adds (e4m3: 64-deep steps with the
                     MFMA's measured alignment loss, _mfma_e4m3) and added to the accumulator in
                     increasing k, split-K partials summed in slice order, the epilogue's
                     operation order without FMA, erf by Abramowitz-Stegun 7.1.26 and tanh as (1-e)/(1+e)
                     with a correctly rounded exp.  A yardstick, never a reference.
  normaliser(case)   per element |alpha| sum_k |A||B| (times both scales for e4m3) + |bias| + |res32| + |res16|
                     + |beta c32_old|: the magnitudes behind that element, not a row or global maximum.
  bound(group)       max(FACTOR x yardstick(group), 2^-22); yardstick = the largest model error over the
                     group's case table.  Nothing a kernel computed enters it.

Errors.  c32: |got - reference| / normaliser.  c16: a correct kernel stores RNE-bf16 of ITS fp32 v, which
lies within half a bf16 ulp of the exact v plus v's own error; so the c16 error is the EXCESS
max(0, |got - v| - ulp_bf16(v) / 2) / normaliser, held to the same bound as c32.  (The plain distance to
RNE-bf16(v) is one ulp wherever the fp32 error crosses a tie: it would hide a truncating store.)  NaN
counts as infinite.

`wrong=` applies one deliberate mistake (MISTAKES) to model(); tests/test_gemm_ref_cpu.py measures how far
each sits from the reference.  No wrong kernel is ever run."""
import dataclasses
import functools
import math
import zlib

import numpy as np
import torch

from oracle import vqa_oracle as orc

FACTOR = 4.0                                   # bound = FACTOR * yardstick, the project's factor
FLOOR = 2.0 ** -22
SEED, COUNTER, SITE = 5, 9, 33                 # dropout stream of every case
FILL = -7.0                                    # sentinel of every output buffer and guard (exact in bf16)
GROWS = 2                                      # guard rows before and after every output
NAN = float("nan")
F32, F64 = np.float32, np.float64
GROUPS = ("plain", "splitk", "conv", "patch", "gelu", "tanh", "fp8")


@dataclasses.dataclass(frozen=True)
class Case:
    group: str
    m: int
    n: int
    k: int
    at: int = 0                # a_trans
    bt: int = 0                # b_trans
    conv: int = 0              # a_conv (1 implicit im2col, 2 LDS patch)
    bconv: int = 0
    geom: tuple = None         # (n, h, w, c, oh, ow, kh, kw, stride, pad)
    bias: int = 0
    res32: int = 0
    res16: int = 0
    mask: int = 0
    p: float = 0.0
    alpha: float = 1.0
    beta: float = 0.0
    act: int = 0
    out: str = "both"          # "both", "c32", "c16"
    batch: int = 1
    shared_b: int = 0          # stride_b = 0
    sbias: int = 0             # the bias moves by stride_bias
    dsite: int = 0             # drop_site_stride
    splitk: int = 0
    fp8: int = 0
    scalar: str = ""           # "" or what forces the scalar epilogue: "ldc" (odd ldc32), "cptr", "bias"
    scale_b: float = 1.0       # standard deviation of B
    seed: int = 0


def name(c):
    s = f"{c.group}_{'At' if c.at else 'A'}{'Bt' if c.bt else 'B'}_{c.m}x{c.n}x{c.k}"
    if c.geom:
        g = c.geom
        s += f"_{'patch' if c.conv == 2 else 'bconv' if c.bconv else 'conv'}{g[0]}x{g[1]}x{g[2]}x{g[3]}k{g[6]}x{g[7]}s{g[8]}p{g[9]}"
    for f, t in (("bias", "b"), ("res32", "r32"), ("res16", "r16"), ("mask", "mk")):
        if getattr(c, f):
            s += "_" + t
    s += (f"_p{c.p}" if c.p else "") + (f"_al{c.alpha}" if c.alpha != 1 else "") + (f"_be{c.beta}" if c.beta else "")
    s += (f"_act{c.act}" if c.act else "") + (f"_{c.out}" if c.out != "both" else "") + (f"_z{c.batch}" if c.batch > 1 else "")
    s += ("_sharedB" if c.shared_b else "") + ("_sbias" if c.sbias else "") + (f"_dsite{c.dsite}" if c.dsite else "")
    s += (f"_sk{c.splitk}" if c.splitk else "") + (f"_{c.scalar}" if c.scalar else "") + (f"_s{c.seed}" if c.seed else "")
    return s


def vec(c):
    """Does the descriptor build() makes take the vectorised epilogue?"""
    return c.n % 8 == 0 and not c.scalar


def conv_out(h, w, kh, kw, stride, pad):
    return (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1


# ------------------------------------------------------------------------------------------ inputs
def _rand(c, tag, *shape):
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.seed}/{tag}/{shape}".encode()))
    return torch.randn(shape, generator=g)


def _bf(t):
    return t.to(torch.bfloat16).float()


def _store(log, ld, stride, dtype, off=0, fill=NAN):
    """[batch, R, C] logical values -> one flat buffer, row pitch ld, batch stride, NaN elsewhere."""
    Z, R, C = log.shape
    flat = torch.full((off + (Z - 1) * stride + R * ld,), fill, dtype=torch.float32)
    for z in range(Z):
        torch.as_strided(flat, (R, C), (ld, 1), off + z * stride).copy_(log[z])
    return flat.to(dtype)


def quant_rows(x):
    """vqa_quant_rows_fp8 on the host: scale = amax / 448 (1 for a zero row), q = e4m3(x / scale), both
    correctly rounded (fp64 quotient, rounded once to fp32: the quotient of two floats rounds the same)."""
    xd = x.double()
    amax = xd.abs().amax(1)
    s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).float()
    q = (xd / s.double()[:, None]).float().to(torch.float8_e4m3fn).view(torch.uint8)
    return q, s


class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def build(c):
    """The buffers and descriptor fields of a case.  The VALUES depend on the shape, layout, batch and seed
    only: cases that differ in outputs, beta, the scalar switch, ... share them."""
    I = Inputs()
    m, n, k, Z = c.m, c.n, c.k, c.batch
    v = vec(c)
    I.alpha, I.beta, I.relu = c.alpha, c.beta, c.act
    # --- A
    if c.conv:
        g = c.geom
        x = _bf(_rand(c, "x", Z, 1, g[0] * g[1] * g[2] * g[3]))
        I.lda, I.stride_a = k, x.shape[2] + 64
        I.a = _store(x, x.shape[2], I.stride_a, torch.bfloat16)
    elif c.fp8:
        I.src_a = _rand(c, "a", Z, m, k) * torch.logspace(-1, 1, m)[None, :, None]
        I.lda, I.stride_a, I.stride_scale_a = k + 16, m * (k + 16) + 64, m + 4
        qs = [quant_rows(I.src_a[z]) for z in range(Z)]
        I.a = _store(torch.stack([q.float() for q, _ in qs]), I.lda, I.stride_a, torch.uint8, fill=127.0)
        I.scale_a = _store(torch.stack([s for _, s in qs])[:, None, :], m, I.stride_scale_a, torch.float32)
    else:
        a = _bf(_rand(c, "a", Z, k, m) if c.at else _rand(c, "a", Z, m, k))
        I.lda = (m + 16) if c.at else (k + 8)
        I.stride_a = a.shape[1] * I.lda + 64
        I.a = _store(a, I.lda, I.stride_a, torch.bfloat16)
    # --- B
    Zb = 1 if c.shared_b else Z
    if c.bconv:
        g = c.geom
        x = _bf(_rand(c, "xb", Zb, 1, g[0] * g[1] * g[2] * g[3]))
        I.ldb, I.stride_b = n, x.shape[2] + 64
        I.b = _store(x, x.shape[2], I.stride_b, torch.bfloat16)
    elif c.fp8:
        I.src_b = _rand(c, "b", Zb, n, k) * c.scale_b
        I.ldb, I.stride_b, I.stride_scale_b = k + 32, n * (k + 32) + 128, n + 8
        qs = [quant_rows(I.src_b[z]) for z in range(Zb)]
        I.b = _store(torch.stack([q.float() for q, _ in qs]), I.ldb, I.stride_b, torch.uint8, fill=127.0)
        I.scale_b = _store(torch.stack([s for _, s in qs])[:, None, :], n, I.stride_scale_b, torch.float32)
    else:
        b = _bf((_rand(c, "b", Zb, k, n) if c.bt else _rand(c, "b", Zb, n, k)) * c.scale_b)
        I.ldb = (n + 8) if c.bt else (k + 24)
        I.stride_b = b.shape[1] * I.ldb + 128
        I.b = _store(b, I.ldb, I.stride_b, torch.bfloat16)
    if c.shared_b:
        I.stride_b = 0
        if c.fp8:
            I.stride_scale_b = 0
    # --- epilogue operands: ldres != ldmask, both wider than n; one stride_res moves all three
    I.ldres, I.ldmask = (n + 24, n + 40) if v else (n + 5, n + 9)
    I.stride_res = m * I.ldmask + (16 if v else 7)
    I.bias_off = 1 if c.scalar == "bias" else 0
    I.stride_bias = (n + 4) if c.sbias else 0
    I.bias = I.res32 = I.res16 = I.mask16 = None
    if c.bias:
        bz = _rand(c, "bias", Z if c.sbias else 1, 1, n)
        I.bias = _store(bz, n, I.stride_bias, torch.float32, off=I.bias_off)
    if c.res32:
        I.res32 = _store(_rand(c, "res32", Z, m, n), I.ldres, I.stride_res, torch.float32)
    if c.res16:
        I.res16 = _store(_bf(_rand(c, "res16", Z, m, n)), I.ldres, I.stride_res, torch.bfloat16)
    if c.mask:
        mk = _bf(_rand(c, "mask", Z, m, n))
        flat = mk.view(-1)
        flat[0::5] = 0.0                                   # +0 and -0: both gate the product off
        flat[2::5] = -0.0
        I.mask16 = _store(mk, I.ldmask, I.stride_res, torch.bfloat16)
    # --- outputs: sentinels, guard rows; the old c32 where beta reads it, NaN where nothing may read it
    I.ldc32 = (n + 8) if (v or c.scalar in ("cptr", "bias")) else (n + 3)
    I.ldc16 = n + 16
    I.stride_c32 = m * I.ldc32 + (24 if v else 5)
    I.stride_c16 = m * I.ldc16 + 40
    I.c32_off = GROWS * I.ldc32 + (1 if c.scalar == "cptr" else 0)
    I.c16_off = GROWS * I.ldc16
    old = _rand(c, "c32_old", Z, m, n) if c.beta else torch.full((Z, m, n), NAN)
    I.c32 = I.c16 = None
    if c.out in ("both", "c32"):
        I.c32 = _store(old, I.ldc32, I.stride_c32, torch.float32, off=I.c32_off, fill=FILL)
        I.c32 = torch.cat([I.c32, torch.full((GROWS * I.ldc32 + 8,), FILL)])
    if c.out in ("both", "c16"):
        I.c16 = torch.full((2 * GROWS * I.ldc16 + (Z - 1) * I.stride_c16 + m * I.ldc16,), FILL, dtype=torch.bfloat16)
    I.old = old
    return I


def written(c, I, which):
    """Boolean map of the elements of the c32 / c16 buffer that the kernel may write."""
    buf, off, ld, st = (I.c32, I.c32_off, I.ldc32, I.stride_c32) if which == "c32" else (I.c16, I.c16_off, I.ldc16, I.stride_c16)
    w = torch.zeros(buf.numel(), dtype=torch.bool)
    for z in range(c.batch):
        torch.as_strided(w, (c.m, c.n), (ld, 1), off + z * st).fill_(True)
    return w


def _view(flat, off, shape, strides):
    """fp64 strided read of a flat buffer (reads past its end give NaN: only a mistake goes there)."""
    need = off + sum((s - 1) * t for s, t in zip(shape, strides)) + 1
    if need > flat.numel():
        flat = torch.cat([flat.double(), torch.full((need - flat.numel(),), NAN, dtype=torch.float64)])
    return torch.as_strided(flat, shape, strides, off).double().numpy()


def im2col(x, g, order="tap", wrong=None):
    """[n, h, w, c] -> the implicit GEMM operand [(img, oh, ow), (kh, kw, c)] of vqa_conv_geom g; order
    "patch": columns (c / 64, kh, kw, c % 64), the a_conv = 2 weight order."""
    n, h, w, ch, oh, ow, kh, kw, st, pad = g
    if wrong == "hw_swapped":
        x = x.reshape(n, w, h, ch).transpose(0, 2, 1, 3)
    sth, stw = st, (1 if wrong == "stride_axis" else st)
    pd = pad + (1 if wrong == "pad_off" else 0)
    cols = np.zeros((n, oh, ow, kh, kw, ch), F64)
    for i in range(kh):
        for j in range(kw):
            ih, iw = np.arange(oh) * sth - pd + i, np.arange(ow) * stw - pd + j
            vh, vw = (ih >= 0) & (ih < h), (iw >= 0) & (iw < w)
            sub = x[:, ih[vh]][:, :, iw[vw]]
            cols[:, np.nonzero(vh)[0][:, None], np.nonzero(vw)[0][None, :], i, j, :] = sub
    if wrong == "khkw_swapped":
        cols = cols.transpose(0, 1, 2, 4, 3, 5)
    if order == "patch" and wrong != "patch_order":
        cols = cols.reshape(n, oh, ow, kh, kw, ch // 64, 64).transpose(0, 1, 2, 5, 3, 4, 6)
    return np.ascontiguousarray(cols).reshape(n * oh * ow, kh * kw * ch)


def _deq(flat):
    return flat.view(torch.float8_e4m3fn).float()


def operands(c, I, z, wrong=None):
    """A(m, k), B(k, n) of batch z as fp64 arrays and the e4m3 row scales (None for bf16)."""
    m, n, k = c.m, c.n, c.k
    sa = sb = None
    if c.conv:
        g = c.geom
        x = _view(I.a, z * I.stride_a, g[:4], (g[1] * g[2] * g[3], g[2] * g[3], g[3], 1))
        A = im2col(x, g, "patch" if c.conv == 2 else "tap", wrong)
    else:
        a = _deq(I.a) if c.fp8 else I.a
        A = _view(a, z * I.stride_a, (m, k), (1, I.lda) if c.at else (I.lda, 1))
    if c.bconv:
        g = c.geom
        x = _view(I.b, z * I.stride_b, g[:4], (g[1] * g[2] * g[3], g[2] * g[3], g[3], 1))
        B = im2col(x, g, "tap", wrong)
    else:
        b = _deq(I.b) if c.fp8 else I.b
        B = _view(b, z * I.stride_b, (k, n), (I.ldb, 1) if c.bt else (1, I.ldb))
    if c.fp8:
        za = 0 if wrong == "scale_batch" else z
        sa = _view(I.scale_a, za * I.stride_scale_a, (m,), (1,))
        sb = _view(I.scale_b, z * I.stride_scale_b, (n,), (1,))
        if wrong == "scale_axis":                           # each scale indexed by the other axis
            sa, sb = np.resize(sb, m), np.resize(sa, n)
    return A, B, sa, sb


def slices(c):
    """effective split-K of the kernel: [(k0, k1)] in elements, whole k-tiles per slice, none empty."""
    tile = 128 if c.fp8 else 64
    nk = -(-c.k // tile)
    if c.splitk <= 1 or nk <= 1:
        return [(0, c.k)]
    per = -(-nk // min(c.splitk, nk))
    return [(s * per * tile, min(c.k, (s + 1) * per * tile)) for s in range(-(-nk // per))]


E4M3_GROUP, E4M3_BITS = 16, 13


def _mfma_e4m3(A, B):
    """One 64-deep step of the e4m3 MFMA as far as it was measured (unit scales, no epilogue, so that the
    instruction is the only operation between the bytes and the output): the products are not summed
    exactly.  256 * 1 + 2^-5 comes out exact, 256 * 1 + 2^-6 as 256, for either sign and wherever the two
    terms are neighbours in k; with the small term 40 elements away, or in the next step, every sum is
    exact.  So within a group of neighbouring k the products are aligned to the largest one's exponent and
    cut, toward zero, below 2^-13 of it.  The model takes groups of 16 and that cut: the coarsest reading
    of the measurement (with log-uniform random bytes it errs 1.9x / 1.7x / 3.1x as much as the instruction
    at k = 64 / 128 / 512: the hardware keeps more of a product that straddles the cut)."""
    out = np.zeros((A.shape[0], B.shape[1]), F64)
    for g in range(0, A.shape[1], E4M3_GROUP):
        P = A[:, None, g:g + E4M3_GROUP] * B[g:g + E4M3_GROUP].T[None, :, :]
        mx = np.abs(P).max(-1, keepdims=True)
        q = np.where(mx == 0, 1.0, np.ldexp(1.0, np.frexp(mx)[1] - 1 - E4M3_BITS))
        out += (np.trunc(P / q) * q).sum(-1)
    return out


def _acc32(c, A, B, wrong):
    tile, step = (128, 64) if c.fp8 else (64, 16)
    A32, B32 = A.astype(F32), B.astype(F32)
    total = np.zeros((c.m, c.n), F32)
    sl = slices(c)
    for si, (k0, k1) in enumerate(sl):
        if wrong == "drop_last_ktile" and k1 == c.k and c.k % tile:
            k1 = c.k // tile * tile
        acc = np.zeros((c.m, c.n), F32)
        for s in range(k0, k1, step):
            if wrong == "miss_ktile" and tile <= s < 2 * tile:
                continue
            if c.fp8:
                acc = (acc.astype(F64) + _mfma_e4m3(A[:, s:min(s + step, k1)], B[s:min(s + step, k1)])).astype(F32)
                continue
            part = np.zeros((c.m, c.n), F32)
            for kk in range(s, min(s + step, k1)):
                part += np.multiply.outer(A32[:, kk], B32[kk])
            acc += part
        if len(sl) == 1:
            return acc
        if wrong == "slice_missing" and si == 1:
            continue
        total += acc
        if wrong == "slice_twice" and si == 1:
            total += acc
    return total


@functools.lru_cache(maxsize=64)
def _mult(p, site, count):
    return orc.dropout_multiplier(p, SEED, COUNTER, site, count)


def _rne16(v32):
    return torch.from_numpy(np.ascontiguousarray(v32, dtype=F32)).to(torch.bfloat16).float().numpy()


def _act(v, act, f, wrong):
    if act == 1:
        return np.maximum(v, f(0))
    if act == 2 and wrong == "gelu_tanh":
        return f(0.5) * v * (f(1) + np.tanh(f(0.7978845608028654) * (v + f(0.044715) * v * v * v)))
    if f is F64:
        if act == 2:
            return 0.5 * v * (1.0 + torch.erf(torch.from_numpy(v / math.sqrt(2.0))).numpy())
        return np.tanh(v)
    if act == 2:                                            # epi_act, operation for operation
        x = v * f(0.7071067811865476)
        ax = np.abs(x)
        t = f(1) / (f(1) + f(0.3275911) * ax)
        poly = ((((f(1.061405429) * t - f(1.453152027)) * t + f(1.421413741)) * t - f(0.284496736)) * t + f(0.254829592)) * t
        y = f(1) - poly * np.exp(-ax * ax)
        return f(0.5) * v * (f(1) + np.copysign(y, x))
    e = np.exp(f(-2) * np.abs(v))
    return np.copysign((f(1) - e) / (f(1) + e), v)


def _epilogue(c, I, z, acc, f, wrong):
    """v and c32 of batch z in dtype f (fp64: the contract; fp32: the kernel's operation order)."""
    m, n = c.m, c.n
    rows, cols = np.arange(m)[:, None], np.arange(n)[None, :]
    zb = 0 if wrong == "bias_stride" else z
    bias = _view(I.bias, I.bias_off + zb * I.stride_bias, (1, n), (0, 1)).astype(f) if c.bias else None
    kf = np.ones((m, n), f)
    if c.mask:
        st = I.stride_c32 if wrong == "mask_stride" else I.stride_res
        mk = _view(I.mask16, z * st, (m, n), (I.ldres if wrong == "mask_ldres" else I.ldmask, 1))
        kf = np.where((mk >= 0) if wrong == "mask_ge" else (mk > 0), f(1), f(0)).astype(f)
        kf = np.where(np.isnan(mk), f(NAN), kf)
    if c.p:
        site = SITE + (z * c.dsite if c.dsite and wrong != "dsite_ignored" else 0)
        pitch = I.ldc32 if wrong == "drop_ldc32" else n
        zm = 0 if (c.dsite and wrong != "dsite_ignored") or wrong == "drop_no_zm" else z * m
        idx = (zm + rows) * pitch + cols
        kf = kf * _mult(c.p, site, int(idx.max()) + 1)[idx].astype(f)
    t = acc.astype(f)
    if wrong == "alpha_on_bias" and c.bias:
        t = (t + bias) * f(c.alpha)
    else:
        t = t * f(c.alpha)
        if c.bias and wrong != "bias_after_k":
            t = t + bias
    v = t * kf
    if wrong == "bias_after_k" and c.bias:
        v = v + bias
    if c.act and wrong == "relu_before_res":
        v = _act(v, c.act, f, wrong)
    if c.res32:
        v = v + _view(I.res32, z * I.stride_res, (m, n), (I.ldc32 if wrong == "res_ldc32" else I.ldres, 1)).astype(f)
    if c.res16:
        v = v + _view(I.res16, z * I.stride_res, (m, n), (I.ldres, 1)).astype(f)
    if c.act and wrong != "relu_before_res":
        v = _act(v, c.act, f, wrong)
    c32 = v
    if c.beta:
        c32 = v + f(c.beta) * I.old[z].numpy().astype(f)
    return v, c32


def _chain(c, exact, wrong=None):
    I = build(c)
    V, C32, C16 = [], [], []
    for z in range(c.batch):
        A, B, sa, sb = operands(c, I, z, wrong)
        if exact:
            acc = (A * sa[:, None]) @ (B * sb[None, :]) if c.fp8 else A @ B
            v, c32 = _epilogue(c, I, z, acc, F64, None)
            c16 = _rne16(v)
        else:
            acc = _acc32(c, A, B, wrong)
            if c.fp8:
                acc = acc * (sa.astype(F32)[:, None] * sb.astype(F32)[None, :])
            v, c32 = _epilogue(c, I, z, acc, F32, wrong)
            src = c32 if wrong == "beta_in_c16" else v
            c16 = (np.ascontiguousarray(src).view(np.int32) & np.int32(-65536)).view(F32) if wrong == "c16_trunc" else _rne16(src)
        V.append(v), C32.append(c32), C16.append(c16)
    return {"v": np.stack(V), "c32": np.stack(C32), "c16": np.stack(C16)}


@functools.lru_cache(maxsize=None)
def reference(c):
    """{"v", "c32", "c16"}: [batch, m, n] fp64 (c16 = RNE-bf16(v), v the value before it)."""
    return _chain(c, True)


def model(c, wrong=None):
    return _chain(c, False, wrong)


@functools.lru_cache(maxsize=None)
def normaliser(c):
    I = build(c)
    out = []
    for z in range(c.batch):
        A, B, sa, sb = operands(c, I, z)
        if c.fp8:
            A, B = A * sa[:, None], B * sb[None, :]
        nm = abs(c.alpha) * (np.abs(A) @ np.abs(B))
        if c.bias:
            nm = nm + np.abs(_view(I.bias, I.bias_off + z * I.stride_bias, (1, c.n), (0, 1)))
        if c.res32:
            nm = nm + np.abs(_view(I.res32, z * I.stride_res, (c.m, c.n), (I.ldres, 1)))
        if c.res16:
            nm = nm + np.abs(_view(I.res16, z * I.stride_res, (c.m, c.n), (I.ldres, 1)))
        if c.beta:
            nm = nm + np.abs(c.beta * I.old[z].numpy().astype(F64))
        out.append(nm)
    return np.stack(out)


def half_ulp16(v):
    """ulp_bf16(v) / 2 of fp64 values (8 significant bits: 2^(e - 8) for |v| in [2^e, 2^(e+1)))."""
    _, e = np.frexp(v)
    return np.where(v == 0, 0.0, np.ldexp(1.0, e - 9))


def errors(c, got):
    """{"c32", "c16"} -> the largest error / normaliser of the outputs `got` holds ([batch, m, n] arrays)."""
    ref, nm = reference(c), normaliser(c)
    out = {}
    if got.get("c32") is not None:
        out["c32"] = np.abs(np.asarray(got["c32"], F64) - ref["c32"]) / nm
    if got.get("c16") is not None:
        d = np.abs(np.asarray(got["c16"], F64) - ref["v"]) - half_ulp16(ref["v"])
        out["c16"] = np.where(np.isnan(d), np.inf, np.maximum(d, 0.0)) / nm
    return {t: float(np.where(np.isnan(e), np.inf, e).max()) for t, e in out.items()}


def error(c, got):
    return max(errors(c, got).values())


# ------------------------------------------------------------------------------------- case tables
LAYOUTS = {"AB": (0, 0), "ABt": (0, 1), "AtB": (1, 0), "AtBt": (1, 1)}
MNS = ((328, 264), (40, 24), (8, 8))           # ragged for every BM / BN; whole waves dead; one fragment corner
KS = (8, 64, 72, 128, 200, 328)                # a partial tile; one; fewer tiles than stages; ...; the ring wraps


def _tiles():
    return {(lay, mn): [Case("plain", mn[0], mn[1], k, at=at, bt=bt, bias=1, res32=1, seed=1) for k in KS]
            for lay, (at, bt) in LAYOUTS.items() for mn in MNS}


TILES = _tiles()                               # A: {(layout, (m, n)): [Case per k]}

_E = dict(group="plain", m=328, n=264, k=72, seed=2)
EPILOGUES = (                                  # B: the terms of the epilogue, one by one and together
    dict(bias=1), dict(res32=1), dict(res16=1), dict(res32=1, res16=1), dict(bias=1, mask=1),
    dict(bias=1, res32=1, p=0.1), dict(bias=1, alpha=0.75, beta=1.0), dict(res16=1, beta=0.5),
    dict(bias=1, p=0.1, act=1), dict(bias=1, res32=1, act=1), dict(bias=1, res16=1, act=1, alpha=0.75),
    dict(bias=1, mask=1, p=0.1, res16=1, alpha=0.75, beta=0.5), dict(bias=1, mask=1, res32=1, beta=1.0),
)
EPI = tuple(Case(**_E, at=0, bt=bt, **e) for bt in (0, 1) for e in EPILOGUES)
SCALAR_EPI = (EPILOGUES[5], EPILOGUES[9], EPILOGUES[11], EPILOGUES[12])
EPI_SCALAR_N = tuple(Case(**{**_E, "n": 262}, **e) for e in SCALAR_EPI)               # B k-contiguous only
EPI_SCALAR = tuple(Case(**_E, bt=bt, scalar=how, **e) for bt in (0, 1) for e in SCALAR_EPI
                   for how in ("ldc", "cptr", "bias") if how != "bias" or e.get("bias"))

_B = dict(group="plain", m=72, n=136, k=136, batch=3, seed=3)
BATCH = (
    Case(**_B, shared_b=1, sbias=1, bias=1, res32=1, mask=1, p=0.1),                  # one site: index (z*m+row)*n+col
    Case(**_B, bt=1, bias=1, sbias=1, res16=1, p=0.1, dsite=5),                       # a site per batch element
    Case(**_B, at=1, bt=1, sbias=1, bias=1, res32=1, mask=1, beta=0.5),
)

_S = dict(group="splitk", batch=2, bias=1, mask=1, res16=1, beta=1.0, seed=4)
_GS = (2, 6, 5, 64, 6, 5, 3, 3, 1, 1)           # a_conv = 1: 9 k-tiles
_GB = (3, 9, 8, 8, 9, 8, 3, 3, 1, 1)            # b_conv: k = 216, 4 k-tiles
SPLITK = tuple(
    [Case(m=72, n=136, k=k, at=at, bt=bt, splitk=sk, **_S) for (at, bt) in LAYOUTS.values()
     for k, sk in ((328, 2), (328, 3), (136, 5), (64, 2))]
    + [Case(m=60, n=72, k=576, conv=1, geom=_GS, splitk=sk, **_S) for sk in (2, 3)]
    + [Case(m=40, n=72, k=216, at=1, bt=1, bconv=1, geom=_GB, splitk=sk, **_S) for sk in (2, 3)])


def _conv(n, h, w, ch, co, kh, kw, st, pad, **kw_):
    oh, ow = conv_out(h, w, kh, kw, st, pad)
    return Case("conv", n * oh * ow, co, kh * kw * ch, conv=1, geom=(n, h, w, ch, oh, ow, kh, kw, st, pad), bias=1,
                act=1, scale_b=0.25, seed=5, **kw_)


def _bconv(n, h, w, ch, co, kh, kw, st, pad):
    oh, ow = conv_out(h, w, kh, kw, st, pad)
    return Case("conv", co, kh * kw * ch, n * oh * ow, at=1, bt=1, bconv=1, geom=(n, h, w, ch, oh, ow, kh, kw, st, pad),
                beta=1.0, seed=5)


def _patch(n, h, w, ch, co):
    return Case("patch", n * h * w, co, 9 * ch, conv=2, geom=(n, h, w, ch, h, w, 3, 3, 1, 1), bias=1, res16=1, act=1,
                scale_b=0.1, seed=6)


CONV = (
    _conv(2, 9, 7, 64, 72, 3, 3, 1, 1), _conv(2, 12, 9, 128, 40, 3, 3, 2, 1), _conv(3, 8, 5, 64, 24, 1, 1, 2, 0),   # cfast
    _conv(2, 9, 12, 16, 40, 3, 4, 1, 1), _conv(3, 7, 9, 32, 24, 2, 2, 2, 0), _conv(2, 8, 11, 32, 72, 3, 2, 1, 3),   # rfast
    _conv(2, 12, 9, 8, 40, 7, 7, 2, 3), _conv(2, 9, 7, 24, 72, 3, 3, 1, 1), _conv(3, 5, 9, 40, 24, 1, 3, 1, 0),     # general
    _conv(2, 7, 12, 24, 40, 3, 3, 2, 0),
)
BCONV = (_bconv(2, 9, 7, 16, 40, 3, 3, 1, 1), _bconv(3, 9, 12, 8, 72, 3, 3, 2, 1))
PATCH = (_patch(1, 8, 8, 64, 64), _patch(2, 7, 7, 128, 136), _patch(1, 6, 10, 64, 72), _patch(1, 5, 12, 128, 64),
         _patch(1, 4, 41, 128, 64), _patch(1, 14, 12, 128, 64))      # the last: ragged row blocks, 10 + 4 and 5 + 5 + 4


def _ext(act):
    e = dict(group="gelu" if act == 2 else "tanh", act=act, bias=1, res32=1, beta=1.0, seed=7)
    return (Case(m=72, n=136, k=72, scale_b=2 / math.sqrt(72), **e), Case(m=40, n=132, k=8, scale_b=2 / math.sqrt(8), **e),
            Case(m=72, n=136, k=72, scale_b=2 / math.sqrt(72), batch=2, sbias=1, **e))


EXT = _ext(2) + _ext(3)

_F = dict(group="fp8", bias=1, res32=1, act=1, scale_b=0.05, seed=8)
FP8 = tuple([Case(m=328, n=264, k=k, fp8=1, **_F) for k in (16, 80, 336)]
            + [Case(m=328, n=260, k=80, fp8=1, **_F),
               Case(m=72, n=136, k=80, fp8=1, batch=3, sbias=1, **_F),
               Case(m=328, n=264, k=336, fp8=1, splitk=2, **_F)])

_T, _N, _K = 72, 136, 200                       # H: dX[T, K] = dY[T, N] W[N, K], dW[N, K] = dY^T X
PAIR = (Case("plain", _T, _K, _N, at=0, bt=1, res16=1, seed=9), Case("plain", _N, _K, _T, at=1, bt=1, beta=1.0, out="c32", seed=9))


def table(group):
    """Every case of `group` that the GPU test compares with the reference."""
    if group == "plain":
        return tuple(c for v in TILES.values() for c in v) + EPI + EPI_SCALAR_N + BATCH + PAIR
    if group in ("gelu", "tanh"):
        return tuple(c for c in EXT if c.group == group)
    return {"splitk": SPLITK, "conv": CONV + BCONV, "patch": PATCH, "fp8": FP8}[group]


@functools.lru_cache(maxsize=None)
def yardstick(group):
    return max(error(c, model(c)) for c in table(group))


def bound(group):
    return max(FACTOR * yardstick(group), FLOOR)


# ---------------------------------------------------------------------------------------- mistakes
# name -> which cases it can show on
MISTAKES = {
    "drop_last_ktile": lambda c: c.k % (128 if c.fp8 else 64) != 0,
    "miss_ktile": lambda c: c.k > 64 and not c.fp8,
    "bias_after_k": lambda c: c.bias and (c.mask or c.p),
    "alpha_on_bias": lambda c: c.bias and c.alpha != 1,
    "relu_before_res": lambda c: c.act == 1 and (c.res32 or c.res16),
    "beta_in_c16": lambda c: c.beta and c.out == "both",
    "mask_ge": lambda c: c.mask,
    "mask_ldres": lambda c: c.mask,
    "res_ldc32": lambda c: c.res32,
    "mask_stride": lambda c: c.mask and c.batch > 1,
    "bias_stride": lambda c: c.sbias,
    "drop_ldc32": lambda c: c.p,
    "drop_no_zm": lambda c: c.p and c.batch > 1 and not c.dsite,
    "dsite_ignored": lambda c: c.p and c.dsite,
    "slice_missing": lambda c: len(slices(c)) > 1,
    "slice_twice": lambda c: len(slices(c)) > 1,
    "khkw_swapped": lambda c: c.geom and c.conv != 2,
    "hw_swapped": lambda c: c.geom and c.geom[1] != c.geom[2],
    "pad_off": lambda c: c.geom,
    "stride_axis": lambda c: c.geom and c.geom[8] > 1,
    "patch_order": lambda c: c.conv == 2 and c.geom[3] > 64,
    "scale_axis": lambda c: c.fp8,
    "scale_batch": lambda c: c.fp8 and c.batch > 1,
    "c16_trunc": lambda c: c.out in ("both", "c16"),
    "gelu_tanh": lambda c: c.act == 2,
}


# ------------------------------------------------------------------------------------------- fdiv
def fdiv(a, d):
    """gemm_common.h fdiv in numpy float32: a / d by a float reciprocal and a one-step correction."""
    a = np.asarray(a, np.int64)
    inv = F32(1) / F32(d)
    q = (a.astype(F32) * inv).astype(np.int64)
    q = q - (q * d > a)
    return q + ((q + 1) * d <= a)


# output-map sizes (oh, ow) of the b_conv geometries: the tables above and the ConvTranspose2d scaler's 3x3 /
# 1 / 1 weight gradient over the layer4 map of a 224 .. 512 pixel image, 7 .. 16 wide (the form b_conv was
# written for; the engines now run it through vqa_tap_shift)
FDIV_MAPS = tuple(sorted({(c.geom[4], c.geom[5]) for c in SPLITK + BCONV if c.bconv} | {(s, s) for s in range(7, 17)}))
