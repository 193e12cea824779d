"""The optimiser tail (csrc/optim.hip, csrc/adamw.h) against tests/optim_ref.py in fp64: the clip
norm (vqa_grad_sqnorm, vqa_grad_sqnorm_final), the step's scalars (vqa_optim_finalize), the dense
AdamW-amsgrad pass (vqa_adamw_amsgrad) and the embedding table's row-split one (vqa_embed_mark +
vqa_adamw_rows).  Every output buffer (p, m, v, vmax, p16, ws, state, mark, counter) sits between
sentinel-filled guard regions that every test checks (the `pool` fixture).

Bounds.  p, m, v and vmax are judged with optim_ref's normalisers against max(4 x yardstick, 2^-22),
the yardstick being the fp32 evaluation of the same formulas against the fp64 one on these very
inputs, measured on the CPU (tests/test_optim_ref_cpu.py; the nearest wrong variant there, the
decay with an LR not multiplied by lam, sits 1326 bounds away):
                 yardstick  p / m / v / vmax                    bound  p / m / v / vmax
  dense step     2.07e-7  2.87e-7  2.61e-7  1.17e-7      8.28e-7  1.15e-6  1.05e-6  4.67e-7
  six steps      2.63e-7  6.07e-7  2.67e-7  2.67e-7      1.05e-6  2.43e-6  1.07e-6  1.07e-6
  table step     2.36e-7  3.82e-7  2.69e-7  1.87e-7      9.45e-7  1.53e-6  1.07e-6  7.46e-7
Sums of squares: both sides fp64 sums of positive terms, n/4 x 2^-50 relative.  GRAD_NORM,
LR_SCALE, BC1, BC2_SQRT: 1 fp32 ulp of the fp64 value (libm pow, nothing else).  CLIP_COEF, the bf16
shadow, windows, the row split and the element update restated in numpy float32: bit for bit.

Measured on an MI355X (profiles/optim_parity.json), factor 4 never raised:
  dense step, 1 / 7 / 8 groups   p 1.31e-7 .. 2.07e-7   m 1.73e-7 .. 2.87e-7   v 1.62e-7 .. 2.61e-7   vmax 9.4e-8 .. 1.17e-7
  six steps                      p 2.63e-7              m 6.07e-7              v 2.67e-7              vmax 2.67e-7
  table step, 18 cases           p 1.00e-7 .. 2.36e-7   m 4.6e-8 .. 3.82e-7    v 5.1e-8 .. 2.69e-7    vmax 0 .. 1.87e-7
  sums of squares                at most 0.4 % of n/4 x 2^-50
Several maxima equal the yardstick's to the last digit: the element update is bit-identical to its
numpy float32 restatement (test_dense), so the kernel IS an fp32 evaluation of these formulas.

Paths no kernel test entered before, and the case here that reaches each:
  * sq_range's 4x-unrolled main loop (n/4 > 3 x 256 x parts) ........ test_sqnorm sizes 3S+1, 4S+5, 9S+77
  * finalize_body's second outer trip (parts > 4096) ................ test_finalize_parts 4097, 8200
  * vqa_adamw_rows with touched > 1 (workgroup-striding grid) ....... test_rows_split touched 2, 7, rows-1, 256
  * vqa_adamw_rows with > 192 float4 per row (second column trip) ... test_rows_split cols 772, 1024
  * a group boundary inside a workgroup / a wave .................... test_dense ends 1, 255, 257, 300, 301
  * more than 3 groups .............................................. test_dense ngroups 7, 8; test_multi_step
  * descriptors as _adam_range_desc builds them (negative ends, ends beyond n) ... test_dense windows
  * grad_scale != 1 ................................................. test_dense, test_multi_step, test_finalize_clip
  * max_norm <= 0 ................................................... test_finalize_clip
  * PENDING == 0 at kernel level .................................... test_dense, test_rows_split
  * param16 == NULL ................................................. test_dense
  * schedule edges (step == warmup, step >= total, warmup 0 / 1, total - warmup <= 1, large step) ... test_finalize_schedule

Non-finite partials (test_finalize_nonfinite): inf gives norm inf, coef 0; NaN gives norm NaN and
coef 1, because fminf drops the NaN -- torch's clip_grad_norm_ would give a NaN coefficient.  The
kernel is left so (include/vqa_hip.h says why): the row-split identity needs a finite coefficient."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as orf

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FILL = -7.0                                    # sentinel of every guard (exact in bf16 and int32 too)
GUARD = 64                                     # guard elements before and after a buffer
B1, B2, EPS, WD = (float(x) for x in (orf.B1, orf.B2, orf.EPS, orf.WD))
ST_STEP, ST_NORM, ST_COEF, ST_LAM, ST_BC1, ST_BC2S, ST_PENDING = 0, 1, 2, 3, 4, 5, 8
ST_SPARE = (6, 7, 9, 10, 11, 12, 13, 14, 15)


@pytest.fixture(scope="module")
def k(pkg):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pkg.lib.load()
    return pkg.lib


class Buf:
    """n elements between two guard regions of GUARD sentinel elements."""

    def __init__(self, n, dtype=torch.float32, init=None):
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device="cuda")
        self.t = self.full[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(torch.from_numpy(np.array(init)).to(dtype))       # (a writable copy: cases are frozen)

    def ptr(self, off=0):
        return self.full.data_ptr() + (GUARD + off) * self.full.element_size()

    def guards_ok(self):
        f = self.full
        return bool((f[:GUARD] == FILL).all()) and bool((f[GUARD + self.n:] == FILL).all())

    def np(self):
        t = self.t.view(torch.int16) if self.t.dtype == torch.bfloat16 else self.t
        a = t.cpu().numpy()
        return a.view(np.uint16) if self.t.dtype == torch.bfloat16 else a


class Pool:
    def __init__(self):
        self.bufs = []

    def new(self, n, dtype=torch.float32, init=None):
        self.bufs.append(Buf(n, dtype, init))
        return self.bufs[-1]

    def state(self, step, pending=0.0):
        """A float[16] state block: STEP set, the spare floats 6, 7, 9..15 marked."""
        st = np.zeros(16, F32)
        st[ST_STEP], st[ST_PENDING] = step, pending
        st[list(ST_SPARE)] = [100.0 + i for i in ST_SPARE]
        return self.new(16, init=st)

    def check(self):
        torch.cuda.synchronize()
        assert all(b.guards_ok() for b in self.bufs), "a guard region was written"


@pytest.fixture
def pool():
    p = Pool()
    yield p
    p.check()


def _rc(L, name, *args):
    return getattr(L.load(), name)(*args, L.stream_handle())


def _call(L, name, *args):
    L.check(_rc(L, name, *args), name)


def _err_invalid():
    from __graft_entry__ import ROOT
    return int(re.search(r"#define VQA_ERR_INVALID (\d+)", open(os.path.join(ROOT, "include", "vqa_hip.h")).read()).group(1))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ulp32(x):
    return float(np.spacing(np.abs(F32(x)))) if np.isfinite(x) and x != 0 else float(np.spacing(F32(1e-30)))


def _within_ulp(got, want64, ulps=1):
    """got (fp32) within `ulps` fp32 ulps of the fp32 rounding of the fp64 value want64."""
    return abs(float(got) - float(F32(want64))) <= ulps * _ulp32(want64)


def _record(report, name, err, bound):
    """Print, record, then assert each tensor's error against its bound."""
    for key in ("p", "m", "v", "vm"):
        print(f"optim {name} {key}: {err[key]:.3e} (bound {bound[key]:.3e})")
        report[f"optim_{name}_{key}"] = err[key]
    for key in ("p", "m", "v", "vm"):
        assert err[key] <= bound[key], (name, key, err[key], bound[key])


# ------------------------------------------------------------------ vqa_grad_sqnorm
def _sq_values(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "mixed":                       # randn, a third x 1e-4, a few x 1e4
        g = rng.standard_normal(n)
        g[rng.random(n) < 1 / 3] *= 1e-4
        g[rng.integers(0, max(n, 1), min(5, n))] *= 1e4
        return g.astype(F32)
    if kind == "tiny":                        # squares underflow in fp32
        return np.full(n, 1e-25, F32)
    g = rng.standard_normal(n).astype(F32)    # "huge": one square overflows fp32
    g[n // 2] = 1e20
    return g


def _partials_ref(g, parts):
    """fp64 partials of the documented partition: float4 i belongs to partial (i mod S) div 256,
    S = 256 parts.  Returns (partials, float4 count per partial)."""
    sq4 = (g.astype(F64) ** 2).reshape(-1, 4).sum(1)
    which = (np.arange(sq4.size) % (256 * parts)) // 256
    return np.bincount(which, weights=sq4, minlength=parts), np.bincount(which, minlength=parts)


def _check_partials(ws, g, parts):
    want, count = _partials_ref(g, parts)
    n4 = g.size // 4
    total = orf.sqnorm(g)
    # positive terms, fp64 on both sides: 4 n/4 additions of 2^-53 each way, n/4 x 2^-50 as stated
    assert abs(float(ws.sum()) - total) <= n4 * 2.0 ** -50 * total, (n4, float(ws.sum()), total)
    assert np.all(np.abs(ws - want) <= np.maximum(count, 1) * 2.0 ** -50 * want), (n4, parts)
    return total


@pytest.mark.parametrize("parts", [1, 3, 64])
def test_sqnorm(k, pool, parts, parity_report):
    """S = 256 parts float4s per sweep: 1, 255, 256, 257 (one block's edge); 3S (the unrolled loop
    is not entered); 3S + 1 (exactly one thread enters it); 4S + 5; 9S + 77 (two unrolled trips plus
    tail trips).  The squares of 1e-25 underflow in fp32 and that of 1e20 overflows it."""
    S, worst = 256 * parts, 0.0
    cases = [(n4, "mixed") for n4 in (1, 255, 256, 257, 3 * S, 3 * S + 1, 4 * S + 5, 9 * S + 77)]
    cases += [(4 * S + 5, "tiny"), (4 * S + 5, "huge")]
    for n4, kind in cases:
        g = _sq_values(kind, 4 * n4, 17 * n4 + parts)
        gb, ws = pool.new(4 * n4, init=g), pool.new(parts, torch.float64)
        _call(k, "vqa_grad_sqnorm", gb.ptr(), 4 * n4, ws.ptr(), parts)
        total = _check_partials(ws.np(), g, parts)
        worst = max(worst, abs(float(ws.np().sum()) - total) / total / (n4 * 2.0 ** -50))
        if kind == "tiny":
            assert abs(np.sqrt(ws.np().sum()) / (np.sqrt(4 * n4) * 1e-25) - 1) < 1e-6        # not 0
        if kind == "huge":
            st = pool.state(0)
            _call(k, "vqa_optim_finalize", ws.ptr(), parts, 1.0, 1.0, 2, 10, B1, B2, st.ptr())
            assert np.isfinite(st.np()[ST_NORM]) and _within_ulp(st.np()[ST_NORM], np.sqrt(total))
    parity_report[f"optim_sqnorm_parts{parts}_of_tolerance"] = worst
    # n = 0: all-zero partials
    gb, ws = pool.new(4, init=np.ones(4, F32)), pool.new(parts, torch.float64)
    _call(k, "vqa_grad_sqnorm", gb.ptr(), 0, ws.ptr(), parts)
    assert np.array_equal(ws.np(), np.zeros(parts))


# ------------------------------------------------------------------ vqa_optim_finalize
def _finalize(L, pool, ws, step, gs=1.0, max_norm=1.0, warmup=2, total=10):
    """vqa_optim_finalize over host-written partials; returns the state block after it, having
    checked what every call must leave: STEP + 1, PENDING = 1, the spare floats untouched."""
    w = pool.new(len(ws), torch.float64, init=np.asarray(ws, F64))
    st = pool.state(step)
    before = st.np().copy()
    _call(L, "vqa_optim_finalize", w.ptr(), len(ws), gs, max_norm, warmup, total, B1, B2, st.ptr())
    out = st.np()
    assert out[ST_STEP] == step + 1 and out[ST_PENDING] == 1.0
    assert _same(out[list(ST_SPARE)], before[list(ST_SPARE)])
    assert _same(w.np(), np.asarray(ws, F64))
    return out


def _coef32(norm32, max_norm):
    if max_norm <= 0:
        return F32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.fmin(F32(1.0), F32(max_norm) / (F32(norm32) + F32(1e-6)))


@pytest.mark.parametrize("parts", [1, 255, 256, 257, 3072, 4096, 4097, 8200])
def test_finalize_parts(k, pool, parts):
    """Partials distinct over six decades, the last the largest; then, so that EVERY slot is loud
    in an fp32 norm, 0 / 1 partials: all ones, and slot i = bit b of i for each b (a dropped or
    doubled slot changes a count of at most 8200 by one: 6e-5 of its root).  parts > 4096 is the
    second trip of the kernel's outer loop; 3072 is what the engine finalizes."""
    i = np.arange(parts, dtype=F64)
    ws = 10.0 ** (-6.0 + 6.0 * (i + 1) / parts) * (1.0 + 1e-4 * np.sin(i))
    assert ws.argmax() == parts - 1 and np.unique(ws).size == parts
    out = _finalize(k, pool, ws, 4, gs=0.5)
    assert _within_ulp(out[ST_NORM], np.sqrt(ws.sum()) * 0.5)
    assert _same(out[ST_COEF], _coef32(out[ST_NORM], 1.0))
    patterns = [np.ones(parts)] + [((np.arange(parts) >> b) & 1).astype(F64) for b in range(int(parts - 1).bit_length())]
    for pat in patterns:
        out = _finalize(k, pool, pat, 0)
        assert _within_ulp(out[ST_NORM], np.sqrt(pat.sum())), (parts, pat.sum(), out[ST_NORM])


def test_finalize_clip(k, pool):
    """grad_scale x max_norm (0 and -1: no clip), CLIP_COEF bit-equal to the fp32 formula on the
    device's own GRAD_NORM; a norm just below and just above max_norm."""
    ws = [3.25, 1.5, 0.0625, 7.0]
    for gs in (1.0, 0.5, 1.0 / 3):
        for mn in (1.0, 0.25, 0.0, -1.0):
            out = _finalize(k, pool, ws, 3, gs=gs, max_norm=mn)
            assert _within_ulp(out[ST_NORM], np.sqrt(sum(ws)) * float(F32(gs))), (gs, mn)
            assert _same(out[ST_COEF], _coef32(out[ST_NORM], mn)), (gs, mn, out[ST_COEF])
            assert (out[ST_COEF] == 1.0) == (mn <= 0), (gs, mn)
            for f in (1 - 1e-4, 1 + 1e-4):
                if mn > 0:
                    out = _finalize(k, pool, [(mn * f / float(F32(gs))) ** 2], 3, gs=gs, max_norm=mn)
                    assert _same(out[ST_COEF], _coef32(out[ST_NORM], mn))
                    assert (out[ST_COEF] == 1.0) == (f < 1), (gs, mn, f, out[ST_COEF])
                    if f > 1:
                        assert abs(float(out[ST_COEF]) * f - 1) < 1e-5


def test_finalize_schedule(k, pool):
    """optim_ref.schedule_table(): step == warmup, step >= total, warmup 0 and 1, total - warmup
    <= 1, and the bias corrections at a large step.  LR_SCALE, BC1 and BC2_SQRT within 1 fp32 ulp
    of the fp32 rounding of the fp64 value (libm pow)."""
    for w, t, s in orf.schedule_table():
        out = _finalize(k, pool, [2.0, 0.5], s, warmup=w, total=t)
        ref = orf.finalize(2.5, s, 1.0, 1.0, w, t)
        for idx, key in ((ST_LAM, "lam"), (ST_BC1, "bc1"), (ST_BC2S, "bc2s")):
            assert _within_ulp(out[idx], ref[key]), (w, t, s, key, out[idx], ref[key])
        if ref["lam"] in (0.0, 1.0, 0.5):
            assert float(out[ST_LAM]) == float(ref["lam"])


def test_finalize_nonfinite(k, pool):
    out = _finalize(k, pool, [1.0, np.inf, 2.0], 3)
    assert out[ST_NORM] == np.inf and out[ST_COEF] == 0.0
    out = _finalize(k, pool, [1.0, np.nan, 2.0], 3)
    assert np.isnan(out[ST_NORM]) and out[ST_COEF] == 1.0            # fminf drops the NaN (see the header)


# ------------------------------------------------------------------ vqa_adamw_amsgrad
KEYS = ("p", "m", "v", "vm")


def _tensors(pool, c, n=None):
    """Device copies of a case's p, g, m, v, vm and a sentinel-filled bf16 shadow."""
    n = c["p"].size if n is None else n
    b = {key: pool.new(n, init=c[key]) for key in ("p", "g", "m", "v", "vm")}
    b["p16"] = pool.new(n, torch.bfloat16)
    return b


def _desc(L, b, st, ends, lrs, gs, lo=0, n=None, p16=True):
    """The descriptor of b's elements [lo, lo + n) with the group ends given relative to lo."""
    d = L.AdamWDesc()
    d.param, d.grad, d.exp_avg = b["p"].ptr(lo), b["g"].ptr(lo), b["m"].ptr(lo)
    d.exp_avg_sq, d.max_exp_avg_sq = b["v"].ptr(lo), b["vm"].ptr(lo)
    d.param16 = b["p16"].ptr(lo) if p16 else None
    d.n, d.ngroups = (b["p"].n - lo if n is None else n), len(ends)
    for i, (e, lr) in enumerate(zip(ends, lrs)):
        d.group_end[i], d.group_lr[i] = e, float(lr)
    d.beta1, d.beta2, d.eps, d.weight_decay, d.grad_scale, d.state = B1, B2, EPS, WD, gs, st.ptr()
    return d


def _dense(L, d):
    L.check(L.load().vqa_adamw_amsgrad(ctypes.byref(d), L.stream_handle()), "vqa_adamw_amsgrad")


def _norm_and_finalize(L, pool, g, n, st, sched, parts=3):
    ws = pool.new(parts, torch.float64)
    _call(L, "vqa_grad_sqnorm", g.ptr(), n, ws.ptr(), parts)
    _call(L, "vqa_optim_finalize", ws.ptr(), parts, sched["grad_scale"], sched["max_norm"], sched["warmup"],
          sched["total"], B1, B2, st.ptr())


def _got(b):
    return {key: b[key].np() for key in KEYS}


def _f32_update(p, g, m, v, vm, lr, st, gs):
    """The element update restated op by op in numpy float32 (no contraction, correctly rounded
    divide and square root), from the scalars the device wrote to its state block."""
    one = F32(1.0)
    coef, lam, bc1, bc2s = (F32(st[i]) for i in (ST_COEF, ST_LAM, ST_BC1, ST_BC2S))
    gmul = F32(gs) * coef
    omb1, omb2 = one - orf.B1, one - orf.B2
    lr = lr.astype(F32) * lam
    decay, step_size = one - lr * orf.WD, lr / bc1
    gr = g * gmul
    p = p * decay
    m = m + omb1 * (gr - m)
    v = v * orf.B2 + omb2 * gr * gr
    vm = np.maximum(vm, v)
    denom = np.sqrt(vm) / bc2s + orf.EPS
    p = p - step_size * (m / denom)
    assert all(a.dtype == F32 for a in (p, m, v, vm))
    return dict(p=p, m=m, v=v, vm=vm)


@pytest.mark.parametrize("ngroups", [1, 7, 8])
def test_dense(k, pool, ngroups, parity_report):
    """n / 4 = 4 x 256 + 37, the non-zero state (vmax well above v on half the elements, overtaken
    on the others), grad_scale 0.5 with an active clip (coef 0.05), group ends in float4 units at 1,
    255, 257, 300, 301, 700 (, 900): a one-float4 group, boundaries inside a wave and inside a
    workgroup, 7 and 8 groups (VQA_MAX_GROUPS)."""
    c, S = orf.dense_case(ngroups), orf.DENSE
    n = c["p"].size
    b, st = _tensors(pool, c), pool.state(S["step"])
    _norm_and_finalize(k, pool, b["g"], n, st, S)
    _dense(k, _desc(k, b, st, c["ends"], c["lrs"], S["grad_scale"]))
    got, state = _got(b), st.np()
    ref, sc = orf.case_ref(c, S)
    assert state[ST_COEF] < 0.1 and _within_ulp(state[ST_NORM], sc["norm"]) and state[ST_LAM] == 0.375
    _record(parity_report, f"dense_ng{ngroups}", orf.errors(got, ref, c["p"]), orf.bounds(orf.yardstick_dense()))
    assert _same(b["p16"].np(), orf.bf16_rne(got["p"]))            # RNE of the device's own p
    assert _same(b["g"].np(), c["g"])
    # bit for bit the op-by-op fp32 restatement, fed with the device's scalars
    want = _f32_update(c["p"], c["g"], c["m"], c["v"], c["vm"], orf.group_lrs(n, c["ends"], c["lrs"]), state, S["grad_scale"])
    for key in KEYS:
        assert _same(got[key], want[key]), (key, int((_bits(got[key]) != _bits(want[key])).sum()))
    # param16 = NULL: the same four tensors, the shadow untouched
    b2 = _tensors(pool, c)
    _dense(k, _desc(k, b2, st, c["ends"], c["lrs"], S["grad_scale"], p16=False))
    assert all(_same(b2[key].np(), got[key]) for key in KEYS)
    assert bool((b2["p16"].full == FILL).all())
    # windows as EngineBase._adam_range_desc builds them: pointers moved to lo, n = hi - lo, ends minus
    # lo (negative below the window, beyond n above it): one mid-group, one spanning three groups,
    # the first float4 alone, the last float4 alone
    for lo4, hi4 in ((400, 500), (256, 301), (0, 1), (orf.N4 - 1, orf.N4)):
        lo, hi = 4 * lo4, 4 * hi4
        bw = _tensors(pool, c)
        ends = [e - lo for e in c["ends"]]
        if ngroups > 1 and lo4 == 400:
            assert min(ends) < 0 and max(ends[:-1]) > hi - lo
        _dense(k, _desc(k, bw, st, ends, c["lrs"], S["grad_scale"], lo=lo, n=hi - lo))
        for key in KEYS:
            w = bw[key].np()
            assert _same(w[lo:hi], got[key][lo:hi]), (key, lo4, hi4)
            assert _same(w[:lo], c[key][:lo]) and _same(w[hi:], c[key][hi:]), (key, lo4, hi4)
        s16 = bw["p16"].np()
        assert _same(s16[lo:hi], b["p16"].np()[lo:hi])
        assert np.all(np.delete(s16, np.s_[lo:hi]) == orf.bf16_rne(np.array([FILL], F32))[0])
    # PENDING == 0: nothing is touched
    b0, st0 = _tensors(pool, c), pool.new(16, init=np.where(np.arange(16) == ST_PENDING, 0, state))
    _dense(k, _desc(k, b0, st0, c["ends"], c["lrs"], S["grad_scale"]))
    assert all(_same(b0[key].np(), c[key]) for key in KEYS) and bool((b0["p16"].full == FILL).all())


def test_multi_step(k, pool, parity_report):
    """Six steps with (warmup, total) = (2, 5): lam 0, 1/2, 1, 2/3, 1/3, 0.  The state block is
    carried on the device (STEP comes from finalize), a fresh gradient each step, every second one
    30 x smaller; against the reference carried in fp64."""
    c, S = orf.multi_case(), orf.MULTI
    n = c["p"].size
    b, st = _tensors(pool, dict(c, g=c["grads"][0])), pool.state(0)
    d = _desc(k, b, st, c["ends"], c["lrs"], S["grad_scale"])
    lams = []
    for g in c["grads"]:
        b["g"].t.copy_(torch.from_numpy(np.array(g)))
        _norm_and_finalize(k, pool, b["g"], n, st, S)
        _dense(k, d)
        lams.append(float(st.np()[ST_LAM]))
    assert lams == [float(F32(x)) for x in (0.0, 0.5, 1.0, 2 / 3, 1 / 3, 0.0)] and st.np()[ST_STEP] == 6
    got = _got(b)
    _record(parity_report, "multi_step", orf.errors(got, orf.multi_ref(), c["p"]), orf.bounds(orf.yardstick_multi()))
    assert _same(b["p16"].np(), orf.bf16_rne(got["p"]))


# ------------------------------------------------------------------ vqa_embed_mark + vqa_adamw_rows
def _rows(L, d, mark, rows, cols, touched, S):
    L.check(L.load().vqa_adamw_rows(ctypes.byref(d), mark.ptr(), rows, cols, touched, S["warmup"], S["total"],
                                    L.stream_handle()), "vqa_adamw_rows")


@pytest.mark.parametrize("kind", orf.ROWS_KINDS)
@pytest.mark.parametrize("rows,cols", orf.ROWS_CASES)
def test_rows_split(k, pool, rows, cols, kind, parity_report):
    """The table's update split by rows against the fp64 reference and, bit for bit, against the
    dense pass, for every grid the pre-finalize pass can take: touched 0 (a block per row) and 2, 7,
    rows - 1, 256 at 300 rows (blocks striding over the rows -- the only form the engine launches),
    rows and rows + 5 (a block per row again).  cols 772 and 1024 are 193 and 256 float4 per row:
    a second trip of the 192-thread column loop.  Two groups, the boundary inside a row.  ids hold
    duplicates, -1, rows and rows + 7 (these mark nothing); some marks are stale (step - 2: they
    count as untouched); `none` / `all`: no row / every row marked."""
    c, S = orf.rows_case(rows, cols, kind), orf.ROWS_SCHED
    n, step = rows * cols, S["step"]
    # the dense pass, and its distance from the fp64 reference
    bd, std = _tensors(pool, c), pool.state(step)
    _norm_and_finalize(k, pool, bd["g"], n, std, S)
    _dense(k, _desc(k, bd, std, c["ends"], c["lrs"], S["grad_scale"]))
    dense = dict(_got(bd), p16=bd["p16"].np())
    _record(parity_report, f"rows_{rows}x{cols}_{kind}", orf.errors(dense, orf.case_ref(c, S)[0], c["p"]),
            orf.bounds(orf.yardstick_rows()))
    want_mark = np.where(c["touched"], step, c["mark0"]).astype(np.int32)
    for touched in sorted({0, 2, 7, rows - 1, rows, rows + 5} | ({256} if rows == 300 else set())):
        b, st = _tensors(pool, c), pool.state(step)                 # PENDING == 0 ...
        mark, ids = pool.new(rows, torch.int32, init=c["mark0"]), pool.new(c["ids"].size, torch.int64, init=c["ids"])
        d = _desc(k, b, st, c["ends"], c["lrs"], S["grad_scale"])
        _call(k, "vqa_embed_mark", ids.ptr(), c["ids"].size, rows, mark.ptr(), st.ptr())
        assert np.array_equal(mark.np(), want_mark)
        _rows(k, d, mark, rows, cols, touched, S)                   # ... which the pre-finalize pass ignores
        pre = _got(b)
        rowwise = lambda a: _bits(a).reshape(rows, cols)            # noqa: E731
        for key in KEYS:
            changed = (rowwise(pre[key]) != rowwise(c[key])).any(1)
            assert not changed[c["touched"]].any() and (key == "vm" or changed[~c["touched"]].all()), (key, touched)
        _norm_and_finalize(k, pool, b["g"], n, st, S)
        _rows(k, d, mark, rows, cols, 1, S)
        for key in KEYS:
            assert _same(b[key].np(), dense[key]), (key, touched)
        assert _same(b["p16"].np(), dense["p16"]) and _same(st.np(), std.np())
        pool.check()
    # the touched = 1 pass while PENDING == 0: a no-op
    b, st = _tensors(pool, c), pool.state(step + 1)
    mark = pool.new(rows, torch.int32, init=want_mark)
    _rows(k, _desc(k, b, st, c["ends"], c["lrs"], S["grad_scale"]), mark, rows, cols, 1, S)
    assert all(_same(b[key].np(), c[key]) for key in KEYS) and bool((b["p16"].full == FILL).all())


# ------------------------------------------------------------------ vqa_grad_sqnorm_final
def _sqnorm_final(L, pool, g0, g1, parts, early, mark, lead, cols, step, gs, max_norm):
    fin = len(early) + 2 * parts
    ws = pool.new(fin, torch.float64, init=np.concatenate([early, np.full(2 * parts, FILL)]))
    cnt = pool.new(L.SQNORM_FINAL_COUNTER_WORDS, torch.int32, init=np.zeros(L.SQNORM_FINAL_COUNTER_WORDS, np.int32))
    st = pool.state(step)
    b0, b1 = pool.new(g0.size, init=g0), pool.new(g1.size, init=g1)
    _call(L, "vqa_grad_sqnorm_final", b0.ptr(), g0.size, b1.ptr(), g1.size, ws.ptr(), parts, fin,
          None if mark is None else mark.ptr(), lead, cols, cnt.ptr(), gs, max_norm, 2, 10, B1, B2, st.ptr())
    w, out = ws.np(), st.np()
    assert _same(w[:len(early)], np.asarray(early, F64)) and not cnt.np().any()
    t0 = _check_partials(w[len(early):len(early) + parts], g0, parts)
    t1 = _check_partials(w[len(early) + parts:], g1, parts)
    total = float(np.sum(early)) + t0 + t1
    assert _within_ulp(out[ST_NORM], np.sqrt(total) * float(F32(gs))), (out[ST_NORM], np.sqrt(total) * gs)
    assert _same(out[ST_COEF], _coef32(out[ST_NORM], max_norm))
    ref = orf.finalize(total, step, gs, max_norm, 2, 10)
    assert all(_within_ulp(out[i], ref[key]) for i, key in ((ST_LAM, "lam"), (ST_BC1, "bc1"), (ST_BC2S, "bc2s")))
    assert out[ST_STEP] == step + 1 and out[ST_PENDING] == 1.0
    assert _same(out[list(ST_SPARE)], np.array([100.0 + i for i in ST_SPARE], F32))


def test_sqnorm_final_unrolled(k, pool):
    """parts = 3, n/4 = 9 S + 77 in both ranges: each enters sq_range's unrolled loop; two earlier
    partials are included by the finalize.  Against the fp64 norm, not the three-call form."""
    n = 4 * (9 * 768 + 77)
    _sqnorm_final(k, pool, _sq_values("mixed", n, 1), _sq_values("mixed", n, 2), 3, [0.75, 3.5], None, 0, 0, 5, 0.5, 1.0)


def test_sqnorm_final_marked_rows(k, pool):
    """Range 1 = 8 leading floats read densely, then the 37 x 772 table of which only the marked
    rows are loaded (sq_range_rows; the others hold exact zeros)."""
    c, step = orf.rows_case(37, 772, "some"), orf.ROWS_SCHED["step"]
    g1 = np.concatenate([np.arange(1, 9, dtype=F32), c["g"]])
    mark = pool.new(37, torch.int32, init=np.where(c["touched"], step, c["mark0"]).astype(np.int32))
    assert not c["g"].reshape(37, 772)[~c["touched"]].any()
    _sqnorm_final(k, pool, _sq_values("mixed", 4 * 300, 3), g1, 3, [0.25], mark, 8, 772, step, 1.0, 0.25)


# ------------------------------------------------------------------ refusals
def test_refusals(k, pool):
    """VQA_ERR_INVALID, nothing launched, every buffer untouched: n <= 0, n % 4, a group end % 4,
    ngroups outside [1, 8], an fp32 stream off 16-byte alignment, param16 off 8-byte alignment,
    rows x cols != n, and a misaligned g of vqa_grad_sqnorm."""
    inv = _err_invalid()
    rows, cols = 37, 64
    c, S = orf.rows_case(rows, cols, "all"), orf.ROWS_SCHED
    n = rows * cols
    b, st = _tensors(pool, c), pool.state(S["step"] + 1, pending=1.0)
    mark = pool.new(rows, torch.int32, init=np.full(rows, S["step"], np.int32))

    def good():
        return _desc(k, b, st, c["ends"], c["lrs"], S["grad_scale"])

    def bad(**kw):
        d = good()
        for key, val in kw.items():
            setattr(d, key, val)
        return d
    descs = {"n 0": bad(n=0), "n -4": bad(n=-4), "n % 4": bad(n=n - 2), "ngroups 0": bad(ngroups=0),
             "ngroups 9": bad(ngroups=9), "param16 + 2 B": bad(param16=b["p16"].ptr() + 2)}
    for field, key in (("param", "p"), ("grad", "g"), ("exp_avg", "m"), ("exp_avg_sq", "v"), ("max_exp_avg_sq", "vm")):
        descs[field + " + 4 B"] = bad(**{field: b[key].ptr() + 4})
        descs[field + " + 8 B"] = bad(**{field: b[key].ptr() + 8})
    d = good()
    d.group_end[0] = c["ends"][0] + 2
    descs["group end % 4"] = d
    for name, d in descs.items():
        assert k.load().vqa_adamw_amsgrad(ctypes.byref(d), k.stream_handle()) == inv, name
        for touched in (0, 1, 7):
            assert k.load().vqa_adamw_rows(ctypes.byref(d), mark.ptr(), rows, cols, touched, 10, 100, k.stream_handle()) == inv, name
    for r, cc in ((rows, cols + 4), (rows - 1, cols), (rows, cols - 2), (0, cols)):
        assert k.load().vqa_adamw_rows(ctypes.byref(good()), mark.ptr(), r, cc, 1, 10, 100, k.stream_handle()) == inv
    ws = pool.new(3, torch.float64)
    assert _rc(k, "vqa_grad_sqnorm", b["g"].ptr() + 4, n - 4, ws.ptr(), 3) == inv
    assert _rc(k, "vqa_grad_sqnorm", b["g"].ptr(), n - 2, ws.ptr(), 3) == inv
    torch.cuda.synchronize()
    assert all(_same(b[key].np(), c[key]) for key in KEYS + ("g",))
    assert bool((b["p16"].full == FILL).all()) and bool((ws.full == FILL).all())
    # the same arguments, well-formed, are accepted
    st2 = pool.state(S["step"])
    _norm_and_finalize(k, pool, b["g"], n, st2, S)
    d = _desc(k, b, st2, c["ends"], c["lrs"], S["grad_scale"])
    _dense(k, d)
    _rows(k, d, mark, rows, cols, 1, S)
