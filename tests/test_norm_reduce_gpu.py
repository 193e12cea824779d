"""The row-norm backward kernels and the deterministic column reductions behind them
(csrc/norms.hip, csrc/elementwise.hip) against tests/norm_ref.py in fp64, at all four widths and
in the DEFERRED form the engines issue: vqa_rmsnorm_bwd(dw = NULL), vqa_layernorm_bwd(dgamma =
dbeta = NULL, dsum as a flag) and vqa_colsum(out = NULL) write per-block partial rows only, and
one vqa_colsum_batched launch over a device array of vqa_colsum_job finishes them.

Rows (the backward kernels take vqa_norm_bwd_parts(rows) blocks, 8 rows each today): 1 = one wave;
5 = a wave's two-row pair in a partial block; 13 = a partial second block with a pair; 37 = a ragged
tail; 136 = 17 parts, one more than the 16 part-groups of the final reduction; 264 = 33 parts, a
third round.

Bound (A to C): 4 x the yardstick of norm_ref.yardstick(): the largest error of the SAME formulas
evaluated by torch in fp32 on the CPU against fp64 over all 24 (D, rows) cases -- dx relative to
its row's max |dx|, column sums relative to the column's sum_r |term| (dsum: of the magnitudes of
its terms' three parts, see norm_ref.ln_terms) -- and never below 2^-22.  The kernel's sums (a
64-lane xor tree, the four-wave LDS sum, 16 part-groups) and torch's are two fp32 orders of the
same sum, so their errors against fp64 are of one magnitude; the wrong variants measured in
tests/test_norm_ref_cpu.py sit 778 bounds away at the nearest (divisor D + 256 in the RMSNorm dx).
The statistics are the forward kernel's own; they are checked apart (rstd within 2^-21 relative:
a 1024-term positive sum by any tree plus one ulp of the reciprocal square root).

Measured on an MI355X (profiles/norm_reduce_parity.json), yardstick dx 1.80e-7 / column sums
3.81e-7, so bounds 7.18e-7 / 1.52e-6, factor 4 never raised: RMSNorm dx 6.3e-8 .. 1.06e-7, LayerNorm
dx 5.9e-8 .. 1.64e-7 (torch fp32 at the same cases: 9.0e-8 .. 1.80e-7); dw 4.0e-8 .. 1.42e-7, dgamma
3.5e-8 .. 1.95e-7, dbeta 0 (one row) .. 1.20e-7, dsum 1.31e-7 .. 4.08e-7 (torch fp32 column sums:
1.39e-7 .. 3.81e-7).  vqa_colsum_batched on randn: 1.47e-7 of sum |term| (torch fp32 .sum(0): 1.42e-7).

D and E pin the deferred form bit for bit against the immediate one and, on integers in [-8, 8]
(sum |x| < 2^24: every fp32 order is exact, tests/test_norm_ref_cpu.py), against int64 sums."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import norm_ref as nr
from oracle import vqa_oracle as orc

pytestmark = pytest.mark.gpu
FILL = -7.0                                    # sentinel of every output / workspace / guard
GUARD = 64                                     # guard floats after a buffer
SEED, COUNTER = 9, 2
BF16_REL = 2.0 ** -8                           # bf16 round-to-nearest is within 2^-9; 2^-8 as stated


@pytest.fixture(scope="module")
def k(pkg):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pkg.lib.load()
    return pkg.lib


def _p(t):
    return None if t is None else t.data_ptr()


def _rc(L, name, *args):
    return getattr(L.load(), name)(*[_p(a) if isinstance(a, torch.Tensor) else a for a in args], L.stream_handle())


def _call(L, name, *args):
    L.check(_rc(L, name, *args), name)


def _full(*shape, dtype=torch.float32):
    return torch.full(shape, FILL, device="cuda", dtype=dtype)


def _err_invalid():
    from __graft_entry__ import ROOT
    return int(re.search(r"#define VQA_ERR_INVALID (\d+)", open(os.path.join(ROOT, "include", "vqa_hip.h")).read()).group(1))


class Drop:
    """vqa_dropout structs of one rng state (kept alive with it) and their multipliers."""

    def __init__(self, L, p):
        self.L, self.p = L, p
        self.rng = torch.tensor([SEED, COUNTER, 1], dtype=torch.int32, device="cuda")
        self.keep = []

    def ptr(self, site):
        d = self.L.Dropout(self.p, site, self.rng.data_ptr())
        self.keep.append(d)
        return ctypes.addressof(d)

    def mult(self, site, rows, D):
        return torch.from_numpy(orc.dropout_multiplier(self.p, SEED, COUNTER, site, rows * D)).view(rows, D)


class Case:
    """One (D, rows): CPU inputs, their device copies, the forward kernels' statistics."""

    def __init__(self, L, D, rows):
        self.D, self.rows = D, rows
        self.c = nr.make_inputs(D, rows)
        self.g = {n: t.cuda() for n, t in self.c.items()}
        g = self.g
        y = _full(rows, D)
        self.rs, self.mu, self.lrs = _full(rows), _full(rows), _full(rows)
        _call(L, "vqa_rmsnorm_fwd", g["x"], g["w"], y, None, self.rs, rows, D, nr.RMS_EPS, None)
        _call(L, "vqa_layernorm_fwd", g["x"], g["w"], g["b"], y, None, self.mu, self.lrs, rows, D, nr.LN_EPS)
        torch.cuda.synchronize()
        self.rs_c, self.mu_c, self.lrs_c = self.rs.cpu(), self.mu.cpu(), self.lrs.cpu()
        self.ws_floats = L.load().vqa_norm_bwd_workspace_floats(rows, D)

    def ws(self):
        return _full(self.ws_floats + GUARD)

    def rms(self, L, dres=True, o32=True, o16=True, dw=None, beta=0.0, ws=None, drops=(None, None, None)):
        """vqa_rmsnorm_bwd -> (dx32, dx16, ws); dw (a tensor, or None = deferred) is written in place."""
        g, rows, D = self.g, self.rows, self.D
        dx32 = _full(rows, D) if o32 else None
        dx16 = _full(rows, D, dtype=torch.bfloat16) if o16 else None
        ws = self.ws() if ws is None else ws
        _call(L, "vqa_rmsnorm_bwd", g["dy"], g["x"], self.rs, g["w"], g["dres"] if dres else None, dx32, dx16, dw,
              beta, ws, rows, D, *drops)
        torch.cuda.synchronize()
        return dx32, dx16, ws

    def ln(self, L, dres=True, o32=True, o16=True, dg=None, db=None, dsum=None, ws=None, drop=None):
        g, rows, D = self.g, self.rows, self.D
        dx32 = _full(rows, D) if o32 else None
        dx16 = _full(rows, D, dtype=torch.bfloat16) if o16 else None
        ws = self.ws() if ws is None else ws
        _call(L, "vqa_layernorm_bwd", g["dy"], g["x"], self.mu, self.lrs, g["w"], g["dres"] if dres else None, dx32,
              dx16, dg, db, ws, rows, D, drop, dsum)
        torch.cuda.synchronize()
        return dx32, dx16, ws

    def rms_ref(self, dres, m_dy=None, m32=None, m16=None):
        c = self.c
        return nr.rms_bwd(c["x"], self.rs_c, c["w"], c["dy"], c["dres"] if dres else None, m_dy, m32, m16)

    def ln_ref(self, dres, m16=None):
        c = self.c
        return nr.ln_bwd(c["x"], self.mu_c, self.lrs_c, c["w"], c["dy"], c["dres"] if dres else None, m16)


@pytest.fixture(scope="module")
def cases(k):
    made = {}

    def get(D, rows):
        if (D, rows) not in made:
            made[(D, rows)] = Case(k, D, rows)
        return made[(D, rows)]
    return get


def _jobs(L, specs):
    """Device array of vqa_colsum_job from (ws pointer, out pointer, stride, parts, cols, beta):
    first_block cumulative ceil(cols / 64).  Returns (device bytes, njobs, nblocks)."""
    arr, nb = (L.ColsumJob * len(specs))(), 0
    for j, (ws, out, stride, parts, cols, beta) in enumerate(specs):
        arr[j] = L.ColsumJob(ws, out, stride, parts, cols, beta, nb)
        nb += -(-cols // 64)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda(), len(specs), nb


def _run_jobs(L, specs):
    dev, n, nb = _jobs(L, specs)
    _call(L, "vqa_colsum_batched", dev, n, nb)
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# --------------------------------------------------------------------------- A
def _bf16_ok(dx16, ref, what):
    ref = ref.double()
    err = (dx16.double().cpu() - ref).abs()
    lim = BF16_REL * ref.abs() + nr.bound("dx") * ref.abs().amax(-1, keepdim=True)
    assert bool((err <= lim).all()), (what, float((err - lim).max()))


@pytest.mark.parametrize("rows", nr.ROWS)
@pytest.mark.parametrize("D", nr.WIDTHS)
def test_backward_matches_fp64(k, cases, parity_report, D, rows):
    cs = cases(D, rows)
    c = cs.c
    parts = k.load().vqa_norm_bwd_parts(rows)
    assert 0 < parts <= rows and parts * D * 3 == cs.ws_floats
    # the forward's statistics, which the references below take as given
    rs64 = nr.rms_stats(c["x"])
    mu64, lrs64 = nr.ln_stats(c["x"])
    assert float(((cs.rs_c.double() - rs64).abs() / rs64).max()) <= 2.0 ** -21
    assert float(((cs.lrs_c.double() - lrs64).abs() / lrs64).max()) <= 2.0 ** -21
    assert float(((cs.mu_c.double() - mu64).abs() / c["x"].double().abs().mean(-1)).max()) <= 2.0 ** -21
    rec = {}

    def dx_ok(name, got, ref):
        e = nr.rel_rows(got.cpu(), ref)
        rec[name] = max(rec.get(name, 0.0), e)

    def col_ok(name, got, ref, terms):
        e = nr.rel_cols(got.cpu(), ref, terms)
        rec[name] = max(rec.get(name, 0.0), e)

    r_terms = nr.rms_terms(c["x"], cs.rs_c, c["dy"], None)
    l_terms = nr.ln_terms(c["x"], cs.mu_c, cs.lrs_c, c["w"], c["dy"], None)
    for dres in (False, True):
        r32, r16, rdw = cs.rms_ref(dres)
        both16 = None
        for o32, o16 in ((True, True), (True, False), (False, True)):
            dw = _full(D + 1)
            dx32, dx16, _ = cs.rms(k, dres, o32, o16, dw=dw)
            if o32:
                dx_ok("rms_dx", dx32, r32)
            if o16:
                _bf16_ok(dx16, r16, "rms dx16")
                both16 = dx16 if both16 is None else both16
                assert torch.equal(_bits(dx16), _bits(both16))          # the same with and without dx32
            col_ok("rms_dw", dw[:D], rdw, r_terms)
            assert float(dw[D]) == FILL
        # dw_beta = 1 accumulates onto what dw holds
        pre = torch.randn(D, generator=torch.Generator().manual_seed(5))
        dw = torch.cat([pre, torch.full((1,), FILL)]).cuda()
        cs.rms(k, dres, True, False, dw=dw, beta=1.0)
        col_ok("rms_dw_beta1", dw[:D], rdw + pre.double(), torch.cat([r_terms, pre.double()[None]]))
        assert float(dw[D]) == FILL
        l32, l16, ldg, ldb, lds = cs.ln_ref(dres)
        both16 = None
        for with_dsum in (False, True):
            for o32, o16 in ((True, True), (True, False), (False, True)):
                dg, db, ds = _full(D + 1), _full(D + 1), _full(D + 1)
                dx32, dx16, _ = cs.ln(k, dres, o32, o16, dg=dg, db=db, dsum=ds if with_dsum else None)
                if o32:
                    dx_ok("ln_dx", dx32, l32)
                if o16:
                    _bf16_ok(dx16, l16, "ln dx16")
                    both16 = dx16 if both16 is None else both16
                    assert torch.equal(_bits(dx16), _bits(both16))
                col_ok("ln_dgamma", dg[:D], ldg, l_terms[0])
                col_ok("ln_dbeta", db[:D], ldb, l_terms[1])
                if with_dsum:
                    col_ok("ln_dsum", ds[:D], lds, l_terms[2])
                else:
                    assert bool((ds == FILL).all())
                assert float(dg[D]) == FILL == float(db[D]) and float(ds[D]) == FILL
    yard = {kind: max(nr.fp32_errors(D, rows, dr)[kind] for dr in (False, True)) for kind in ("dx", "colsum")}
    print(f"norm bwd D={D} rows={rows}: " + " ".join(f"{n} {v:.2e}" for n, v in rec.items()) +
          f" | fp32 torch here dx {yard['dx']:.2e} colsum {yard['colsum']:.2e}"
          f" | bounds dx {nr.bound('dx'):.2e} colsum {nr.bound('colsum'):.2e}")
    parity_report.setdefault("norm_bwd_rel_err", {})[f"{D}x{rows}"] = {
        "kernel": rec, "torch_fp32_this_case": yard, "yardstick": dict(nr.yardstick()),
        "bound": {kind: nr.bound(kind) for kind in ("dx", "colsum")}}
    for name, e in rec.items():
        kind = "dx" if name.endswith("_dx") else "colsum"
        assert e <= nr.bound(kind), (name, e, nr.bound(kind))


# --------------------------------------------------------------------------- B
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("D", [256, 1024])
def test_dropout_hooks_at_other_widths(k, cases, D, p):
    rows = 13
    cs, dr = cases(D, rows), Drop(k, p)
    c = cs.c
    m_dy, m32, m16 = (dr.mult(s, rows, D) for s in (40, 41, 42))
    assert 0 < int((m32 == 0).sum()) < rows * D

    def zeros_ok(got, mult, ref, what):
        got = got.float().cpu()
        assert bool((got[mult == 0] == 0).all()), what                       # exactly zero where dropped
        stray = (got == 0) & (mult != 0)
        assert bool((ref[stray] == 0).all()), what                           # and nowhere else

    dw = _full(D + 1)
    dx32, dx16, _ = cs.rms(k, True, True, True, dw=dw, drops=(dr.ptr(40), dr.ptr(41), dr.ptr(42)))
    r32, r16, rdw = cs.rms_ref(True, m_dy, m32, m16)
    assert nr.rel_rows(dx32.cpu(), r32) <= nr.bound("dx")
    _bf16_ok(dx16, r16, "rms dx16")
    assert nr.rel_cols(dw[:D].cpu(), rdw, nr.rms_terms(c["x"], cs.rs_c, c["dy"], m_dy)) <= nr.bound("colsum")
    zeros_ok(dx32, m32, r32, "rms dx32")
    zeros_ok(dx16, m16, r16, "rms dx16")
    # drop_dy alone: the mask reaches dx through dy (and the row sum), dw through its terms
    dx32, _, _ = cs.rms(k, False, True, False, dw=dw, drops=(dr.ptr(40), None, None))
    r32, _, rdw = cs.rms_ref(False, m_dy)
    assert nr.rel_rows(dx32.cpu(), r32) <= nr.bound("dx")
    assert nr.rel_cols(dw[:D].cpu(), rdw, nr.rms_terms(c["x"], cs.rs_c, c["dy"], m_dy)) <= nr.bound("colsum")
    # LayerNorm: the mask is on the branch gradient (dx16, dsum) alone
    dg, db, ds = _full(D + 1), _full(D + 1), _full(D + 1)
    dx32, dx16, _ = cs.ln(k, True, True, True, dg=dg, db=db, dsum=ds, drop=dr.ptr(42))
    l32, l16, ldg, ldb, lds = cs.ln_ref(True, m16)
    terms = nr.ln_terms(c["x"], cs.mu_c, cs.lrs_c, c["w"], c["dy"], m16)
    assert nr.rel_rows(dx32.cpu(), l32) <= nr.bound("dx")
    _bf16_ok(dx16, l16, "ln dx16")
    zeros_ok(dx16, m16, l16, "ln dx16")
    assert not bool((dx32 == 0).any())                                       # dx32 carries no mask
    for got, ref, t in ((dg, ldg, terms[0]), (db, ldb, terms[1]), (ds, lds, terms[2])):
        assert nr.rel_cols(got[:D].cpu(), ref, t) <= nr.bound("colsum")
    # dx16 only + dsum: the same bits, the same sums
    ds2 = _full(D + 1)
    _, dx16b, _ = cs.ln(k, False, False, True, dg=dg, db=db, dsum=ds2, drop=dr.ptr(42))
    assert torch.equal(_bits(dx16), _bits(dx16b)) and torch.equal(ds, ds2)


# --------------------------------------------------------------------------- C
@pytest.mark.parametrize("D", nr.WIDTHS)
def test_bf16_outputs_round_the_fp32_ones(k, cases, D):
    rows = 13
    cs, dr = cases(D, rows), Drop(k, 0.1)
    for dres in (False, True):
        for drops in ((None, None, None), (None, dr.ptr(41), dr.ptr(41)), (dr.ptr(40), dr.ptr(42), dr.ptr(42))):
            dx32, dx16, _ = cs.rms(k, dres, True, True, dw=_full(D), drops=drops)
            assert torch.equal(_bits(dx16), _bits(dx32.to(torch.bfloat16))), (dres, drops)
        plain, _, _ = cs.ln(k, False, True, False, dg=_full(D), db=_full(D))
        _, dx16, _ = cs.ln(k, dres, True, True, dg=_full(D), db=_full(D))
        assert torch.equal(_bits(dx16), _bits(plain.to(torch.bfloat16))), dres
        m = dr.mult(42, rows, D).cuda()
        _, dx16, _ = cs.ln(k, dres, True, True, dg=_full(D), db=_full(D), drop=dr.ptr(42))
        assert torch.equal(_bits(dx16), _bits((plain * m).to(torch.bfloat16))), dres


# --------------------------------------------------------------------------- D
@pytest.mark.parametrize("rows", [13, 136, 264])
@pytest.mark.parametrize("D", nr.WIDTHS)
def test_deferred_norm_reductions_equal_immediate(k, cases, D, rows):
    cs, dr = cases(D, rows), Drop(k, 0.1)
    parts = k.load().vqa_norm_bwd_parts(rows)
    assert k.load().vqa_norm_bwd_workspace_floats(rows, D) == 3 * parts * D
    drops = (dr.ptr(40), dr.ptr(41), dr.ptr(42))
    # RMSNorm: dw = NULL, then one job over ws [parts][D]
    dw_i = _full(D + 1)
    i32, i16, _ = cs.rms(k, True, True, True, dw=dw_i, drops=drops)
    d32, d16, ws = cs.rms(k, True, True, True, dw=None, drops=drops)
    assert torch.equal(i32, d32) and torch.equal(_bits(i16), _bits(d16))
    assert bool((ws[parts * D:] == FILL).all())                  # partial rows only; guard tail untouched
    before = ws.clone()
    dw_d = _full(D + 1)
    _run_jobs(k, [(ws.data_ptr(), dw_d.data_ptr(), D, parts, D, 0.0)])
    assert torch.equal(dw_i, dw_d) and float(dw_d[D]) == FILL and torch.equal(ws, before)
    # LayerNorm: dgamma = dbeta = NULL, dsum only flags the third slot of ws [parts][3][D]
    for with_dsum in (True, False):
        gi, bi, si = _full(D + 1), _full(D + 1), _full(D + 1)
        i32, i16, _ = cs.ln(k, True, True, True, dg=gi, db=bi, dsum=si if with_dsum else None, drop=drops[2])
        flag = _full(D + 1)
        d32, d16, ws = cs.ln(k, True, True, True, dg=None, db=None, dsum=flag if with_dsum else None, drop=drops[2])
        assert torch.equal(i32, d32) and torch.equal(_bits(i16), _bits(d16))
        assert bool((flag == FILL).all())                        # the flag pointer is never written
        w3 = ws[:3 * parts * D].view(parts, 3, D)
        assert bool((ws[3 * parts * D:] == FILL).all())
        assert not bool((w3[:, :2] == FILL).any())
        assert bool((w3[:, 2] == FILL).all()) != with_dsum       # third slot written iff dsum is given
        outs = [_full(D + 1) for _ in range(3)]
        n = 3 if with_dsum else 2
        _run_jobs(k, [(ws.data_ptr() + 4 * j * D, outs[j].data_ptr(), 3 * D, parts, D, 0.0) for j in range(n)])
        for got, want in list(zip(outs, (gi, bi, si)))[:n]:
            assert torch.equal(got, want)


@pytest.mark.parametrize("bf16", [False, True])
def test_deferred_colsum_equals_immediate(k, bf16):
    lib = k.load()
    rows, cols = 200, 772
    parts = lib.vqa_colsum_parts(rows)
    assert parts == -(-rows // 64) and lib.vqa_colsum_workspace_floats(rows, cols) == parts * cols
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(3)).cuda()
    x = x.to(torch.bfloat16) if bf16 else x
    out_i, ws_i = _full(cols + 1), _full(parts * cols + GUARD)
    _call(k, "vqa_colsum", x, int(bf16), rows, cols, cols, out_i, 0.0, ws_i)
    out_d, ws_d = _full(cols + 1), _full(parts * cols + GUARD)
    _call(k, "vqa_colsum", x, int(bf16), rows, cols, cols, None, 0.0, ws_d)
    torch.cuda.synchronize()
    assert torch.equal(ws_i, ws_d) and bool((ws_d[parts * cols:] == FILL).all())
    assert not bool((ws_d[:parts * cols] == FILL).any())
    _run_jobs(k, [(ws_d.data_ptr(), out_d.data_ptr(), cols, parts, cols, 0.0)])
    assert torch.equal(out_i, out_d) and float(out_d[cols]) == FILL
    ref = x.double().sum(0).cpu()
    assert float(((out_d[:cols].double().cpu() - ref).abs() / x.double().abs().sum(0).cpu()).max()) <= 2.0 ** -21


# --------------------------------------------------------------------------- E
def _ints(shape, seed, even=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-4, 5, shape, generator=g) * 2 if even else torch.randint(-8, 9, shape, generator=g)
    return t


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
def test_colsum_is_exact_on_integers(k, bf16, pad):
    lib = k.load()
    dt = torch.bfloat16 if bf16 else torch.float32
    for rows in (1, 63, 64, 65, 200):
        for cols in (4, 252, 256, 260, 772):
            ld, c0 = (cols + 12, 4) if pad else (cols, 0)
            xi = _ints((rows, cols), 100 * rows + cols)
            big = torch.full((rows, ld), 1000.0)                  # beside the slice: would spoil any sum that read it
            big[:, c0:c0 + cols] = xi.float()
            x = big.to(dt).cuda()
            keep = x.clone()
            ws = _full(lib.vqa_colsum_workspace_floats(rows, cols) + GUARD)
            o0 = _ints((cols,), 7 * rows + cols)
            for beta in (0.0, 1.0):
                out = torch.cat([o0.float(), torch.full((1,), FILL)]).cuda()
                _call(k, "vqa_colsum", x.data_ptr() + c0 * x.element_size(), int(bf16), rows, cols, ld, out, beta, ws)
                torch.cuda.synchronize()
                want = xi.sum(0) + (o0 if beta else 0)
                assert torch.equal(out[:cols].cpu(), want.float()), (rows, cols, beta)
                assert float(out[cols]) == FILL and torch.equal(x, keep)
                assert bool((ws[lib.vqa_colsum_workspace_floats(rows, cols):] == FILL).all())


PARTS, COLS = (1, 15, 16, 17, 49), (1, 63, 64, 65, 1000)


def test_colsum_partials_and_batch_sum_are_exact_on_integers(k):
    for parts in PARTS:
        for cols in COLS:
            stride = cols + 3
            xi = _ints((parts, cols), 1000 * parts + cols)
            wide = torch.full((parts, stride), 1000.0)
            wide[:, :cols] = xi.float()
            wide, dense = wide.cuda(), xi.float().cuda()
            o0 = _ints((cols,), parts + cols, even=True)
            for beta in (0.0, 1.0, 0.5):
                want = (xi.sum(0).double() + beta * o0.double()).float()
                for name, args in (("vqa_colsum_partials", (wide, parts, stride, cols)),
                                   ("vqa_batch_sum", (dense, parts, cols))):
                    out = torch.cat([o0.float(), torch.full((1,), FILL)]).cuda()
                    _call(k, name, *args, out, beta)
                    torch.cuda.synchronize()
                    assert torch.equal(out[:cols].cpu(), want), (name, parts, cols, beta)
                    assert float(out[cols]) == FILL


def _job_list(make):
    """The batched launch's job list over tensors from make(shape, seed): [(ws tensor, float offset,
    stride, parts, cols, beta)].  First job: one block; last: the most (2304 columns, 36 blocks)."""
    jobs, seed = [], [0]

    def data(*shape):
        seed[0] += 1
        return make(shape, seed[0])
    for i, (parts, cols) in enumerate([(17, 1), (1, 63), (15, 64), (16, 65), (49, 1000), (17, 64), (49, 63),
                                       (1, 1000), (16, 1), (15, 65), (49, 65), (17, 1000)]):
        jobs.append((data(parts, cols + 3), 0, cols + 3, parts, cols, (0.0, 1.0, 0.5)[i % 3]))
    ln = data(5, 3, 256)                                          # the LayerNorm layout ws[(p*3 + k)*D + c]
    jobs += [(ln, j * 256, 3 * 256, 5, 256, 0.0) for j in range(3)]
    ln = data(33, 3, 512)
    jobs += [(ln, j * 512, 3 * 512, 33, 512, 0.0) for j in range(3)]
    for parts, cols, beta in ((33, 768, 0.0), (4, 8, 1.0), (64, 1, 0.0), (2, 768, 0.5), (32, 8, 0.0), (4, 2304, 1.0)):
        jobs.append((data(parts, cols), 0, cols, parts, cols, beta))
    assert len(jobs) >= 24 and jobs[0][4] <= 64 and jobs[-1][4] == max(j[4] for j in jobs)
    return jobs


def _arena(jobs, make):
    """Outputs back to back, one guard float after each: (arena, [float offset of each output])."""
    offs, n = [], 0
    for j in jobs:
        offs.append(n)
        n += j[4] + 1
    arena = make((n,), 999)
    for o, j in zip(offs, jobs):
        arena[o + j[4]] = FILL
    return arena, offs


def _launch_list(k, jobs, arena, offs):
    _run_jobs(k, [(ws.data_ptr() + 4 * off, arena.data_ptr() + 4 * o, stride, parts, cols, beta)
                  for (ws, off, stride, parts, cols, beta), o in zip(jobs, offs)])


def _job_view(job):
    ws, off, stride, parts, cols, _ = job
    return ws.reshape(-1)[off:].as_strided((parts, cols), (stride, 1))


def test_colsum_batched_is_exact_on_integers(k):
    jobs = _job_list(lambda shape, seed: _ints(shape, seed).float().cuda())
    arena, offs = _arena(jobs, lambda shape, seed: _ints(shape, seed, even=True).float().cuda())
    before = arena.clone()
    _launch_list(k, jobs, arena, offs)
    for j, o in zip(jobs, offs):
        cols, beta = j[4], j[5]
        want = _job_view(j).double().sum(0) + beta * before[o:o + cols].double()
        assert torch.equal(arena[o:o + cols], want.float()), j[2:]
        assert float(arena[o + cols]) == FILL
    # a one-job launch
    j = jobs[4]
    out = _full(j[4] + 1)
    _launch_list(k, [j[:5] + (0.0,)], out, [0])
    assert torch.equal(out[:j[4]], _job_view(j).double().sum(0).float()) and float(out[j[4]]) == FILL


def test_colsum_batched_on_randn_matches_partials_and_fp64(k, parity_report):
    make = lambda shape, seed: torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()
    jobs = _job_list(make)
    arena, offs = _arena(jobs, make)
    before = arena.clone()
    _launch_list(k, jobs, arena, offs)
    kern, yard = 0.0, 0.0
    for j, o in zip(jobs, offs):
        ws, off, stride, parts, cols, beta = j
        one = before[o:o + cols + 1].clone()
        _call(k, "vqa_colsum_partials", ws.data_ptr() + 4 * off, parts, stride, cols, one, beta)
        torch.cuda.synchronize()
        assert torch.equal(arena[o:o + cols + 1], one), j[2:]     # bit-equal to the job done alone
        v, o0 = _job_view(j).cpu(), before[o:o + cols].cpu()
        ref = v.double().sum(0) + beta * o0.double()
        norm = v.double().abs().sum(0) + abs(beta) * o0.double().abs()
        t32 = v.sum(0) + beta * o0 if beta else v.sum(0)
        kern = max(kern, float(((arena[o:o + cols].cpu().double() - ref).abs() / norm).max()))
        yard = max(yard, float(((t32.double() - ref).abs() / norm).max()))
    # one yardstick for the list (the largest torch-fp32 error of any job): a single job of one or
    # eight columns can be exact by luck in either order
    print(f"colsum batched on randn: kernel {kern:.3e}, torch fp32 {yard:.3e}")
    parity_report["colsum_rel_err"] = {"kernel": kern, "torch_fp32": yard}
    assert kern <= 4 * yard, (kern, yard)


@pytest.mark.parametrize("causal", [False, True])
def test_relbias_bwd_is_exact_on_integers(k, pkg, causal):
    heads, nb = 12, 32
    n = 20 if causal else 32
    bucket = torch.from_numpy(pkg.layout.t5_bucket_map(n, n).astype(np.int32))
    if causal:
        bucket[torch.triu(torch.ones(n, n, dtype=torch.bool), 1)] = -1
    hit = torch.unique(bucket[bucket >= 0])
    assert 0 < len(hit) < nb                                      # some buckets are never hit
    dbias = _ints((heads, n * n), 77 + n)
    want = torch.zeros(nb, heads, dtype=torch.int64)
    live = (bucket >= 0).view(-1)
    want.index_add_(0, bucket.view(-1)[live].long(), dbias.t()[live])
    dtab = _full(nb * heads + 1)
    _call(k, "vqa_t5_relbias_bwd", dbias.float().cuda(), bucket.cuda(), dtab, heads, n, n, nb)
    torch.cuda.synchronize()
    assert torch.equal(dtab[:nb * heads].cpu().view(nb, heads), want.float())
    assert float(dtab[nb * heads]) == FILL


# --------------------------------------------------------------------------- F
@pytest.mark.parametrize("T", [1, 33, 300])
@pytest.mark.parametrize("D", [132, 768])
def test_embedding_zero_rows_keeps_the_table_sparse(k, D, T):
    vocab = 1000
    g = torch.Generator().manual_seed(T + D)
    steps = []
    for s in range(3):
        ids = torch.randint(0, vocab, (T,), generator=g)
        if s and T > 1:
            ids[:T // 3] = steps[-1][T // 3:2 * (T // 3)]         # overlap with the previous step
        if T > 8:
            ids[-(T // 4):] = 0                                   # a run of the pad id
            ids[T // 2] = ids[T // 2 - 1]                         # a duplicate
        steps.append(ids)
    steps[2][0] = vocab - 1
    table = torch.zeros(vocab * D + 1, device="cuda")
    table[vocab * D] = FILL
    prev = torch.zeros(T, dtype=torch.int64, device="cuda")
    ws = torch.zeros(3 * T, dtype=torch.int32, device="cuda")
    for s, ids in enumerate(steps):
        dh = _ints((T, D), 10 * T + s)
        cur = ids.cuda()
        _call(k, "vqa_embedding_zero_rows", prev, cur, T, table, D, vocab)
        _call(k, "vqa_embedding_bwd", cur, dh.float().cuda(), table, T, D, vocab, ws)
        torch.cuda.synchronize()
        want = torch.zeros(vocab, D, dtype=torch.int64).index_add_(0, ids, dh)
        assert torch.equal(table[:vocab * D].cpu().view(vocab, D), want.float()), s
        assert torch.equal(prev, cur) and float(table[vocab * D]) == FILL
    _call(k, "vqa_embedding_zero_rows", prev, None, T, table, D, vocab)
    torch.cuda.synchronize()
    assert torch.equal(prev.cpu(), steps[2]) and not bool(table[:vocab * D].any())


# --------------------------------------------------------------------------- G
def test_bad_arguments_are_refused_and_write_nothing(k):
    inv = _err_invalid()
    rows, D = 8, 256
    f = _full
    x, w, dy, st = f(rows, 1280), f(1280), f(rows, 1280), f(rows)
    outs = [f(rows, 1280), f(rows, 1280, dtype=torch.bfloat16), f(1280), f(1280), f(1280), f(3 * rows * 1280)]
    dx32, dx16, g1, g2, g3, ws = outs
    dr = Drop(k, 1.0)
    bad = []
    for d, r in [(0, rows), (128, rows), (300, rows), (1280, rows), (D, 0), (D, -1)]:
        bad += [("vqa_rmsnorm_fwd", (x, w, dx32, dx16, g1, r, d, 1e-6, None)),
                ("vqa_rmsnorm_bwd", (dy, x, st, w, None, dx32, dx16, g1, 0.0, ws, r, d, None, None, None)),
                ("vqa_rmsnorm_bwd", (dy, x, st, w, None, dx32, dx16, None, 0.0, ws, r, d, None, None, None)),
                ("vqa_layernorm_fwd", (x, w, w, dx32, dx16, g1, g2, r, d, 1e-5)),
                ("vqa_layernorm_bwd", (dy, x, st, st, w, None, dx32, dx16, g1, g2, ws, r, d, None, g3)),
                ("vqa_layernorm_bwd", (dy, x, st, st, w, None, dx32, dx16, None, None, ws, r, d, None, g3))]
    p1 = dr.ptr(40)
    bad += [("vqa_rmsnorm_fwd", (x, w, dx32, dx16, g1, rows, D, 1e-6, p1)),
            ("vqa_rmsnorm_bwd", (dy, x, st, w, None, dx32, dx16, g1, 0.0, ws, rows, D, p1, None, None)),
            ("vqa_rmsnorm_bwd", (dy, x, st, w, None, dx32, dx16, g1, 0.0, ws, rows, D, None, p1, None)),
            ("vqa_rmsnorm_bwd", (dy, x, st, w, None, dx32, dx16, g1, 0.0, ws, rows, D, None, None, p1)),
            ("vqa_layernorm_bwd", (dy, x, st, st, w, None, dx32, dx16, g1, g2, ws, rows, D, p1, g3)),
            ("vqa_layernorm_bwd", (dy, x, st, st, w, None, dx32, dx16, g1, None, ws, rows, D, None, g3)),
            ("vqa_layernorm_bwd", (dy, x, st, st, w, None, dx32, dx16, None, g2, ws, rows, D, None, g3)),
            ("vqa_colsum", (x, 0, rows, 6, 1280, g1, 0.0, ws)),
            ("vqa_colsum", (x, 0, 0, 8, 1280, g1, 0.0, ws)),
            ("vqa_colsum", (x, 0, -1, 8, 1280, None, 0.0, ws)),
            ("vqa_colsum", (x, 0, rows, 0, 1280, g1, 0.0, ws)),
            ("vqa_colsum_batched", (ws, 0, 1)),
            ("vqa_colsum_batched", (ws, 1, 0))]
    for name, args in bad:
        assert _rc(k, name, *args) == inv, (name, args[-8:])
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == FILL).all())
