"""The attention kernels (csrc/attention.hip, csrc/attention_mfma.hip) against tests/attn_ref.py in
fp64: all 30 MFMA instantiations (dh 64 / 96 / 128 x 1..5 key tiles, forward and backward), the VALU
kernels up to their LDS limit, the long forward up to its 1024 keys, vqa_attn_probs.

Bound: 4 x attn_ref.yardstick(path) per tensor -- the largest error, against fp64 and relative to the
sum of the magnitudes behind each element (attn_ref.normalisers), of the same chain evaluated by torch
on the CPU in fp32 with the path's roundings, over the path's own case table.  Nothing a kernel computed
enters a bound; tests/test_attn_ref_cpu.py shows that every one of 17 plausible kernel mistakes sits at
least 7.7 bounds away on these same inputs.

Every output lies inside a larger buffer of sentinels (o / dq / dk / dv with a row pitch of D + 4 and
guard rows, P / dbias / the bias gradient with guard tails) and everything outside the written region
must still hold the sentinel; q | k | v come from one fused buffer of pitch 3 D + 8 whose unused
elements are NaN.  (batch, heads) is (3, 1) or (1, 3) but for a few (2, 2): an odd number of pairs, so
the last two-wave block of the NT <= 2 kernels has a dead second wave.  vqa_attn_path is asserted
before each run.

Measured on an MI355X (profiles/attn_parity.json; largest error over a path's cases / its bound, the
factor 4 never raised and no __expf term needed):
  MFMA (83 cases)  o 6.52e-3 / 2.61e-2   dq 4.57e-3 / 1.83e-2   dk 6.19e-3 / 2.48e-2   dv 7.50e-3 / 3.00e-2
                   p 2.97e-7 / 1.19e-6   ds 1.42e-6 / 7.17e-6   bias gradient 2.1e-7 .. 1.19e-6 / 7.17e-6
  VALU (8 cases)   o 3.69e-3 / 1.48e-2   dq 2.48e-3 / 9.91e-3   dk 2.85e-3 / 1.14e-2   dv 3.16e-3 / 1.26e-2
                   p 1.62e-7 / 8.97e-7   ds 1.53e-6 / 5.17e-6
  long (12 cases)  o 9.9e-4 (5 x 1024) .. 3.65e-3 / 1.49e-2
  vqa_attn_probs   p 1.01e-7 .. 1.72e-7 / 8.75e-7
The bf16 outputs reach their yardstick itself: there the error is the rounding of the stored value, which
the kernel and the model share; the least errors are exact zeros (one key: P = 1, dS = 0).
"""
import ctypes
import os
import re

import pytest
import torch

import attn_ref as ar

pytestmark = pytest.mark.gpu
FILL = -7.0                                    # sentinel of every output and guard (exact in bf16)
GROWS = 2                                      # guard rows before and after a bf16 output
TAIL = 64                                      # guard floats before and after an fp32 output
NAN = float("nan")


@pytest.fixture(scope="module")
def k(pkg):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pkg.lib.load()
    return pkg.lib


def _err_invalid():
    from __graft_entry__ import ROOT
    return int(re.search(r"#define VQA_ERR_INVALID (\d+)", open(os.path.join(ROOT, "include", "vqa_hip.h")).read()).group(1))


def _addr(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


class Run:
    """The device buffers and the descriptor of one case.  save_p / dbias False: that pointer NULL;
    train: rng[2], the training flag of vqa_dropout."""

    def __init__(self, L, s, save_p=True, dbias=True, train=1):
        self.L, self.s, c = L, s, ar.make_case(s)
        B, H, lq, lk, dh = s.B, s.H, s.lq, s.lk, s.dh
        D = H * dh
        self.D, self.ldi, self.ldo, self.lddo = D, 3 * D + 8, D + 4, D + 8
        dev = "cuda"
        fused = torch.full((B * max(lq, lk), self.ldi), NAN, dtype=torch.bfloat16)
        fused[:B * lq, :D] = ar.rows(c["q"])
        fused[:B * lk, D:2 * D] = ar.rows(c["k"])
        fused[:B * lk, 2 * D:3 * D] = ar.rows(c["v"])
        do = torch.full((B * lq, self.lddo), NAN, dtype=torch.bfloat16)
        do[:, :D] = ar.rows(c["do"])
        self.fused, self.do = fused.to(dev), do.to(dev)
        self.bias = None if c["bias"] is None else c["bias"].to(dev)
        self.mask = None if c["mask"] is None else c["mask"].to(dev)
        self.n = B * H * lq * lk
        self.out16 = {t: torch.full((B * L_ + 2 * GROWS, self.ldo), FILL, device=dev, dtype=torch.bfloat16)
                      for t, L_ in (("o", lq), ("dq", lq), ("dk", lk), ("dv", lk))}
        self.out32 = {t: torch.full((self.n + 2 * TAIL,), FILL, device=dev) for t in ("p", "ds")}
        self.rng = torch.tensor([ar.SEED, ar.COUNTER, train], dtype=torch.int32, device=dev)
        d = self.d = L.AttnDesc()
        d.q, d.k, d.v = _addr(self.fused), _addr(self.fused, D), _addr(self.fused, 2 * D)
        d.ldq = d.ldk = d.ldv = self.ldi
        d.o, d.ldo = _addr(self.out16["o"], GROWS * self.ldo), self.ldo
        d.p = _addr(self.out32["p"], TAIL) if save_p else None
        d.bias, d.key_mask = _addr(self.bias), _addr(self.mask)
        d.batch, d.heads, d.lq, d.lk, d.dh, d.scale = B, H, lq, lk, dh, c["scale"]
        if s.p:
            d.drop = L.Dropout(s.p, ar.SITE, self.rng.data_ptr())
        self.want_dbias = dbias

    def set_bwd(self):
        d = self.d
        d.dout, d.lddo = _addr(self.do), self.lddo
        for t in ("dq", "dk", "dv"):
            setattr(d, t, _addr(self.out16[t], GROWS * self.ldo))
        d.lddq = d.lddk = d.lddv = self.ldo
        d.dbias = _addr(self.out32["ds"], TAIL) if self.want_dbias else None

    def path(self, backward):
        return self.L.load().vqa_attn_path(ctypes.byref(self.d), backward)

    def fwd(self):
        return self.L.load().vqa_attn_fwd(ctypes.byref(self.d), self.L.stream_handle())

    def bwd(self):
        return self.L.load().vqa_attn_bwd(ctypes.byref(self.d), self.L.stream_handle())

    def probs(self):
        return self.L.load().vqa_attn_probs(ctypes.byref(self.d), self.L.stream_handle())

    def result(self, tensors):
        """The named outputs as CPU [B, H, ., .] tensors, after checking that every OTHER element of
        every output buffer still holds the sentinel."""
        torch.cuda.synchronize()
        s, got = self.s, {}
        for t, buf in self.out16.items():
            host = buf.cpu()
            L_ = s.lq if t in ("o", "dq") else s.lk
            if t in tensors:
                got[t] = ar.unrows(host[GROWS:-GROWS, :self.D].float(), s.B, s.H, L_, s.dh).contiguous()
                host[GROWS:-GROWS, :self.D] = FILL
            assert bool((host == FILL).all()), f"{ar.name(s)}: {t} written outside its region"
        for t, buf in self.out32.items():
            host = buf.cpu()
            if t in tensors:
                got[t] = host[TAIL:-TAIL].view(s.B, s.H, s.lq, s.lk).clone()
                host[TAIL:-TAIL] = FILL
            assert bool((host == FILL).all()), f"{ar.name(s)}: {t} written outside its region"
        return got


PATH_CODE = {ar.MFMA: "ATTN_MFMA", ar.LONG: "ATTN_LONG", ar.VALU: "ATTN_VALU"}


def run_case(L, s, **kw):
    """Forward (+ backward unless the path is the long forward) of one case on the path it is meant
    for; every output as CPU tensors."""
    r = Run(L, s, save_p=s.path != ar.LONG, **kw)
    code = getattr(L, PATH_CODE[s.path])
    assert r.path(0) == code, ar.name(s)
    L.check(r.fwd(), "vqa_attn_fwd")
    if s.path == ar.LONG:
        return r.result(("o",))
    r.set_bwd()
    assert r.path(1) == code, ar.name(s)
    L.check(r.bwd(), "vqa_attn_bwd")
    return r.result(ar.TENSORS if r.want_dbias else ("o", "p", "dq", "dk", "dv"))


def check(s, got, report):
    """Each checked tensor within its bound; the figures are printed and recorded first."""
    errs = ar.errors(s, got)
    line = {t: f"{e:.2e}/{ar.bound(s.path, t):.2e}" for t, e in errs.items()}
    print(ar.name(s), line)
    rec = report.setdefault("attn_parity_rel_err", {}).setdefault(s.path, {})
    rec[ar.name(s)] = errs
    report["attn_parity_bounds"] = {p: {t: ar.bound(p, t) for t in ar.checked(p)}
                                    for p in (ar.MFMA, ar.VALU, ar.LONG, ar.PROBS)}
    for t, e in errs.items():
        assert e <= ar.bound(s.path, t), (ar.name(s), t, e, ar.bound(s.path, t))
    if "p" in got:                                         # rows of P sum to 1
        dev = (got["p"].double().sum(-1) - 1).abs().max()
        assert float(dev) <= s.lk * 2.0 ** -23, (ar.name(s), float(dev))


def check_mask_rows(s, got):
    """Partially masked rows are exactly 0 at their masked keys; a fully masked row is exactly
    float32(1) / float32(lk)."""
    uniform = (torch.ones(1) / torch.full((1,), float(s.lk))).item()
    for b, n in enumerate(s.lens or ()):
        if n == 0:
            assert bool((got["p"][b] == uniform).all()), (ar.name(s), b)
        else:
            assert bool((got["p"][b, :, :, n:] == 0).all()), (ar.name(s), b)


# ------------------------------------------------------------------------------------ A. MFMA sweep
@pytest.mark.parametrize("dh,nt", sorted(ar.SWEEP))
def test_mfma_sweep(k, parity_report, dh, nt):
    for s in ar.SWEEP[(dh, nt)]:
        check(s, run_case(k, s), parity_report)


# ------------------------------------------------------------------------- B. bias and mask (MFMA)
@pytest.mark.parametrize("s", ar.BIAS, ids=ar.name)
def test_mfma_bias_and_mask(k, parity_report, s):
    got = run_case(k, s)
    check(s, got, parity_report)
    check_mask_rows(s, got)
    if s.bias:
        check_bias_gradient(k, s, got, parity_report)


def check_bias_gradient(L, s, got, report):
    """vqa_batch_sum of the per-sample dS against the fp64 bias gradient, within the dS bound of the
    summed normalisers (B samples of it)."""
    ref, norm = ar._ref_cached(s)
    n = s.H * s.lq * s.lk
    ds = got["ds"].cuda().contiguous()
    red = torch.full((n + 2 * TAIL,), FILL, device="cuda")
    L.check(L.load().vqa_batch_sum(ds.data_ptr(), s.B, n, _addr(red, TAIL), 0.0, L.stream_handle()), "vqa_batch_sum")
    torch.cuda.synchronize()
    host = red.cpu()
    e = ar.rel_err(host[TAIL:-TAIL].view(s.H, s.lq, s.lk), ref["ds"].sum(0), norm["ds"].sum(0))
    host[TAIL:-TAIL] = FILL
    assert bool((host == FILL).all())
    print(ar.name(s), f"bias gradient {e:.2e}/{ar.bound(s.path, 'ds'):.2e}")
    report.setdefault("attn_parity_bias_gradient", {})[ar.name(s)] = e
    assert e <= ar.bound(s.path, "ds"), (ar.name(s), e)


# ------------------------------------------------------------------------------------------ C. VALU
@pytest.mark.parametrize("s", ar.VALU_CASES, ids=ar.name)
def test_valu(k, parity_report, s):
    got = run_case(k, s)
    check(s, got, parity_report)
    check_mask_rows(s, got)
    if s.bias:
        check_bias_gradient(k, s, got, parity_report)


def _refused(r, rc):
    """The call returned VQA_ERR_INVALID and no output element was written."""
    assert rc == _err_invalid(), (rc, r.L.load().vqa_last_error())
    assert r.result(()) == {}


def test_valu_lds_limit(k):
    """bwd_smem(64, 64, 64) = 67,072 B: refused, nothing launched (63 x 63 x 64, 65,520 B, runs: VALU_CASES);
    fwd_smem(64, 64, 256) = 115,712 B likewise."""
    r = Run(k, ar.Spec(ar.VALU, 1, 1, 64, 64, 64, None, None, 0.0))
    r.out32["p"][TAIL:-TAIL] = 1.0 / 64                    # a saved P for the backward to read, were it to run
    r.set_bwd()
    assert r.path(1) == k.ATTN_VALU
    rc = r.bwd()
    r.out32["p"][TAIL:-TAIL] = FILL
    _refused(r, rc)
    r = Run(k, ar.Spec(ar.VALU, 1, 1, 64, 64, 256, None, None, 0.0))
    assert r.path(0) == k.ATTN_VALU
    _refused(r, r.fwd())


# --------------------------------------------------------------------------------- D. long forward
@pytest.mark.parametrize("s", ar.LONG_CASES, ids=ar.name)
def test_long_forward(k, parity_report, s):
    check(s, run_case(k, s), parity_report)


def test_long_forward_key_limit(k):
    r = Run(k, ar.Spec(ar.LONG, 1, 1, 5, 1025, 64, None, None, 0.0), save_p=False)
    assert r.path(0) == k.ATTN_VALU                        # no kernel takes it: the VALU check refuses
    _refused(r, r.fwd())


# ------------------------------------------------------------------------------ E. exact relations
EXACT = (ar.Spec(ar.MFMA, 3, 1, 20, 33, 96, None, None, 0.1), ar.Spec(ar.MFMA, 1, 3, 31, 157, 64, "rel", None, 0.1),
         ar.Spec(ar.VALU, 1, 3, 20, 31, 8, None, None, 0.1), ar.Spec(ar.VALU, 3, 1, 48, 40, 64, "rel", (40, 7, 0), 0.1))


def _same(a, b, tensors):
    for t in tensors:
        assert torch.equal(a[t], b[t]), t


@pytest.mark.parametrize("s", EXACT, ids=ar.name)
def test_exact_relations(k, s):
    base = run_case(k, s)
    _same(base, run_case(k, s), ar.TENSORS)                                # two runs, the same bits
    _same(base, run_case(k, s, dbias=False), ("o", "p", "dq", "dk", "dv"))   # dbias == NULL
    plain = s._replace(p=0.0)
    assert torch.equal(ar.make_case(plain)["q"], ar.make_case(s)["q"])
    _same(run_case(k, plain), run_case(k, s, train=0), ar.TENSORS)         # rng[2] == 0: no dropout
    if s.lq <= 32 and s.lk <= 64:                                          # p == NULL on the same path
        r = Run(k, s, save_p=False)
        assert r.path(0) == getattr(k, PATH_CODE[s.path])
        k.check(r.fwd(), "vqa_attn_fwd")
        _same(base, r.result(("o",)), ("o",))


# ------------------------------------------------------------------------------- F. vqa_attn_probs
@pytest.mark.parametrize("s", ar.PROBS_CASES, ids=ar.name)
def test_attn_probs(k, parity_report, s):
    r = Run(k, s)
    k.check(r.probs(), "vqa_attn_probs")
    got = r.result(("p",))
    assert bool(torch.isfinite(got["p"]).all())
    check(s, got, parity_report)
    check_mask_rows(s, got)
    if s.bias == "causal":                                 # the forward's uniform rows, bit for bit
        fwd = run_case(k, s._replace(path=ar.MFMA))
        pad = s.lens.index(0)
        assert torch.equal(got["p"][pad], fwd["p"][pad])


# ------------------------------------------------------------------------------------ G. refusals
REFUSE_FWD = ("q", "k", "v", "o", "ldo")
REFUSE_BWD = ("dout", "dq", "dk", "dv", "lddq", "lddk", "lddv")


@pytest.mark.parametrize("what", REFUSE_FWD + REFUSE_BWD)
def test_valu_argument_checks(k, what):
    """q / k / v / dO off 16 bytes, an output off 4 bytes, an odd output pitch: VQA_ERR_INVALID, no launch."""
    s = ar.Spec(ar.VALU, 1, 2, 33, 16, 8, None, None, 0.0)
    r = Run(k, s)
    bwd = what in REFUSE_BWD
    if bwd:
        r.out32["p"][TAIL:-TAIL] = 1.0 / s.lk
        r.set_bwd()
    d = r.d
    if what.startswith("ld"):
        setattr(d, what, getattr(d, what) + 1)             # the guard rows cover the longer pitch
    elif what in ("q", "k", "v", "dout"):
        setattr(d, what, getattr(d, what) + 8)             # 8-byte aligned only
    else:
        setattr(d, what, getattr(d, what) + 2)             # 2-byte aligned only
    assert r.path(int(bwd)) == k.ATTN_VALU
    rc = r.bwd() if bwd else r.fwd()
    r.out32["p"][TAIL:-TAIL] = FILL
    _refused(r, rc)
