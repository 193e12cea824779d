"""vqa_gemm / vqa_gemm_pair (csrc/gemm.hip, gemm_fp8.hip, conv_patch.inl) against tests/gemm_ref.py in fp64:
every tile config on every operand layout and k-tile count, the whole epilogue, batch strides, split-K,
the three implicit-im2col loader paths and the LDS-patch convolution on non-square geometries, the GELU /
tanh kernel, the e4m3 kernels, the paired launch, and the refusals.

Bound: gemm_ref.bound(group) = max(4 x yardstick, 2^-22) of |error| / normaliser, the normaliser being the
sum of the magnitudes behind each element; the yardstick is the fp32 model's own error over the group's
table.  Nothing a kernel computed enters a bound; tests/test_gemm_ref_cpu.py shows that each of 25 plausible
kernel mistakes sits at least 257 bounds away on these inputs.  A bf16 output is held to the same bound
beyond the half ulp its rounding may take (gemm_ref.errors), and must equal RNE-bf16 of the fp32 output
bit for bit wherever both are written without beta.

Every output lies in a buffer of sentinels (-7): c32 with a pitch of n + 8 (n + 3 in the scalar cases), c16
with n + 16, guard rows before and after, gaps between the batch elements; everything outside the written
region must still hold the sentinel.  Every input has its own, wider pitch with NaN in the padding.  The
first eligible config is compared with the reference, every other one with the first bit for bit (guards
included); eligible configs come from lib.gemm_config_fits / GEMM_NO_SPLITK.

Measured on an MI355X (profiles/gemm_parity.json; largest error over a group's cases / its bound; the
factor 4 is never raised and __expf needs no term):
  plain (107 cases)  1.38e-7 / 5.91e-7    split-K (20)  8.13e-8 / 3.25e-7    conv (12)  7.58e-8 / 2.60e-7
  patch (6)          8.71e-8 / 2.56e-7    GELU (3)      1.22e-7 / 6.13e-7    tanh (3)   5.41e-8 / 2.38e-7 (the floor)
  fp8 (6)            2.37e-5 / 2.31e-4
The bf16 kernels sit at their yardsticks (split-K equals the model bit for bit).  The e4m3 kernels do not
sit at an fp32 yardstick (9.6e-8): measured 2.4e-5 at k = 16, 1.4e-5 at k = 80, 5.8e-6 at k = 336.  Between
the e4m3 bytes and the accumulator the kernel has one operation, v_mfma_scale_f32_32x32x64_f8f6f4, and run
alone (unit scales, no epilogue) it drops products 2^-13 below the largest of their neighbours (256 * 1 +
2^-6 gives 256).  That loss is part of the model now (gemm_ref._mfma_e4m3, which states the measurement);
the fp8 yardstick is 5.8e-5 with it, the factor stays 4.
"""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import gemm_ref as gr

pytestmark = pytest.mark.gpu
WS_TAIL, WS_MARK = 256, 0x5A5A5A5A              # sentinel ints behind a split-K workspace
PTRS = ("a", "b", "bias", "res32", "res16", "mask16", "scale_a", "scale_b")
ESZ = {"a": 2, "b": 2, "bias": 4, "res32": 4, "res16": 2, "mask16": 2, "scale_a": 4, "scale_b": 4}


@pytest.fixture(scope="module")
def L(pkg):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pkg.lib.load()
    return pkg.lib


def _err_invalid():
    from __graft_entry__ import ROOT
    return int(re.search(r"#define VQA_ERR_INVALID (\d+)", open(os.path.join(ROOT, "include", "vqa_hip.h")).read()).group(1))


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def same(a, b):
    """Two results hold the same bits, guards included."""
    return all((a[t] is None) == (b[t] is None) and (a[t] is None or torch.equal(_bits(a[t]), _bits(b[t])))
               for t in ("c32", "c16"))


class Run:
    """The device inputs of one case; each launch gets fresh output buffers."""

    def __init__(self, L, c):
        self.L, self.c, self.I = L, c, gr.build(c)
        I = self.I
        self.dev = {k: getattr(I, k).cuda() for k in PTRS if getattr(I, k, None) is not None}
        self.rng = torch.tensor([gr.SEED, gr.COUNTER, 1], dtype=torch.int32, device="cuda")
        if c.fp8:
            self._quantise()

    def _quantise(self):
        """The e4m3 operands come from vqa_quant_rows_fp8 (into NaN-filled padded rows) and must be the
        bytes and scales the reference was built from."""
        c, I = self.c, self.I
        for t, src, rows, ld, st, sst in (("a", I.src_a, c.m, I.lda, I.stride_a, I.stride_scale_a),
                                          ("b", I.src_b, c.n, I.ldb, I.stride_b, I.stride_scale_b)):
            q = torch.full_like(self.dev[t], 127)
            s = torch.full_like(self.dev["scale_" + t], gr.NAN)
            x = src.cuda().contiguous()
            for z in range(src.shape[0]):
                self.L.call("vqa_quant_rows_fp8", x[z].data_ptr(), 0, c.k, rows, c.k, q.data_ptr() + z * st, ld,
                            s.data_ptr() + 4 * z * sst)
            torch.cuda.synchronize()
            assert torch.equal(q, self.dev[t]) and torch.equal(_bits(s), _bits(self.dev["scale_" + t])), t
            self.dev[t], self.dev["scale_" + t] = q, s

    def prepare(self, cfg=0, z=None, inplace=False):
        """(descriptor, output buffers).  z: the separate launch of batch element z.  inplace: the fp32
        residual lies in c32 itself (c32 == res32, ldres = ldc32)."""
        c, I, L = self.c, self.I, self.L
        out = {"c32": None if I.c32 is None else I.c32.cuda(), "c16": None if I.c16 is None else I.c16.cuda()}
        d = L.GemmDesc()
        zz = z or 0
        esz_ab = 1 if c.fp8 else 2
        step = {"a": I.stride_a * esz_ab, "b": I.stride_b * esz_ab, "bias": I.stride_bias * 4,
                "scale_a": getattr(I, "stride_scale_a", 0) * 4, "scale_b": getattr(I, "stride_scale_b", 0) * 4}
        for t in PTRS:
            if t in self.dev:
                first = 4 * I.bias_off if t == "bias" else 0
                setattr(d, t, self.dev[t].data_ptr() + first + zz * step.get(t, I.stride_res * ESZ[t]))
        d.lda, d.ldb, d.a_trans, d.b_trans = I.lda, I.ldb, c.at, c.bt
        d.m, d.n, d.k = c.m, c.n, c.k
        if out["c32"] is not None:
            d.c32, d.ldc32 = out["c32"].data_ptr() + 4 * (I.c32_off + zz * I.stride_c32), I.ldc32
        if out["c16"] is not None:
            d.c16, d.ldc16 = out["c16"].data_ptr() + 2 * (I.c16_off + zz * I.stride_c16), I.ldc16
        d.ldres, d.ldmask = I.ldres, I.ldmask
        d.alpha, d.beta, d.relu = c.alpha, c.beta, c.act
        if c.geom:
            g = L.ConvGeom(*c.geom)
            if c.conv:
                d.a_conv, d.ga = c.conv, g
            else:
                d.b_conv, d.gb = 1, g
        d.batch = 1 if z is not None else c.batch
        d.stride_a, d.stride_b, d.stride_c32, d.stride_c16 = I.stride_a, I.stride_b, I.stride_c32, I.stride_c16
        d.stride_res, d.stride_bias, d.drop_site_stride = I.stride_res, I.stride_bias, c.dsite
        d.config = cfg
        if c.p:
            d.drop = L.Dropout(c.p, gr.SITE + zz * c.dsite, self.rng.data_ptr())
        if c.fp8:
            d.fp8, d.stride_scale_a, d.stride_scale_b = 1, I.stride_scale_a, I.stride_scale_b
        if inplace:
            assert c.res32 and c.batch == 1 and out["c32"] is not None
            res = torch.as_strided(I.res32, (c.m, c.n), (I.ldres, 1))
            torch.as_strided(out["c32"], (c.m, c.n), (I.ldc32, 1), I.c32_off).copy_(res)
            d.res32, d.ldres = d.c32, I.ldc32
        self.keep = out
        return d, out

    def workspace(self, d):
        """Split-K: a zeroed workspace of exactly vqa_gemm_workspace_bytes, sentinels behind it."""
        d.splitk = self.c.splitk
        need = int(self.L.load().vqa_gemm_workspace_bytes(ctypes.byref(d)))
        assert need % 4 == 0
        ws = torch.full((need // 4 + WS_TAIL,), WS_MARK, dtype=torch.int32, device="cuda")
        ws[:need // 4] = 0
        d.workspace, d.workspace_bytes = ws.data_ptr(), need
        return ws, need // 4

    def launch(self, d):
        return self.L.load().vqa_gemm(ctypes.byref(d), self.L.stream_handle())

    def go(self, cfg=0, **kw):
        d, out = self.prepare(cfg, **kw)
        self.L.check(self.launch(d), f"vqa_gemm {gr.name(self.c)} config {cfg}")
        return self.host(out)

    @staticmethod
    def host(out):
        torch.cuda.synchronize()
        return {t: None if b is None else b.cpu() for t, b in out.items()}

    def values(self, res, zs=None):
        """The written regions as [batch, m, n] fp64 arrays, after checking that every other element of
        every output buffer still holds the sentinel (zs: the batch elements this launch wrote)."""
        c, I, got = self.c, self.I, {}
        for t in ("c32", "c16"):
            if res[t] is None:
                continue
            off, ld, st = (I.c32_off, I.ldc32, I.stride_c32) if t == "c32" else (I.c16_off, I.ldc16, I.stride_c16)
            w = gr.written(c, I, t)
            if zs is not None:
                w = torch.zeros_like(w)
                for z in zs:
                    torch.as_strided(w, (c.m, c.n), (ld, 1), off + z * st).fill_(True)
            init = I.c32 if t == "c32" else I.c16
            assert torch.equal(_bits(res[t])[~w], _bits(init)[~w]), f"{gr.name(c)}: {t} written outside its region"
            got[t] = torch.stack([torch.as_strided(res[t], (c.m, c.n), (ld, 1), off + z * st)
                                  for z in range(c.batch)]).double().numpy()
        return got


def eligible(L, r, splitk=False):
    d, _ = r.prepare()
    if r.c.act >= 2:                                       # gemm_ext_kernel: one tile whatever the config
        return [cfg for cfg in sorted(L.GEMM_TILES) if cfg not in L.GEMM_PATCH_ONLY]
    return [cfg for cfg in sorted(L.GEMM_TILES) if L.gemm_config_fits(cfg, d) and not (splitk and cfg in L.GEMM_NO_SPLITK)]


def check(r, res, report, zs=None):
    """The result against the reference within the group's bound; the figures are recorded first."""
    c = r.c
    got = r.values(res, zs)
    errs = gr.errors(c, got)
    b = gr.bound(c.group)
    print(gr.name(c), {t: f"{e:.2e}" for t, e in errs.items()}, f"bound {b:.2e}")
    rec = report.setdefault("gemm_parity", {}).setdefault(c.group, {"bound": b, "yardstick": gr.yardstick(c.group),
                                                                   "largest": 0.0, "cases": 0})
    rec["largest"], rec["cases"] = max(rec["largest"], max(errs.values())), rec["cases"] + 1
    for t, e in errs.items():
        assert e <= b, (gr.name(c), t, e, b)
    if c.beta == 0 and got.keys() >= {"c32", "c16"}:        # c16 = RNE-bf16 of the very v that c32 holds
        assert np.array_equal(got["c16"], torch.from_numpy(got["c32"]).float().bfloat16().double().numpy()), gr.name(c)
    return got


def sweep(L, r, report, cfgs=None, auto=None):
    """First config against the reference, the others against the first; config 0 runs what
    vqa_gemm_select names.  Returns the first result."""
    cfgs = cfgs or eligible(L, r)
    assert cfgs, gr.name(r.c)
    first = r.go(cfgs[0])
    check(r, first, report)
    for cfg in cfgs[1:]:
        assert same(r.go(cfg), first), f"{gr.name(r.c)}: config {cfg} differs from config {cfgs[0]}"
    d, out = r.prepare(0)
    sel = L.load().vqa_gemm_select(ctypes.byref(d))
    assert sel in cfgs and (auto is None or sel == auto), (gr.name(r.c), sel, auto)
    L.check(r.launch(d), "vqa_gemm config 0")
    assert same(r.host(out), first), f"{gr.name(r.c)}: config 0 differs"
    return first


def variants(L, r, first, cfg):
    """c16-only and c32-only runs give the bits of the run that wrote both; beta does not reach c16."""
    c = r.c
    for out in ("c32", "c16"):
        one = Run(L, dataclasses.replace(c, out=out))
        res = one.go(cfg)
        one.values(res)
        assert torch.equal(_bits(res[out]), _bits(first[out])), f"{gr.name(c)}: {out} alone differs"
    if c.beta:
        nb = Run(L, dataclasses.replace(c, beta=0.0))
        res = nb.go(cfg)
        assert torch.equal(_bits(res["c16"]), _bits(first["c16"])), f"{gr.name(c)}: beta changed c16"


# ---------------------------------------------------------------------------- A. tiles x layouts x K
@pytest.mark.parametrize("layout,mn", sorted(gr.TILES), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_tiles_layouts_k(L, parity_report, layout, mn):
    for c in gr.TILES[(layout, mn)]:
        r = Run(L, c)
        cfgs = eligible(L, r)
        kc_b = 0 if c.bt else len(L.GEMM_KC_B_ONLY)
        assert len(cfgs) == 16 + kc_b + (len(L.GEMM_K64_ONLY) if c.k <= 64 else 0), cfgs
        sweep(L, r, parity_report, cfgs, auto=4 if c.k <= 128 else None)


# --------------------------------------------------------------------------------- B. epilogue matrix
@pytest.mark.parametrize("c", gr.EPI, ids=gr.name)
def test_epilogue_matrix(L, parity_report, c):
    r = Run(L, c)
    cfgs = eligible(L, r)
    first = sweep(L, r, parity_report, cfgs)
    variants(L, r, first, cfgs[-1])
    if c.res32 and not c.beta and not c.res16:                             # the residual added in place, as the engines do
        for cfg in cfgs:
            res = r.go(cfg, inplace=True)
            assert same(res, first), f"{gr.name(c)}: c32 == res32 differs at config {cfg}"


@pytest.mark.parametrize("c", gr.EPI_SCALAR_N, ids=gr.name)
def test_scalar_epilogue_odd_n(L, parity_report, c):
    r = Run(L, c)
    first = sweep(L, r, parity_report)
    variants(L, r, first, eligible(L, r)[0])


@pytest.mark.parametrize("c", gr.EPI_SCALAR, ids=gr.name)
def test_scalar_epilogue_equals_vector(L, c):
    """An odd ldc32, a c32 or a bias pointer 4 bytes off 16: the scalar epilogue, the vector run's bits."""
    v = Run(L, dataclasses.replace(c, scalar=""))
    want = v.values(v.go(eligible(L, v)[0]))
    r = Run(L, c)
    assert not gr.vec(c) and gr.vec(v.c)
    for cfg in eligible(L, r):
        got = r.values(r.go(cfg))
        assert all(np.array_equal(got[t], want[t]) for t in want), f"{gr.name(c)}: config {cfg}"


# --------------------------------------------------------------------------------------- C. batch
@pytest.mark.parametrize("c", gr.BATCH, ids=gr.name)
def test_batch_strides(L, parity_report, c):
    r = Run(L, c)
    cfgs = eligible(L, r)
    first = sweep(L, r, parity_report, cfgs)
    got = r.values(first)
    for z in range(c.batch):
        if c.p and not c.dsite and z:                      # one site: element (z*m + row)*n + col has no
            continue                                       # separate launch; the oracle hash has checked it
        one = r.values(r.go(cfgs[0], z=z), zs=(z,))
        assert all(np.array_equal(one[t][z], got[t][z]) for t in got), f"{gr.name(c)}: batch {z} != its own launch"


# ------------------------------------------------------------------------------------- D. split-K
@pytest.mark.parametrize("c", gr.SPLITK, ids=gr.name)
def test_splitk(L, parity_report, c):
    r = Run(L, c)
    cfgs = eligible(L, r, splitk=True)
    assert cfgs and not set(cfgs) & set(L.GEMM_NO_SPLITK)
    first = None
    for cfg in cfgs:
        d, out = r.prepare(cfg)
        ws, n = r.workspace(d)
        assert (n == 0) == (len(gr.slices(c)) == 1)
        for launch in range(2):                            # the second launch finds the counters it left
            if launch:
                d, out = r.prepare(cfg)
                d.splitk, d.workspace, d.workspace_bytes = c.splitk, ws.data_ptr(), 4 * n
            L.check(r.launch(d), f"vqa_gemm split-K config {cfg}")
            res = r.host(out)
            if first is None:
                first = res
                check(r, first, parity_report)
            assert same(res, first), f"{gr.name(c)}: config {cfg} launch {launch} differs"
            assert int(ws[:min(n, 16384)].abs().sum()) == 0, "arrival counters must be left zero"
            assert bool((ws[n:] == WS_MARK).all()), "written behind vqa_gemm_workspace_bytes"
    if len(gr.slices(c)) == 1:                             # one k-tile: the bits of splitk = 1
        plain = Run(L, dataclasses.replace(c, splitk=0))
        assert same(plain.go(cfgs[0]), first)


# ------------------------------------------------------------------------- E. convolution geometry
@pytest.mark.parametrize("c", gr.CONV + gr.BCONV, ids=gr.name)
def test_conv_geometry(L, parity_report, c):
    r = Run(L, c)
    cfgs = eligible(L, r)
    assert not set(cfgs) & set(L.GEMM_PLAIN_ONLY) and len(cfgs) >= 12
    sweep(L, r, parity_report, cfgs)


@pytest.mark.parametrize("c", gr.PATCH, ids=gr.name)
def test_patch_conv(L, parity_report, c):
    r = Run(L, c)
    cfgs = eligible(L, r)
    assert cfgs == sorted(L.GEMM_PATCH_ONLY)
    first = sweep(L, r, parity_report, cfgs)
    variants(L, r, first, cfgs[0])                         # c16 alone at ldc16 > Cout: the engine's placement


# --------------------------------------------------------------------------------- F. GELU / tanh
@pytest.mark.parametrize("c", gr.EXT, ids=gr.name)
def test_gelu_tanh(L, parity_report, c):
    r = Run(L, c)
    cfgs = eligible(L, r)
    assert len(cfgs) == len(L.GEMM_TILES) - len(L.GEMM_PATCH_ONLY)
    pre = gr.reference(dataclasses.replace(c, act=0, beta=0.0))["v"]
    assert pre.min() < -5 and pre.max() > 5 and np.abs(pre).min() < 1e-2      # spans the activation's range
    first = sweep(L, r, parity_report, cfgs)
    variants(L, r, first, cfgs[0])


# ------------------------------------------------------------------------------------------ G. fp8
@pytest.mark.parametrize("c", gr.FP8, ids=gr.name)
def test_fp8(L, parity_report, c):
    r = Run(L, c)
    if not c.splitk:
        cfgs = eligible(L, r)
        assert cfgs == sorted(L.GEMM_FP8)
        sweep(L, r, parity_report, cfgs, auto=4)
        return
    cfgs = eligible(L, r, splitk=True)
    assert cfgs == sorted(set(L.GEMM_FP8) - set(L.GEMM_NO_SPLITK)) and len(gr.slices(c)) == 2
    first = None
    for cfg in cfgs:
        d, out = r.prepare(cfg)
        ws, n = r.workspace(d)
        L.check(r.launch(d), f"vqa_gemm fp8 split-K config {cfg}")
        res = r.host(out)
        if first is None:
            first = res
            check(r, first, parity_report)
        assert same(res, first), f"config {cfg}"
        assert int(ws[:16384].abs().sum()) == 0 and bool((ws[n:] == WS_MARK).all())


# ----------------------------------------------------------------------------------------- H. pair
def test_pair_equals_two_launches(L, parity_report):
    rx, rw = Run(L, gr.PAIR[0]), Run(L, gr.PAIR[1])
    wx, ww = rx.go(L.GEMM_PAIR[0]), rw.go(L.GEMM_PAIR[0])
    check(rx, wx, parity_report)
    check(rw, ww, parity_report)
    for c1 in L.GEMM_PAIR:
        for c2 in L.GEMM_PAIR:
            dx, ox = rx.prepare(c1)
            dw, ow = rw.prepare(c2)
            L.check(L.load().vqa_gemm_pair(ctypes.byref(dx), ctypes.byref(dw), L.stream_handle()), "vqa_gemm_pair")
            assert same(Run.host(ox), wx) and same(Run.host(ow), ww), (c1, c2)


# ------------------------------------------------------------------------------------ I. refusals
def _refused(r, rc, *outs):
    assert rc == _err_invalid(), (rc, r.L.load().vqa_last_error())
    for out in outs:
        res = Run.host(out)
        for t, init in (("c32", r.I.c32), ("c16", r.I.c16)):
            assert res[t] is None or torch.equal(_bits(res[t]), _bits(init)), f"{t} written by a refused call"


_X = dict(group="gelu", m=72, n=136, k=72, bias=1, seed=7)
REFUSE_ACT = {
    "a_trans": gr.Case(**{**_X, "at": 1}), "b_trans": gr.Case(**{**_X, "bt": 1}),
    "a_conv": dataclasses.replace(gr.CONV[0], group="gelu"), "b_conv": dataclasses.replace(gr.BCONV[0], group="gelu"),
    "splitk": gr.Case(**{**_X, "k": 328, "splitk": 2}), "fp8": gr.Case(**{**_X, "k": 80, "fp8": 1}),
    "patch": dataclasses.replace(gr.PATCH[0], group="gelu"),
}


@pytest.mark.parametrize("act", (2, 3))
@pytest.mark.parametrize("what", sorted(REFUSE_ACT))
def test_gelu_tanh_refused_elsewhere(L, what, act):
    """GELU / tanh exist in gemm_ext_kernel alone (k-contiguous A and B, no conv operand, no split-K, no
    e4m3): every other form is refused, never run as a silent ReLU -- the patch convolution included."""
    c = dataclasses.replace(REFUSE_ACT[what], act=act)
    r = Run(L, c)
    for cfg in (0, L.GEMM_PATCH_ONLY[0] if what == "patch" else 4):
        d, out = r.prepare(cfg)
        if c.splitk:
            r.workspace(d)
        _refused(r, r.launch(d), out)


@pytest.mark.parametrize("which", ("dx", "dw", "both"))
def test_pair_refuses_gelu_tanh(L, which):
    rx, rw = Run(L, gr.PAIR[0]), Run(L, gr.PAIR[1])
    for act in (2, 3):
        dx, ox = rx.prepare(4)
        dw, ow = rw.prepare(4)
        if which in ("dx", "both"):
            dx.relu = act
        if which in ("dw", "both"):
            dw.relu = act
        rc = L.load().vqa_gemm_pair(ctypes.byref(dx), ctypes.byref(dw), L.stream_handle())
        _refused(rx, rc, ox)                               # neither half is launched
        _refused(rw, rc, ow)


def test_splitk_refuses_too_many_tiles(L):
    """More than 16384 tiles x batch do not fit the counter block.  (Every batch element shares one set
    of buffers here, so even a launch would stay in bounds.)"""
    c = gr.Case("splitk", 64, 64, 136, bias=1, splitk=2, out="c32")
    r = Run(L, c)
    d, out = r.prepare(3)
    d.batch, d.stride_a, d.stride_b, d.stride_c32 = 16385, 0, 0, 0
    ws, n = r.workspace(d)
    assert n > 16385 * 2 * 64 * 64
    _refused(r, r.launch(d), out)
    assert int(ws[:n].abs().sum()) == 0 and bool((ws[n:] == WS_MARK).all())


def test_bconv_refuses_k_beyond_fdiv(L):
    """b_conv splits k into (image, row, column) with a float reciprocal, exact below 2^24
    (tests/test_gemm_ref_cpu.py): k >= 2^24 is refused.  The operands are allocated in full."""
    n_img, h, w, ch = 1 << 16, 16, 16, 8
    k = n_img * h * w
    c = gr.Case("conv", 8, 72, 64, at=1, bt=1, out="c32")
    r = Run(L, c)
    dy = torch.zeros(k * 8, dtype=torch.bfloat16, device="cuda")
    x = torch.zeros(k * ch, dtype=torch.bfloat16, device="cuda")
    d, out = r.prepare(4)
    d.a, d.lda, d.b, d.ldb, d.k = dy.data_ptr(), 8, x.data_ptr(), 72, k
    d.b_conv, d.gb = 1, L.ConvGeom(n_img, h, w, ch, h, w, 3, 3, 1, 1)
    _refused(r, r.launch(d), out)
    d.k, d.gb = k - 256, L.ConvGeom(n_img - 1, h, w, ch, h, w, 3, 3, 1, 1)      # just below: accepted
    L.check(r.launch(d), "vqa_gemm b_conv below 2^24")
    got = r.values(Run.host(out))
    assert float(np.abs(got["c32"]).max()) == 0.0
