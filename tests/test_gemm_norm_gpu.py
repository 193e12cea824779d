"""GEMM with a fused row-norm tail (vqa_gemm_desc.norm) against GEMM + the stand-alone
vqa_layernorm_fwd / vqa_rmsnorm_fwd launch on its c32: the same bits, in one launch.

The fused and the unfused run share every input; the unfused c32 is the stand-alone kernel's
input, so GEMM accumulation order never enters a comparison."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LN, RMS = 1, 2
NORM_CONFIGS = (0, 3, 4, 5, 6, 7, 21)        # auto + every tile config with a norm tail
SHAPES = [(64, 256, 64), (100, 768, 200), (200, 1024, 136), (64, 768, 768)]
SENT = -1024.0                               # exact in bf16 too


@pytest.fixture(scope="module")
def k(pkg):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pkg.lib.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    return pkg


def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, device="cuda", generator=g) * scale).to(dtype)


def call(k, name, *args):
    k.ops.Call(name, *[k.ops.addr(a) if isinstance(a, torch.Tensor) else a for a in args])(k.lib.stream_handle())


def workspace():
    return torch.zeros(65536 // 4, dtype=torch.int32, device="cuda")


class Case:
    """Inputs of one GEMM (+ bias + fp32 residual + branch dropout p = 0.1) and norm, and
    sentinel-filled outputs with `pad` rows beyond m."""

    def __init__(self, k, M, N, K, kind, pad=0, seed=0, fp8=False):
        self.k, self.M, self.N, self.K, self.kind, self.fp8 = k, M, N, K, kind, fp8
        self.rng = torch.tensor([5, 3, 1], dtype=torch.int32, device="cuda")
        self.drop = k.lib.Dropout(0.1, 17, self.rng.data_ptr())
        if fp8:
            xf, wf = rnd((M, K), seed + 1), rnd((N, K), seed + 2, 0.05)
            self.x, self.sx = self.quant(xf)
            self.w, self.sw = self.quant(wf)
        else:
            self.x, self.w = rnd((M, K), seed + 1, dtype=torch.bfloat16), rnd((N, K), seed + 2, 0.05, torch.bfloat16)
        self.bias, self.res = rnd(N, seed + 3), rnd((M, N), seed + 4)
        self.g, self.b = 1 + 0.1 * rnd(N, seed + 5), 0.1 * rnd(N, seed + 6)
        self.rows = M + pad

    def quant(self, x):
        q = torch.empty(x.shape, dtype=torch.uint8, device="cuda")
        s = torch.empty(x.shape[0], device="cuda")
        call(self.k, "vqa_quant_rows_fp8", x, 0, x.shape[1], x.shape[0], x.shape[1], q, x.shape[1], s)
        return q, s

    def outputs(self):
        R, N = self.rows, self.N
        f = lambda *s: torch.full(s, SENT, device="cuda")
        return dict(c32=f(R, N), y32=f(R, N), y16=torch.full((R, N), SENT, device="cuda", dtype=torch.bfloat16),
                    mean=f(R), rstd=f(R))

    def desc(self, o, norm, cfg=0, ws=None, norm_drop=None, **over):
        M, N, K = self.M, self.N, self.K
        kw = dict(lda=K, ldb=K, c32=o["c32"], ldc32=N, bias=self.bias, res32=self.res, ldres=N)
        if self.fp8:
            kw.update(fp8=True, scale_a=self.sx, scale_b=self.sw)
        if norm:
            kw.update(norm=self.kind, norm_w=self.g, norm_b=self.b if self.kind == LN else None,
                      norm_eps=1e-5 if self.kind == LN else 1e-6, norm_y32=o["y32"], norm_y16=o["y16"],
                      norm_mean=o["mean"] if self.kind == LN else None, norm_rstd=o["rstd"], workspace=ws,
                      norm_drop=norm_drop)
        kw.update(over)
        d = self.k.ops.gemm_desc(self.x, self.w, M, N, K, **kw)
        d.drop = self.drop
        d.config = cfg
        return d

    def standalone(self, o, drop=None):
        """the stand-alone norm launch on o['c32']"""
        M, N = self.M, self.N
        if self.kind == LN:
            call(self.k, "vqa_layernorm_fwd", o["c32"], self.g, self.b, o["y32"], o["y16"], o["mean"], o["rstd"], M, N,
                 1e-5)
        else:
            call(self.k, "vqa_rmsnorm_fwd", o["c32"], self.g, o["y32"], o["y16"], o["rstd"], M, N, 1e-6,
                 ctypes.addressof(drop) if drop is not None else None)

    def unfused(self, cfg=0, drop=None):
        o = self.outputs()
        self.k.ops.run(self.desc(o, False, cfg))
        self.standalone(o, drop)
        return o

    def fused(self, cfg=0, ws=None, norm_drop=None):
        o = self.outputs()
        self.k.ops.run(self.desc(o, True, cfg, ws if ws is not None else workspace(), norm_drop))
        return o


def same(a, b, kind, what=""):
    torch.cuda.synchronize()
    for key in ("c32", "y32", "y16", "rstd") + (("mean",) if kind == LN else ()):
        assert torch.equal(a[key], b[key]), (what, key, (a[key].float() - b[key].float()).abs().max().item())


# ------------------------------------------------------------------ 1. fused == unfused, bitwise
@pytest.fixture(scope="module")
def unfused_ref(k):
    """(case, GEMM + stand-alone norm) of a (shape, kind, config): the same descriptor without
    norm, at the same tile config, then the stand-alone launch.  Computed once per key."""
    cases, refs = {}, {}

    def get(M, N, K, kind, cfg):
        if (M, N, K, kind) not in cases:
            cases[(M, N, K, kind)] = Case(k, M, N, K, kind, pad=28 if M == 100 else 0)
        c = cases[(M, N, K, kind)]
        if (M, N, K, kind, cfg) not in refs:
            refs[(M, N, K, kind, cfg)] = c.unfused(cfg)
            torch.cuda.synchronize()
        return c, refs[(M, N, K, kind, cfg)]
    return get


@pytest.mark.parametrize("cfg", NORM_CONFIGS)
@pytest.mark.parametrize("kind", [LN, RMS])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fused_equals_unfused(k, unfused_ref, M, N, K, kind, cfg):
    c, ref = unfused_ref(M, N, K, kind, cfg)
    ws = workspace()
    got = c.fused(cfg, ws)
    same(got, ref, kind, (M, N, K, kind, cfg))
    assert int(ws.abs().max()) == 0
    if c.rows > M:                                      # rows >= M of every output keep the sentinel
        for key, t in got.items():
            if not (key == "mean" and kind == RMS):
                assert torch.all(t[M:].float() == SENT), key
        assert torch.all(got["mean"].float() == SENT) or kind == LN


# ------------------------------------------------------------------ 2. against torch
@pytest.mark.parametrize("kind", [LN, RMS])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fused_against_torch(k, M, N, K, kind):
    c = Case(k, M, N, K, kind)
    o = c.fused()
    torch.cuda.synchronize()
    x = o["c32"]
    # the GEMM itself against fp32 matmul (accumulation order only: test_gemm_gpu.py's bound)
    keep = torch.from_numpy(_oracle().dropout_multiplier(0.1, 5, 3, 17, M * N)).cuda().view(M, N)
    ref_c = (c.x.float() @ c.w.float().T + c.bias) * keep + c.res
    scale = (c.x.float().abs() @ c.w.float().abs().T).max().item() / 0.9
    assert (x - ref_c).abs().max().item() <= 2e-5 * scale + 1e-6
    # the norm of the kernel's own c32, at the stand-alone kernels' tolerances
    if kind == LN:
        ref = F.layer_norm(x, (N,), c.g, c.b, 1e-5)
        torch.testing.assert_close(o["mean"], x.mean(-1), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(o["rstd"], torch.rsqrt(x.var(-1, unbiased=False) + 1e-5), rtol=1e-5, atol=1e-5)
    else:
        r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)
        ref = c.g * (x * r)
        torch.testing.assert_close(o["rstd"], r.squeeze(-1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(o["y32"], ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(o["y16"].float(), ref.to(torch.bfloat16).float(), rtol=1e-2, atol=1e-2)


def _oracle():
    from oracle import vqa_oracle as orc
    return orc


# ------------------------------------------------------------------ 3. batched, signed strides
@pytest.mark.parametrize("kind", [LN, RMS])
def test_batched_signed_strides(k, kind):
    NB, M, N, K = 3, 100, 768, 136
    ops, Lb = k.ops, k.lib
    rng = torch.tensor([7, 1, 1], dtype=torch.int32, device="cuda")
    x, w = rnd((NB, M, K), 1, dtype=torch.bfloat16), rnd((NB, N, K), 2, 0.05, torch.bfloat16)
    bias, res = rnd((NB, N), 3), rnd((M, N), 4)
    g, b = 1 + 0.1 * rnd((NB, N), 5), 0.1 * rnd((NB, N), 6)
    site0, dsite = 30, 6
    mk = lambda: dict(c32=torch.full((NB, M, N), SENT, device="cuda"), y32=torch.full((NB, M, N), SENT, device="cuda"),
                      y16=torch.full((NB, M, N), SENT, device="cuda", dtype=torch.bfloat16),
                      mean=torch.full((NB, M), SENT, device="cuda"), rstd=torch.full((NB, M), SENT, device="cuda"))
    eps = 1e-5 if kind == LN else 1e-6
    # fused: one launch; the y stacks are written last block first (slot NB-1-z)
    o = mk()
    d = ops.gemm_desc(x, w, M, N, K, lda=K, ldb=K, c32=o["c32"], ldc32=N, bias=bias, res32=res, ldres=N, batch=NB,
                      stride_a=M * K, stride_b=N * K, stride_c32=M * N, stride_res=0, stride_bias=N,
                      drop_site_stride=dsite, norm=kind, norm_w=g, norm_b=b if kind == LN else None, norm_eps=eps,
                      norm_y32=o["y32"][NB - 1], norm_y16=o["y16"][NB - 1], norm_mean=o["mean"] if kind == LN else None,
                      norm_rstd=o["rstd"], stride_norm_w=N, stride_norm_y=-M * N, stride_norm_stat=M,
                      workspace=workspace())
    d.drop = Lb.Dropout(0.1, site0, rng.data_ptr())
    ops.run(d)
    # unfused: three separate launches
    r = mk()
    for z in range(NB):
        dz = ops.gemm_desc(x[z], w[z], M, N, K, lda=K, ldb=K, c32=r["c32"][z], ldc32=N, bias=bias[z], res32=res, ldres=N)
        dz.drop = Lb.Dropout(0.1, site0 + z * dsite, rng.data_ptr())
        ops.run(dz)
        s = NB - 1 - z
        if kind == LN:
            call(k, "vqa_layernorm_fwd", r["c32"][z], g[z], b[z], r["y32"][s], r["y16"][s], r["mean"][z], r["rstd"][z],
                 M, N, eps)
        else:
            call(k, "vqa_rmsnorm_fwd", r["c32"][z], g[z], r["y32"][s], r["y16"][s], r["rstd"][z], M, N, eps, None)
    same(o, r, kind)


# ------------------------------------------------------------------ 4. RMSNorm norm_drop
def test_rmsnorm_norm_drop(k):
    M, N, K = 100, 768, 200
    c = Case(k, M, N, K, RMS)
    nd = k.lib.Dropout(0.1, 40, c.rng.data_ptr())
    ref = c.unfused(drop=nd)
    got = c.fused(norm_drop=nd)
    same(got, ref, RMS)
    plain = c.fused()
    torch.cuda.synchronize()
    mult = torch.from_numpy(_oracle().dropout_multiplier(0.1, 5, 3, 40, M * N)).cuda().view(M, N)
    assert torch.equal(got["y32"], plain["y32"] * mult)
    assert torch.equal(got["rstd"], plain["rstd"])


# ------------------------------------------------------------------ 5. counter hygiene
@pytest.mark.parametrize("kind", [LN, RMS])
def test_counters_left_zero(k, kind):
    c = Case(k, 200, 1024, 136, kind)
    ws = workspace()
    ref = c.unfused()
    o = c.outputs()
    d = c.desc(o, True, 0, ws)
    for it in range(5):
        for t in o.values():
            t.fill_(SENT)
        k.ops.run(d)
        same(o, ref, kind, it)
    assert int(ws.abs().max()) == 0
    c2 = Case(k, 100, 768, 200, kind, seed=9)           # another shape on the same workspace
    same(c2.fused(6, ws), c2.unfused(), kind)
    assert int(ws.abs().max()) == 0


# ------------------------------------------------------------------ 6. validation
def _bad_descs(k, c, o, ws):
    M, N, K = c.M, c.N, c.K
    small = torch.zeros(64, dtype=torch.int32, device="cuda")
    mask = torch.ones(M, N, device="cuda", dtype=torch.bfloat16)
    yield "no c32", c.desc(o, True, 0, ws, c32=None, ldc32=0, c16=o["y16"], ldc16=N)
    yield "ldc32 != n", c.desc(o, True, 0, ws, ldc32=N + 8)
    yield "beta", c.desc(o, True, 0, ws, beta=1.0)
    yield "relu", c.desc(o, True, 0, ws, relu=True, res32=None)
    yield "splitk", c.desc(o, True, 0, ws, splitk=2)
    yield "mask16", c.desc(o, True, 0, ws, mask16=mask, ldmask=N)
    yield "no workspace", c.desc(o, True, 0, None)
    yield "small workspace", c.desc(o, True, 0, small)
    yield "not vectorised", c.desc(o, True, 0, ws, ldres=N + 4)
    yield "b_trans", c.desc(o, True, 0, ws, b_trans=True, ldb=N)
    g = k.ops.conv_geom(1, 10, 10, 8, 10, 10, 3, 3, 1, 1)
    yield "a_conv", c.desc(o, True, 0, ws, ga=g)
    yield "b_conv", c.desc(o, True, 0, ws, gb=g, b_trans=True, ldb=N)
    # more (batch, row block) pairs than counters: 8193 x 2 row blocks of 64 rows (zero batch
    # strides: no large buffers)
    yield "16386 pairs", c.desc(o, True, 0, ws, batch=8193)
    yield "16386 pairs, config 5", c.desc(o, True, 5, ws, batch=8193)
    yield "16385 pairs, 128-row tiles", c.desc(o, True, 6, ws, batch=16385)
    for cfg in (1, 2, 8, 9, 13, 22, 26):
        yield f"config {cfg}", c.desc(o, True, cfg, ws)
    if c.kind == LN:
        yield "LN without beta", c.desc(o, True, 0, ws, norm_b=None)
        yield "LN without mean", c.desc(o, True, 0, ws, norm_mean=None)
        yield "LN with norm_drop", c.desc(o, True, 0, ws, norm_drop=k.lib.Dropout(0.1, 3, c.rng.data_ptr()))
    else:
        yield "RMS with beta", c.desc(o, True, 0, ws, norm_b=c.b)
        yield "RMS with mean", c.desc(o, True, 0, ws, norm_mean=o["mean"])
    yield "no y", c.desc(o, True, 0, ws, norm_y32=None, norm_y16=None)
    d = c.desc(o, True, 0, ws)
    d.norm = 3
    yield "bad kind", d


@pytest.mark.parametrize("kind", [LN, RMS])
def test_validation_rejects_and_writes_nothing(k, kind):
    c = Case(k, 100, 768, 200, kind)
    ws = workspace()
    o = c.outputs()
    n = 0
    for what, d in _bad_descs(k, c, o, ws):
        with pytest.raises(RuntimeError):
            k.ops.run(d)
            pytest.fail(f"accepted: {what}")
        n += 1
    assert n >= 24
    # n not a multiple of 256 / wider than 1024
    for N in (320, 1280):
        c2 = Case(k, 64, N, 64, kind)
        o2 = c2.outputs()
        with pytest.raises(RuntimeError):
            k.ops.run(c2.desc(o2, True, 0, ws))
        torch.cuda.synchronize()
        assert all(torch.all(t.float() == SENT) for t in o2.values())
    # a norm descriptor in the paired launch is rejected
    good = c.desc(o, True, 0, ws)
    plain = c.desc(o, False, 0)
    with pytest.raises(RuntimeError):
        k.ops.Call("vqa_gemm_pair", ctypes.byref(good), ctypes.byref(plain))(k.lib.stream_handle())
    torch.cuda.synchronize()
    assert all(torch.all(t.float() == SENT) for t in o.values())
    assert int(ws.abs().max()) == 0
    assert k.lib.load().vqa_gemm_workspace_bytes(ctypes.byref(good)) == 65536
    assert k.lib.load().vqa_gemm_select(ctypes.byref(good)) in k.lib.GEMM_NORM


# ------------------------------------------------------------------ 7. fp8
@pytest.mark.parametrize("kind", [LN, RMS])
def test_fp8_fused_equals_unfused(k, kind):
    c = Case(k, 128, 1024, 256, kind, fp8=True)
    same(c.fused(21), c.unfused(21), kind)


# ------------------------------------------------------------------ 8. / 9. engine
def _engine(k, fuse, B=5):
    sd = _engine.sd = getattr(_engine, "sd", None) or k.synthetic.make_state_dict("resnet50", seed=0)
    eng = k.engine.VQAEngine(sd, vision="resnet50", batch=B, seq_len=16, image_size=64, dropout=0.1, seed=0,
                             pipeline=False, fuse_norm=fuse)
    eng.load_batch(k.synthetic.make_batch(B, 16, 64, seed=1))
    return eng


def _state(eng):
    torch.cuda.synchronize()
    return dict(LOGP=eng.LOGP.clone(), LOSS=eng.LOSS.clone(), gn=eng.opt_state.clone(), P32=eng.P32.clone())


def _names(eng):
    return [c.name for c in eng.fwd_calls]


def test_engine_fused_equals_unfused(k):
    on, off = _engine(k, True), _engine(k, False)
    assert not on.fuse_norm_kept
    assert len(off.fwd_calls) - len(on.fwd_calls) == 33
    assert _names(on).count("vqa_layernorm_fwd") == 0 and _names(on).count("vqa_rmsnorm_fwd") == 1
    for step in range(3):
        on.train_step()
        off.train_step()
        a, b = _state(on), _state(off)
        for key in a:
            assert torch.equal(a[key], b[key]), (step, key)
    assert all(int(w.abs().max()) == 0 for w in on.NORM_WS)
    for e in (on, off):                                 # eval mode: every dropout the identity
        e.flush_optimizer()
        e.set_training(False)
        e.forward()
    a, b = _state(on), _state(off)
    assert torch.equal(a["LOGP"], b["LOGP"]) and torch.equal(a["LOSS"], b["LOSS"])
    assert torch.equal(on.TXT32, off.TXT32)


def test_deferred_update_ranges_cover_what_each_t5_layer_reads(k):
    """The captured step applies the previous step's AdamW range by range beside the T5 encoder
    (engine._forward_branches_deferred); a layer's calls start once the ranges of _t5_waits(i)
    and of the layers before it are applied.  Every parameter a layer's calls read must lie in
    one of those ranges -- with fuse_norm a layer's wo GEMM reads the NEXT layer's ln0 gain."""
    for fuse in (False, True):
        eng = _engine(k, fuse)
        spans = {"P32": (eng.P32.data_ptr(), 4, eng.P32.numel()), "P16": (eng.P16.data_ptr(), 2, eng.P16.numel())}
        starts = list(eng._t5_layer_start) + [eng._fsplit[2]]
        awaited, seen = set(), 0
        for i in range(eng.nl):
            awaited |= set(eng._t5_waits(i))
            ok = [eng.adam_cuts[n] for n in awaited]
            for c in eng.fwd_calls[starts[i]:starts[i + 1]]:
                for where, p in k.ops._pointers(c):
                    for base, size, numel in spans.values():
                        if base <= p < base + size * numel:
                            off = (p - base) // size
                            assert any(lo <= off < hi for lo, hi in ok), (fuse, i, c.name, where)
                            seen += 1
        assert seen >= 6 * eng.nl                       # q|k|v, o, wi, wo and two gains per layer
        assert ("t5.1" in eng._t5_waits(0)) == fuse


def test_engine_fused_graph_equals_stream(k):
    g, s = _engine(k, True), _engine(k, True)
    g.capture()
    for step in range(2):
        g.train_step()
        s.train_step()
        a, b = _state(g), _state(s)
        for key in a:
            assert torch.equal(a[key], b[key]), (step, key)


def test_default_plan_has_no_norm_fields(k, monkeypatch):
    monkeypatch.delenv("VQA_FUSE_NORM", raising=False)
    eng = _engine(k, None)
    assert not eng.fuse_norm
    n = _names(eng)
    assert n.count("vqa_layernorm_fwd") == 9 and n.count("vqa_rmsnorm_fwd") == 25
    for c in eng.fwd_calls + eng.bwd_calls:
        for d in (c.desc if isinstance(c.desc, tuple) else (c.desc,)):
            if isinstance(d, k.lib.GemmDesc):
                assert d.norm == 0 and not d.norm_w and not d.norm_y32 and not d.norm_y16 and not d.norm_rstd
    monkeypatch.setenv("VQA_FUSE_NORM", "1")
    assert _engine(k, None).fuse_norm


# ------------------------------------------------------------------ 10. the stand-alone kernels' bits
def test_standalone_norm_bits_are_the_recorded_ones(k):
    """vqa_rmsnorm_fwd / vqa_layernorm_fwd at D = 256, 512, 768, 1024 against the bits recorded
    from the build before their row arithmetic moved into norm_rows.h
    (tests/golden/norm_fwd_bits.npz, tests/golden/make_norm_fwd_bits.py)."""
    import importlib.util
    import os
    import numpy as np
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_norm_fwd_bits", os.path.join(gdir, "make_norm_fwd_bits.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    gold = np.load(os.path.join(gdir, "norm_fwd_bits.npz"))
    for D in (256, 512, 768, 1024):
        got = rec.run_norms(k.lib.load(), *rec.inputs(D))
        for name, t in got.items():
            assert np.array_equal(t.view(np.uint32), gold[f"{name}_{D}"].view(np.uint32)), (D, name)
