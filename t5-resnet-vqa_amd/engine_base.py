"""EngineBase: what the two training engines (engine.VQAEngine, vit_engine.VitVQAEngine)
share -- the flat fp32 parameter / gradient / AdamW arenas with their bf16 shadow, the
builders of prepared library calls (every tensor a call bakes an address of is recorded in
its `keep`; _wgemm is the one place a weight GEMM gets bf16 or e4m3 operands, _dw_batched the one
launch over consecutive weight-gradient segments), the AdamW descriptors (the full arena and any
sub-range of it), the eager forward / backward / optimizer entry points, and the readouts in reference layout
(state_dict, optimizer state, parameter views).  An engine adds its own plan:
`_plan_forward` / `_plan_backward` / `_plan_optimizer`, `load_batch`, `train_step`, `capture`.
The forward-only evaluation graph (eval_plan ... eval_result) is shared too; an engine supplies
the calls of its evaluation step (`_run_eval_streams`) and says whether it may evaluate
(`_eval_setup`).  The builders are also what t5_stack.T5Stack, the one plan of a T5 layer stack
(the ResNet model's encoder, the ViT model's encoder and decoder), and sga_stack.SGAStack, the one
plan of the ResNet model's SGA blocks, append their calls through.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc

import numpy as np
import torch

from . import lib as L
from . import ops
from . import tune

BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64

# dropout site ids (the hash key of each nn.Dropout application of the step)
SITE_EMBED, SITE_FINAL = 1, 2                  # T5Stack: dropout(inputs_embeds) :725, dropout(final_ln) :745


def t5_site(layer, kind):
    """kind 0 attention probs (:168), 1 attention residual branch (:400), 2 FF inner (:86), 3 FF residual (:140)"""
    return 16 + 4 * layer + kind


class _Seq:
    """Several prepared calls issued as one (a deferred AdamW range and the e4m3 weight
    copies that follow it)."""
    def __init__(self, calls):
        self.calls = calls

    def __call__(self, stream):
        for c in self.calls:
            c(stream)


@contextlib.contextmanager
def no_gc_capture():
    """Stream capture with the cyclic garbage collector held off.  Engines (and the graphs /
    tensors they own) are reclaimed through reference cycles; a collection that lands inside
    a capture destroys another engine's graph execs and frees its blocks while the capture
    is being recorded (measured: the later replay of the captured graph crashed in the
    runtime).  Collect first, then keep the collector off until the capture has ended."""
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _after(stream, other):
    """`stream` waits for everything issued so far on `other` (an event, no host sync)."""
    if stream is other:
        return
    ev = torch.cuda.Event()
    ev.record(other)
    stream.wait_event(ev)


_WARNED_ATTN = set()


def _check_attn_path(d, fn):
    """Say it loudly (once per shape) when a planned attention call would run the scalar VALU
    kernel (include/vqa_hip.h vqa_attn_path): it is correct but an order of magnitude slower
    than the MFMA kernels, which cover lq <= 32, lk <= 160 (key mask: lk <= 64)."""
    path = L.load().vqa_attn_path(ctypes.byref(d), int(fn == "vqa_attn_bwd"))
    if path == L.ATTN_VALU:
        key = (fn, d.lq, d.lk, d.dh, bool(d.key_mask))
        if key not in _WARNED_ATTN:
            _WARNED_ATTN.add(key)
            import warnings
            warnings.warn(f"{fn}: lq={d.lq} lk={d.lk} dh={d.dh} key_mask={bool(d.key_mask)} runs the scalar VALU "
                          "attention kernel (no MFMA kernel covers this shape)", RuntimeWarning, stacklevel=3)
    return path


def _h2d(dst, src):
    """dst <- src (numpy / torch, host or device).  Asynchronous only from device or pinned
    memory: an async copy out of a pageable temporary (freed when this returns) may be read
    by the runtime after the free."""
    src = torch.as_tensor(src).to(dst.dtype).reshape(dst.shape)
    dst.copy_(src, non_blocking=src.is_cuda or src.is_pinned())


IGNORE_INDEX = -100          # nn.NLLLoss's default ignore_index: the head skips rows with a target < 0


def batch_rows(batch, key, planned, allow_empty=False):
    """Rows of a collate batch (the reference's loaders have no drop_last, so an epoch's last
    batch is short: faster_rcnn_vqa_trainer.py:172-197); 1 <= rows <= the planned batch (0 rows
    only for a data-parallel rank whose share of the global batch is empty: allow_empty)."""
    n = int(torch.as_tensor(batch[key]).shape[0])
    if not (0 if allow_empty else 1) <= n <= planned:
        lo = 0 if allow_empty else 1
        raise ValueError(f"{key}: batch of {n} rows; this engine is planned for {lo}..{planned} rows")
    return n


def _is_rows_of(dst, src, n):
    """src already is the first n rows of the buffer dst (a collate wrote them in place, e.g.
    DaquarVitCollate(out=eng.PIX)): nothing to copy."""
    return (isinstance(src, torch.Tensor) and src.device == dst.device and src.dtype == dst.dtype
            and src.data_ptr() == dst.data_ptr() and src.is_contiguous() and dst.is_contiguous()
            and tuple(src.shape) == (n,) + tuple(dst.shape[1:]))


def load_rows(dst, src, n, fill=None, empty_fill=0):
    """dst[:n] <- src (n rows); the planned rows past n are padding: copies of rows 0..n-1
    (real samples, so every activation stays finite) or `fill` (targets: IGNORE_INDEX, so the
    padded rows add nothing to the loss or to any gradient -- the NLL mean runs over the n
    real rows).  n = 0 (an empty data-parallel rank): every row is `fill`, else `empty_fill`
    (finite inputs whose targets are all ignored: the rank's gradient is exactly zero).
    A src that is dst's own first n rows is not copied onto itself."""
    if src is None:
        return
    B = dst.shape[0]
    if n == 0:
        dst.fill_(fill if fill is not None else empty_fill)
        return
    if not _is_rows_of(dst, src, n):
        _h2d(dst[:n] if n < B else dst, src)
    if n == B:
        return
    if fill is not None:
        dst[n:].fill_(fill)
        return
    i = n
    while i < B:                                   # doubling copies of the real rows
        k = min(i, B - i)
        dst[i:i + k].copy_(dst[:k])
        i += k


def _plain_device_copy(dst, src):
    """dst <- src is a plain device copy vqa_copy_multi can take: a contiguous device tensor of the
    buffer's dtype and size (all planned rows), 16-byte aligned."""
    return (isinstance(src, torch.Tensor) and src.is_cuda and src.device == dst.device and src.dtype == dst.dtype
            and src.numel() == dst.numel() and src.is_contiguous() and dst.is_contiguous()
            and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and (dst.numel() * dst.element_size()) % 16 == 0)


def load_rows_multi(items, n):
    """load_rows for several (dst, src, kwargs) buffers of one batch of n rows.  The full device
    batches among them (a training loop's usual case: n = the planned rows, sources already on the
    device in the buffers' dtypes) go in ONE vqa_copy_multi launch on the current stream instead of
    a runtime copy launch each; anything else keeps load_rows."""
    jobs = []
    for dst, src, kw in items:
        if src is not None and n == dst.shape[0] and len(jobs) < L.COPY_MAX_JOBS and _plain_device_copy(dst, src):
            jobs.append((dst, src))
        else:
            load_rows(dst, src, n, **kw)
    if jobs:
        arr = (L.CopyJob * len(jobs))(*[L.CopyJob(d.data_ptr(), s.data_ptr(), d.numel() * d.element_size())
                                         for d, s in jobs])
        L.call("vqa_copy_multi", arr, len(jobs))


class EngineBase:
    TIED = {}                         # reference keys that alias another trainable key (tied weights)

    def __init__(self, device, dropout, seed, warmup, total, max_norm, betas, eps, weight_decay, grad_scale=1.0,
                 group_lr=None):
        L.load()
        self.dev = torch.device(device)
        self.p_drop, self.seed = float(dropout), int(seed)
        self.warmup, self.total, self.max_norm = warmup, total, max_norm
        self.betas, self.eps, self.wd = betas, eps, weight_decay
        self.grad_scale = grad_scale
        self.group_lr = dict(group_lr or {})  # per-group LR overrides (trainer optimizer_kwargs)
        self.fp8 = False                  # e4m3 forward weight GEMMs (VQAEngine, config 5)
        self.pair_bwd = False             # _dxdw as one paired launch (VQAEngine)
        self.graph = None
        self.eval_graph = None            # a forward-only evaluation graph (eval_capture)
        self.eval_call = None             # its vqa_eval_rows tail (eval_plan)
        self.eval_rollout = False         # the evaluation step also carries the attention rollout (VitVQAEngine)
        self.eval_heatmap = False         # ... the vision map's heat map (VQAEngine)
        self._keep_graph = False          # capture(keep_graph=True): the hipGraph_t of each part is kept
        self._scratch = None              # split-K workspace used while autotuning
        self._jobs = []                   # column-sum reductions queued by _defer until _flush
        self.GACC = None                  # gradient accumulator the optimizer plan reads instead of G32 (G_OPT)

    # ------------------------------------------------------------------ hooks
    def _model_specs(self):
        """{reference state-dict key: shape} of the whole model."""
        raise NotImplementedError

    def _trainable_keys(self):
        """The reference keys held in the flat arenas (tied aliases not among them)."""
        return [k for s in self.lay.segments.values() for k in s.parts]

    def _adam_groups(self):
        """(ends, lrs): the end offset and learning rate of each parameter group of the layout."""
        raise NotImplementedError

    def _tune_calls(self):
        """The prepared calls whose GEMMs autotune() times."""
        return self.fwd_calls + self.bwd_calls

    def _alloc_shadow_arenas(self):
        """Parameter shadows beyond the bf16 one, allocated between G32 and the AdamW moments."""

    def flush_optimizer(self):
        """Apply a deferred AdamW update now (nothing is deferred unless an engine says so)."""

    # ------------------------------------------------------------------ allocation
    def _t(self, shape, dtype=F32, zero=False):
        f = torch.zeros if zero else torch.empty
        return f(shape, dtype=dtype, device=self.dev)

    def _alloc_arenas(self, sd):
        lay = self.lay
        self.P32 = torch.from_numpy(lay.pack(sd)).to(self.dev)
        self.P16 = self.P32.to(BF16)
        self.G32 = self._t(lay.total, zero=True)
        self._alloc_shadow_arenas()
        self.M, self.V, self.VMAX = (self._t(lay.total, zero=True) for _ in range(3))
        self.p32, self.p16, self.g32 = {}, {}, {}
        for s in lay.segments.values():
            sl = slice(s.offset, s.offset + s.numel)
            self.p32[s.name] = self.P32[sl].view(s.shape)
            self.p16[s.name] = self.P16[sl].view(s.shape)
            self.g32[s.name] = self.G32[sl].view(s.shape)
        self.opt_state = self._t(L.ST_FLOATS, zero=True)
        # dropout RNG state {seed, counter, training}; the forward's first call advances the counter
        self.RNG = torch.from_numpy(np.array([self.seed & 0xFFFFFFFF, 0, 1, 0], np.uint32).view(np.int32)).to(self.dev)

    # ------------------------------------------------------------------ call helpers
    # Every helper records the tensors it bakes into a call (ops.Call.keep), so no
    # buffer can be freed while a prepared call still points at it.  Raw int
    # addresses (sub-views made with ops.addr) must come from tensors that are
    # passed too or are engine attributes.
    def _gemm(self, lst, a, b, m, n, k, keep=(), **kw):
        ts = [a, b] + [v for v in kw.values() if isinstance(v, torch.Tensor)] + list(keep)
        lst.append(ops.gemm_call(ops.gemm_desc(a, b, m, n, k, **kw), [t for t in ts if isinstance(t, torch.Tensor)]))

    def _call(self, lst, name, *args, extra=()):
        ts = tuple(a for a in args if isinstance(a, torch.Tensor)) + tuple(extra)
        lst.append(ops.Call(name, *[ops.addr(a) if isinstance(a, torch.Tensor) else a for a in args], keep=ts))

    def _attn(self, lst, fn, drop=None, keep=(), **kw):
        d = L.AttnDesc()
        for k, v in kw.items():
            setattr(d, k, ops.addr(v) if isinstance(v, torch.Tensor) else v)
        ts = tuple(v for v in kw.values() if isinstance(v, torch.Tensor)) + tuple(keep)
        dd = self._drop(drop) if drop is not None else None
        if dd is not None:
            d.drop = dd
            ts = ts + (self.RNG,)
        _check_attn_path(d, fn)
        lst.append(ops.Call(fn, ctypes.byref(d), keep=ts, desc=d))

    def _drop(self, site):
        """vqa_dropout for `site` (None when dropout is off)."""
        if self.p_drop <= 0.0:
            return None
        return L.Dropout(self.p_drop, site, self.RNG.data_ptr())

    def _dptr(self, site, keep):
        """`const vqa_dropout*` argument (0 = none); the struct is kept alive through `keep`."""
        d = self._drop(site)
        if d is None:
            return None
        keep.append(d)
        return ctypes.addressof(d)

    def _set_drop(self, call, site):
        """Dropout `site` (None: none) on the output of a prepared GEMM."""
        d = self._drop(site) if site is not None else None
        if d is not None:
            call.desc.drop = d
            call.keep = call.keep + (self.RNG,)

    @property
    def drop_scale(self):
        """1/(1-p) in fp32, the multiplier of a kept element (as the kernels compute it)."""
        p = np.float32(self.p_drop)
        return float(np.float32(1.0) / (np.float32(1.0) - p))

    def _wgemm(self, lst, x16, wname, m, n=None, batch=None, drop=None, keep=(), **kw):
        """y = x W^T with weight segment `wname` as one vqa_gemm, on bf16 operands or, for the
        weights of _is_fp8, on e4m3 ones: the one place that choice is made (the activation's
        row-wise e4m3 copy, the weight's, both scale vectors, their strides and the keeps).
        n: the output columns where side-by-side segments form one matrix (default: the segment's
        rows).  batch: one launch over x16 [batch, m, k] and `batch` segments from `wname` on, at
        stride kw["stride_b"] (ParamLayout.stride).  kw: the other ops.gemm_desc keywords -- outputs,
        bias, residual, their strides, a fused norm; drop: the dropout site of the output."""
        nn, k = self.p16[wname].shape
        if batch is not None:
            kw.update(batch=batch, stride_a=m * k)
        a, b = x16, self.p16[wname]
        if self.fp8 and self._is_fp8(wname):
            off = self.lay[wname].offset
            a, xs = self._quant_act(lst, (wname, "x"), x16, m * (batch or 1))
            b = self.W8[off:]
            kw.update(fp8=True, scale_a=xs, scale_b=ops.addr(self.WSC, off))
            if batch is not None:
                kw.update(stride_scale_a=m, stride_scale_b=kw.get("stride_b", 0))
            keep = tuple(keep) + (self.W8, self.WSC)
        self._gemm(lst, a, b, m, nn if n is None else n, k, lda=k, ldb=k, keep=keep, **kw)
        self._set_drop(lst[-1], drop)

    def _linear_kw(self, x16, wname, m, out32=None, out16=None, bias=True, relu=False, res32=None, drop=None,
                   norm=None):
        """_wgemm keywords of a Linear over one weight.  norm: vqa_gemm_desc norm fields
        (ops.gemm_desc keywords) of a row norm fused behind this GEMM (fuse_norm), or None."""
        n = self.p16[wname].shape[0]
        return dict(norm or {}, x16=x16, wname=wname, m=m, c32=out32, ldc32=n, c16=out16, ldc16=n,
                    bias=self.p32[wname[:-1] + "b"] if bias else None, relu=relu, res32=res32, ldres=n, drop=drop)

    def _linear(self, lst, *args, **kw):
        self._wgemm(lst, **self._linear_kw(*args, **kw))

    def _dx(self, lst, dy16, wname, m, out32=None, out16=None, res32=None, mask16=None, beta=0.0, alpha=1.0):
        """dX[m, k] = alpha * dY[m, n] W[n, k]  (+res) (*mask>0) (+beta*out32)"""
        w = self.p16[wname]
        n, k = w.shape
        self._gemm(lst, dy16, w, m, k, n, lda=n, ldb=k, b_trans=True, c32=out32, ldc32=k, c16=out16, ldc16=k,
                   res32=res32, ldres=k, mask16=mask16, ldmask=k, beta=beta, alpha=alpha)

    def _dw(self, lst, dy16, x16, wname, rows, bias_from=None):
        """dW[n, k] = dY[rows, n]^T X[rows, k]; optional bias grad = colsum(bias_from), bf16.
        Tagged `side`: nothing on the dX chain reads them, so a step with a weight-gradient
        stream (VQAEngine._run_tagged) runs them beside the chain, joined before the optimizer."""
        g = self.g32[wname]
        n, k = g.shape
        self._gemm(lst, dy16, x16, n, k, rows, lda=n, ldb=k, a_trans=True, b_trans=True, c32=g, ldc32=k)
        lst[-1].side = True
        if bias_from is not None:
            assert bias_from.shape[-1] == n
            self._bias_colsum(lst, bias_from, rows, wname[:-1] + "b")

    def _dxdw(self, lst, dy16, x16, wname, rows, bias_from=None, **dxkw):
        """A layer's input gradient and weight gradient (they share dY), then the bias column
        sum; with pair_bwd the two GEMMs as ONE paired launch (vqa_gemm_pair)."""
        tmp = []
        self._dx(tmp, dy16, wname, rows, **dxkw)
        self._dw(tmp, dy16, x16, wname, rows, bias_from=bias_from)
        if self.pair_bwd:
            gx, gw = tmp[:2]
            tmp[:2] = [ops.Call("vqa_gemm_pair", ctypes.byref(gx.desc), ctypes.byref(gw.desc), keep=gx.keep + gw.keep,
                                desc=(gx.desc, gw.desc))]
        lst.extend(tmp)

    def _dx_only(self, lst, dy16, x16, wname, rows, bias_from=None, **dxkw):
        """_dxdw without the weight gradient (left to _dw_batched, a launch batched over layers)."""
        self._dx(lst, dy16, wname, rows, **dxkw)
        if bias_from is not None:
            self._bias_colsum(lst, bias_from, rows, wname[:-1] + "b")

    def _dw_batched(self, lst, dys, xs, names, rows, slot=0, stride=None):
        """The weight gradients of the consecutive segments `names` as ONE launch: dW_j =
        dys[slot + j]^T xs[slot + j] over `rows` rows, the stacks and the gradient segments at
        constant strides (stride: the segments', default ParamLayout.stride).  Tagged `side`."""
        g = self.g32[names[0]]
        n, k = g.shape
        self._gemm(lst, ops.addr(dys, slot * rows * n), ops.addr(xs, slot * rows * k), n, k, rows, lda=n, ldb=k,
                   a_trans=True, b_trans=True, c32=g, ldc32=k, batch=len(names), stride_a=rows * n, stride_b=rows * k,
                   stride_c32=self.lay.stride(names) if stride is None else stride, keep=(dys, xs, self.G32))
        lst[-1].side = True

    def _bias_colsum(self, lst, dy16, rows, bname):
        """A Linear bias gradient = column sums of its bf16 output gradient: the partial
        column sums now, the final sum deferred (_flush)."""
        lib = L.load()
        n = dy16.shape[-1]
        ws = self._t(lib.vqa_colsum_workspace_floats(rows, n))
        self._call(lst, "vqa_colsum", dy16, 1, rows, n, n, None, 0.0, ws)
        self._defer(ws, lib.vqa_colsum_parts(rows), n, n, self.g32[bname])

    def _defer(self, ws, parts, stride, cols, out, beta=0.0, offset=0, keep=()):
        """Queue the final reduction out = beta*out + sum_p ws[offset + p*stride + c] (a norm
        weight/bias or Linear bias gradient whose per-block partial rows a backward kernel
        wrote); _flush() finishes every queued one in a single vqa_colsum_batched launch.
        keep: what the job reads or writes beyond `ws` and `out`."""
        self._jobs.append((ops.addr(ws) + 4 * offset, ops.addr(out), stride, parts, cols, beta,
                           (ws, out) + tuple(keep)))

    def _flush(self, lst):
        if not self._jobs:
            return
        arr = (L.ColsumJob * len(self._jobs))()
        blk = 0
        keep = []
        for j, (ws, out, stride, parts, cols, beta, k) in enumerate(self._jobs):
            arr[j] = L.ColsumJob(ws, out, stride, parts, cols, beta, blk)
            blk += -(-cols // 64)
            keep += list(k)
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.dev)
        lst.append(ops.Call("vqa_colsum_batched", raw.data_ptr(), len(self._jobs), blk, keep=tuple(keep) + (raw,)))
        self._jobs = []

    def _norm_ws(self, rows=None):
        """A private partial-row workspace for one deferred norm backward over `rows` (T) rows."""
        return self._t(L.load().vqa_norm_bwd_workspace_floats(self.T if rows is None else rows, self.D))

    def _run(self, calls):
        s = L.stream_handle()
        for c in calls:
            c(s)

    # ------------------------------------------------------------------ AdamW descriptors
    @property
    def G_OPT(self):
        """The gradient arena the optimizer plan reads (squared norms, AdamW descriptors): G32, or
        the accumulator of an engine that accumulates micro-batches (VQAEngine.use_accumulation)."""
        return self.G32 if self.GACC is None else self.GACC

    def _adam_desc_full(self):
        """The AdamW-amsgrad descriptor of the whole flat arena."""
        d = L.AdamWDesc()
        d.param, d.grad = self.P32.data_ptr(), self.G_OPT.data_ptr()
        d.exp_avg, d.exp_avg_sq, d.max_exp_avg_sq = self.M.data_ptr(), self.V.data_ptr(), self.VMAX.data_ptr()
        d.param16 = self.P16.data_ptr()
        d.n = self.lay.total
        ends, lrs = self._adam_groups()
        d.ngroups = len(ends)
        for i, (e, lr) in enumerate(zip(ends, lrs)):
            d.group_end[i], d.group_lr[i] = e, lr
        d.beta1, d.beta2, d.eps, d.weight_decay = self.betas[0], self.betas[1], self.eps, self.wd
        d.grad_scale = self.grad_scale
        d.state = self.opt_state.data_ptr()
        return d

    def _adam_range_desc(self, lo, hi):
        """self._adam_desc restricted to flat elements [lo, hi): the six arena pointers moved to
        `lo`, n = hi - lo, the group ends relative to `lo`; every other field as in the full one."""
        d = self._adam_desc
        ds = L.AdamWDesc()
        ctypes.memmove(ctypes.addressof(ds), ctypes.addressof(d), ctypes.sizeof(d))
        ds.param, ds.grad = ops.addr(self.P32, lo), d.grad + 4 * lo      # the full one's arena: G32 or GACC
        ds.exp_avg, ds.exp_avg_sq = ops.addr(self.M, lo), ops.addr(self.V, lo)
        ds.max_exp_avg_sq, ds.param16 = ops.addr(self.VMAX, lo), ops.addr(self.P16, lo)
        ds.n = hi - lo
        for i in range(d.ngroups):
            ds.group_end[i] = d.group_end[i] - lo
        return ds

    def _adam_keep(self):
        return (self.P32, self.G_OPT, self.M, self.V, self.VMAX, self.P16, self.opt_state)

    def _adam_call(self, d):
        return ops.Call("vqa_adamw_amsgrad", ctypes.byref(d), desc=d, keep=self._adam_keep())

    def adam_range_call(self, lo, hi):
        """The fused AdamW-amsgrad pass over flat parameters [lo, hi) only (the step's device
        state: clip coefficient, schedule, bias corrections; no-op unless an update is pending)."""
        return self._adam_call(self._adam_range_desc(lo, hi))

    def configure_optimizer(self, group_lr=None, warmup=None, total=None, max_norm=None, weight_decay=None,
                            betas=None, eps=None):
        """Re-plan the clip + AdamW + schedule tail (faster_rcnn_vqa_trainer.py:231-287 knobs)."""
        if group_lr:
            self.group_lr.update(group_lr)
        if warmup is not None:
            self.warmup = int(warmup)
        if total is not None:
            self.total = int(total)
        if max_norm is not None:
            self.max_norm = float(max_norm)
        if weight_decay is not None:
            self.wd = float(weight_decay)
        if betas is not None:
            self.betas = tuple(betas)
        if eps is not None:
            self.eps = float(eps)
        self._replan_optimizer()

    def _replan_optimizer(self):
        """Plan the optimizer tail again from the current settings; a captured step graph holds
        the old calls and is dropped."""
        self.opt_calls = []
        self._plan_optimizer()
        self.graph = None

    def _optim_scalars(self):
        """The clip and schedule scalars of vqa_optim_finalize (and vqa_grad_sqnorm_final), in
        argument order."""
        return (float(self.grad_scale), float(self.max_norm), int(self.warmup), int(self.total),
                float(self.betas[0]), float(self.betas[1]))

    def _finalize_call(self, ws, parts):
        """vqa_optim_finalize over the `parts` squared-norm partials in `ws`."""
        return ops.Call("vqa_optim_finalize", ops.addr(ws), parts, *self._optim_scalars(), ops.addr(self.opt_state),
                        keep=(ws, self.opt_state))

    # ------------------------------------------------------------------ execution
    def set_training(self, mode=True):
        """model.train() / model.eval(): the dropout kernels read this device flag at run
        time, so captured graphs stay valid."""
        self.RNG[2].fill_(1 if mode else 0)

    def forward(self):
        self._run(self.fwd_calls)

    def backward(self):
        self._run(self.bwd_calls)

    def optimizer_step(self):
        self._run(self.opt_calls)

    def autotune(self, reps=5, table=None, save=None, cold=False):
        """Pick the fastest (tile config, split-K) of every prepared GEMM of _tune_calls()
        (tune.autotune); the captured graphs hold the old choices and are dropped."""
        chosen = tune.autotune(self, self._tune_calls(), reps=reps, table=table, save=save, cold=cold)
        self.graph = None
        self.eval_graph = None
        return chosen

    # ------------------------------------------------------------------ evaluation graph
    # valid_one_epoch / generate_answers of the reference (trainer/faster_rcnn_vqa_trainer.py:
    # 408-480): the forward in eval mode, top-k of the log-probs and the epoch's loss / accuracy /
    # WUPS sums, as one replayed forward-only graph ending in vqa_eval_rows.  The graph leaves out
    # the forward's leading vqa_rng_advance: the reference's model.eval() forward draws no random
    # numbers, so an evaluation between two training steps must not move the dropout counter.
    EVAL_CAPACITY = 1 << 16

    def _eval_setup(self, rollout):
        """Hook of eval_plan: raise ValueError if this engine may not evaluate (with `rollout`:
        with the attention rollout in the step), and prepare what its evaluation step needs
        beyond the shared vqa_eval_rows tail."""
        if rollout:
            raise ValueError("rollout=True: this engine has no attention rollout (VitVQAEngine has)")

    def _eval_heat_setup(self, heatmap):
        """Hook of eval_plan: raise ValueError if this engine has no feature heat map, else
        prepare the call its evaluation step issues when `heatmap` is set."""
        if heatmap:
            raise ValueError("heatmap=True: this engine has no CNN feature map (VQAEngine has; the ViT model's "
                             "heat map is rollout=True)")

    def _run_eval_streams(self):
        """Hook: issue the evaluation step's calls on the current stream -- the forward without
        its rng advance, then self.eval_call."""
        raise NotImplementedError

    def _new_graph(self):
        return torch.cuda.CUDAGraph(keep_graph=self._keep_graph)

    def eval_plan(self, topk=5, similarity=None, capacity=None, rollout=False, heatmap=False):
        """Allocate the evaluation outputs -- TOPK_IDX / TOPK_LOGP [B, topk], and one int32 buffer
        EVAL_BUF = accumulator block (64 bytes) | prediction log | target log, `capacity` rows
        each -- upload the [A, A] similarity table if one is given, and prepare the
        vqa_eval_rows call over LOGP / TGT / NLL / LOSS.  rollout: the step also computes the
        attention rollout of its images (VitVQAEngine); heatmap: the heat map of its vision map, into
        HEAT [B, fh, fh] (VQAEngine).  Drops an evaluation graph."""
        self._eval_setup(bool(rollout))
        self._eval_heat_setup(bool(heatmap))
        if not 1 <= int(topk) <= L.EVAL_MAX_K:
            raise ValueError(f"topk={topk}: vqa_eval_rows supports 1..{L.EVAL_MAX_K}")
        capacity = self.EVAL_CAPACITY if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError(f"capacity={capacity} must be >= 0")
        from .metrics import check_similarity
        sim = check_similarity(similarity, self.A)
        k = int(topk)
        with torch.cuda.device(self.dev):
            self.TOPK_IDX, self.TOPK_LOGP = self._t((self.B, k), torch.int32, zero=True), self._t((self.B, k), zero=True)
            self.EVAL_BUF = self._t(16 + 2 * capacity, torch.int32, zero=True)
            self.EVAL_SIM = None if sim is None else torch.from_numpy(sim).to(self.dev)
        d = L.EvalDesc()
        d.logp, d.targets, d.nll, d.loss = (ops.addr(t) for t in (self.LOGP, self.TGT, self.NLL, self.LOSS))
        d.similarity = ops.addr(self.EVAL_SIM)
        d.batch, d.answers, d.k = self.B, self.A, k
        d.topk_idx, d.topk_logp = ops.addr(self.TOPK_IDX), ops.addr(self.TOPK_LOGP)
        d.acc = ops.addr(self.EVAL_BUF)
        d.pred_log, d.tgt_log = ops.addr(self.EVAL_BUF, 16), ops.addr(self.EVAL_BUF, 16 + capacity)
        d.capacity = capacity
        keep = (self.LOGP, self.TGT, self.NLL, self.LOSS, self.TOPK_IDX, self.TOPK_LOGP, self.EVAL_BUF) + \
            (() if self.EVAL_SIM is None else (self.EVAL_SIM,))
        self.eval_call = ops.Call("vqa_eval_rows", ctypes.byref(d), keep=keep, desc=d)
        self.eval_k, self.eval_capacity, self.eval_rollout = k, capacity, bool(rollout)
        self.eval_heatmap = bool(heatmap)
        self.eval_graph = None

    def eval_prepare(self, topk=5, similarity=None, capacity=None, graph=True, rollout=False, heatmap=False):
        """Make the evaluation plan (and, with `graph`, its graph) match the arguments, reusing
        what exists: a new table of an engine that already has one is copied into place."""
        from .metrics import check_similarity
        sim = check_similarity(similarity, self.A)
        if capacity is None:                               # keep the planned capacity
            capacity = self.eval_capacity if self.eval_call is not None else self.EVAL_CAPACITY
        cap = int(capacity)
        same = (self.eval_call is not None and self.eval_k == int(topk) and self.eval_capacity == cap
                and (sim is None) == (self.EVAL_SIM is None) and self.eval_rollout == bool(rollout)
                and self.eval_heatmap == bool(heatmap))
        if not same:
            self.eval_plan(topk, sim, cap, rollout, heatmap)
        elif sim is not None:
            _h2d(self.EVAL_SIM, sim)
        if graph and self.eval_graph is None:
            self.eval_capture_graph()

    def eval_capture(self, topk=5, similarity=None, capacity=None, rollout=False, heatmap=False):
        """Plan (eval_plan) and capture the evaluation graph.  The warm-up launch outside the
        capture leaves RNG, opt_state and the accumulators as it found them.  The training graph
        is untouched: both live on one engine; configure_optimizer / use_global_rows re-plan
        calls this graph does not hold."""
        self.eval_plan(topk, similarity, capacity, rollout, heatmap)
        self.eval_capture_graph()

    def eval_capture_graph(self):
        self.flush_optimizer()           # the graph reads the parameters: no update may be pending
        s = torch.cuda.Stream(self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        saved = (self.opt_state.clone(), self.RNG.clone(), self.EVAL_BUF.clone())
        with torch.cuda.stream(s):
            self._run_eval_streams()                    # warm-up launch outside the capture
        torch.cuda.current_stream(self.dev).wait_stream(s)
        torch.cuda.synchronize(self.dev)
        g = self._new_graph()
        with no_gc_capture():
            with torch.cuda.graph(g, stream=s):
                self._run_eval_streams()
        for dst, src in zip((self.opt_state, self.RNG, self.EVAL_BUF), saved):
            dst.copy_(src)
        if self._keep_graph:
            g.instantiate()
        self.eval_graph = g

    def eval_step(self, use_graph=True):
        """Evaluate the loaded batch (load_batch): a pending deferred AdamW update is applied
        first, the training flag RNG[2] is 0 while the step runs and gets its previous value
        back (the kernels read it at run time, so one graph serves both modes), and the step
        adds to the accumulators.  No host sync.  use_graph=False issues the same calls eagerly."""
        if self.eval_call is None or (use_graph and self.eval_graph is None):
            raise RuntimeError("eval_step: call eval_capture() (or eval_plan() for use_graph=False) first")
        self.flush_optimizer()
        flag = self.RNG[2:3]
        was = flag.clone()
        flag.zero_()
        if use_graph:
            self.eval_graph.replay()
        else:
            self._run_eval_streams()
        flag.copy_(was)

    def eval_reset(self):
        """Zero the accumulators and the log cursor (the start of an evaluation epoch)."""
        self.EVAL_BUF[:16].zero_()

    def eval_result(self):
        """The epoch's one device -> host read: the accumulator words by name (Python ints and
        floats) and the logged `predictions` / `targets` of the valid rows, in order, up to the
        log capacity (cursor > capacity: the rows past it were counted but not logged)."""
        h = self.EVAL_BUF.cpu().numpy()
        out = {n: int(v) for n, v in zip(L.EVAL_ACC_INTS, h[:10].view(np.int64))}
        out.update({n: float(v) for n, v in zip(L.EVAL_ACC_F64, h[10:16].view(np.float64))})
        n, cap = min(out["cursor"], self.eval_capacity), self.eval_capacity
        out["predictions"] = h[16:16 + n].tolist()
        out["targets"] = h[16 + cap:16 + cap + n].tolist()
        return out

    # ------------------------------------------------------------------ readouts (tests / API)
    def forward_backward(self, batch):
        self.load_batch(batch)
        self.forward()
        self.backward()
        torch.cuda.synchronize(self.dev)
        return self.LOGP[:self.rows].cpu().numpy(), float(self.LOSS.item())

    def grad_norm(self):
        return float(self.G_OPT.double().norm()) * self.grad_scale

    def group_grad_norms(self):
        return {g: float(self.G_OPT[a:e].double().norm()) * self.grad_scale for g, (a, e) in self.lay.groups.items()}

    def last_grad_norm(self):
        return float(self.opt_state[L.ST_GRAD_NORM].item())

    def state_dict(self):
        """Reference-layout state_dict (SURVEY Appendix B keys), fp32 numpy."""
        self.flush_optimizer()
        sd = dict(self._frozen)
        sd.update(self.lay.unpack(self.P32.cpu().numpy()))
        return {k: sd[k] for k in self._model_specs()}

    def optimizer_state(self):
        """AdamW(amsgrad) state in reference layout: ({key: exp_avg}, {key: exp_avg_sq},
        {key: max_exp_avg_sq}, step, dropout RNG {seed, counter, training}) over the trainable
        keys.  The pending deferred update is applied first, as state_dict() does."""
        self.flush_optimizer()
        torch.cuda.synchronize(self.dev)
        unpack = lambda t: {k: v for k, v in self.lay.unpack(t.cpu().numpy()).items() if k not in self.TIED}  # noqa: E731
        return (unpack(self.M), unpack(self.V), unpack(self.VMAX), float(self.opt_state[L.ST_STEP].item()),
                self.RNG.cpu().numpy().copy())

    def load_optimizer_state(self, exp_avg, exp_avg_sq, max_exp_avg_sq, step, rng=None):
        """Restore what optimizer_state() returned (keys missing from the dicts: zero state)."""
        self.flush_optimizer()
        specs = self._model_specs()
        zeros = {k: np.zeros(specs[k], np.float32) for k in self._trainable_keys()}
        for arena, st in ((self.M, exp_avg), (self.V, exp_avg_sq), (self.VMAX, max_exp_avg_sq)):
            full = dict(zeros)
            full.update({k: np.asarray(v, np.float32) for k, v in st.items() if k in full})
            arena.copy_(torch.from_numpy(self.lay.pack(full)))
        self.opt_state.zero_()
        self.opt_state[L.ST_STEP] = float(step)
        if rng is not None:
            self.RNG.copy_(torch.as_tensor(np.asarray(rng).astype(np.uint32).view(np.int32)))
        torch.cuda.synchronize(self.dev)

    def param_view(self, key):
        """(parameter, gradient) device views of reference state-dict entry `key` inside the
        flat fp32 arenas (no copy: they alias the engine's live weights / gradients; a tied key
        aliases the segment of the key it is tied to).  The q|k|v and k|v stacks are row blocks,
        so their parts are exact reference-shaped views; the ConvTranspose2d scaler is stored as
        the flipped conv weight, so its view has the kernel layout [768, 3, 3, Cin] (layout.py).
        None if `key` is frozen or unknown."""
        specs = self._model_specs()
        key = self.TIED.get(key, key)
        for sg in self.lay.segments.values():
            if key not in sg.parts:
                continue
            p32, g32 = self.p32[sg.name], self.g32[sg.name]
            if sg.kind == "convT":
                return p32, g32
            if sg.kind == "flat":
                return p32.view(specs[key]), g32.view(specs[key])
            row = 0
            for part in sg.parts:
                n = specs[part][0]
                if part == key:
                    return p32[row:row + n].view(specs[key]), g32[row:row + n].view(specs[key])
                row += n
        return None

    def refresh_shadow(self):
        """Re-derive the bf16 GEMM shadow from the fp32 masters (after writing weights through
        param_view / ParameterGroup views)."""
        self.P16.copy_(self.P32)
