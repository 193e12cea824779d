"""VQAEngine: the MI355X training step of `ResnetVQAModel` as an explicit,
statically planned schedule of libvqa_hip kernel calls.

Mirrors, op for op:
  forward   ResnetVQAModel.forward            model/resnet_vqa_model.py:101-165
            SGA.forward                        model/multi_head_vision_text_attn.py:145-158
            T5Stack (encoder, eval)            TF/models/t5/modeling_t5.py:640-751
  backward  loss.backward()                    trainer/faster_rcnn_vqa_trainer.py:397
  step      clip_grad_norm_ + AdamW + sched    trainer/faster_rcnn_vqa_trainer.py:399-404

Design (MI355X-first, not a translation of eager PyTorch):
  * every trainable parameter, gradient and AdamW state lives in one flat fp32
    arena (layout.ParamLayout) + a bf16 shadow for GEMM operands, so the clip
    norm and AdamW are single HBM passes and DP all-reduces one contiguous
    buffer;
  * the frozen ResNet is BN-folded, bf16, NHWC, run as implicit-GEMM convs
    (no im2col buffers); the ConvTranspose2d scaler is an implicit GEMM over
    the layer4 map whose rows are already the [B, HW, 768] token order the
    reference obtains with view+permute (:142-143);
  * activations/workspaces are allocated once for a fixed (B, L, H), every
    kernel call is prepared once with fixed device addresses, and the whole
    step is replayed as one hipGraph (torch.cuda.CUDAGraph capture);
  * dropout (p = 0.1 at the reference's 12 sites per step) is
    applied inside the producing kernels from a stateless counter hash
    (include/vqa_hip.h "dropout"); the backward regenerates the masks, nothing
    is stored.  dropout=0 gives eval-mode numerics (golden-vector parity).

This module holds what is the ResNet engine's own: the frozen-ResNet plan, the scaler and head
calls, the fp8 arenas, the deferred and row-split optimizer plan, the stream schedule of the step,
graph capture and the evaluation graph.  The SGA blocks are planned by sga_stack.SGAStack, the T5
encoder by t5_stack.T5Stack, the plan the ViT engine's stacks use too; what this engine adds to
the latter is its own: activations stacked per layer and one gradient slot
per layer, so that the weight gradients run per group of layers as batched launches on the side
stream (t5_dw_group, _t5_group_dw; t5_dw_groups is its one form: the list of group sizes, or
None for paired dX + dW per layer), the ready marks between groups, and opt-in fuse_norm.  The
arenas, the call builders, the AdamW descriptors and the state-dict / optimizer-state readouts
are engine_base.EngineBase's, shared with vit_engine.VitVQAEngine; the GEMM tuner is tune.py.
The stacks issue the calls the engines' own plans issued.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import lib as L
from . import ops
from . import synthetic as S
from .engine_base import (BF16, F32, I64, IGNORE_INDEX, SITE_EMBED, SITE_FINAL, EngineBase, _after,  # noqa: F401
                          _check_attn_path, _h2d, _Seq, batch_rows, load_rows, load_rows_multi, no_gc_capture,
                          t5_site)       # (_check_attn_path, _h2d and sga_site: re-exported, tests/test_api_cpu.py)
from .layout import ParamLayout, fold_bn, t5_bucket_map
from .sga_stack import SGAGrads, SGAStack, sga_site  # noqa: F401
from .t5_stack import T5Grads, T5Stack


def stem_s2d_weight(wf):
    """The 7x7 stride-2 stem conv weight [Cout, 7, 7, 3] (NHWC order) as the 4x4 stride-1
    weight [Cout, 4, 4, 16] over vqa_image_to_s2d16's image:
    W'[o, a, e, (2p+q)*3 + c] = W[o, 2a+p, 2e+q, c], zero where 2a+p or 2e+q is 7."""
    co, kh, kw, ci = wf.shape
    w8 = np.zeros((co, 8, 8, ci), np.float32)
    w8[:, :kh, :kw] = wf
    w = w8.reshape(co, 4, 2, 4, 2, ci).transpose(0, 1, 3, 2, 4, 5).reshape(co, 4, 4, 4 * ci)
    return np.concatenate([w, np.zeros((co, 4, 4, 16 - 4 * ci), np.float32)], 3)


def accum_spans(rows, batch, k):
    """The (lo, hi) row spans of the k micro-batches of a `rows`-row global batch, `batch` rows
    planned per micro-batch: a contiguous split, full micro-batches first, then the remainder,
    then empty ones (lo == hi).  1 <= rows <= k x batch."""
    rows, batch, k = int(rows), int(batch), int(k)
    if batch < 1 or k < 1:
        raise ValueError(f"accum_spans: batch={batch} and k={k} must be >= 1")
    if not 1 <= rows <= k * batch:
        raise ValueError(f"global batch of {rows} rows: {k} micro-batches of {batch} rows take 1..{k * batch}")
    return [(min(j * batch, rows), min((j + 1) * batch, rows)) for j in range(k)]


class StepTail:
    """The calls of the step's tail, each planned once (VQAEngine._plan_optimizer) and taken by
    name; the three forms the steps run are lists of these names.
      sq_a, sq_b, sq_c   vqa_grad_sqnorm partials of [0, a), [a, rel-bias) and [rel-bias, n)
      finalize           vqa_optim_finalize over the three
      after              what follows finalize in the dense form: the whole AdamW pass and the e4m3
                         copies, or with a deferred update the [rel-bias, n) range
      mark, rows_rest    embed_split: vqa_embed_mark of the step's ids; the untouched rows (grid 256)
      relbias, rows_touched          ... the rel-bias-only range; the touched rows (grid 1)
      sort, scatter      fused_tail: the embedding scatter's id sort; the scatter over the sorted ids
      sq_final           ... vqa_grad_sqnorm_final: sq_b + sq_c + finalize in one launch"""
    mark = rows_rest = relbias = rows_touched = sort = scatter = sq_final = None

    def __init__(self, sq_a, sq_b, sq_c, finalize):
        self.sq_a, self.sq_b, self.sq_c, self.finalize = sq_a, sq_b, sq_c, finalize
        self.after = []

    @property
    def dense(self):
        """opt_calls: eager steps."""
        return [self.sq_a, self.sq_b, self.sq_c, self.finalize] + self.after

    @property
    def split(self):
        """tail_calls_unfused: what follows sq_a and sq_b when the untouched rows ran earlier
        (dp.DataParallelStep's and the accumulated step's finish graphs); without the row split
        the rest of the dense form."""
        if self.rows_touched is None:
            return [self.sq_c, self.finalize] + self.after
        return [self.sq_c, self.finalize, self.relbias, self.rows_touched]

    @property
    def short(self):
        """tail_calls: what the stream / graph step runs after run_backward_streams."""
        if self.sq_final is None:
            return self.split
        return [self.sq_final, self.relbias, self.rows_touched]


class VQAEngine(EngineBase):
    def __init__(self, state_dict, vision="resnet50", batch=64, seq_len=32, image_size=224, device="cuda:0",
                 warmup=10, total=100, num_blocks=3, answer_spaces=170, grad_scale=1.0, max_norm=1.0,
                 betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1, dropout=0.1, seed=0, pipeline=False,
                 t5_dw_group=None, defer_optimizer=True, dw_stream=None, sga_dw_batch=True, pair_bwd=True,
                 language_model="t5-base", fp8=False, sga_attn_group=True, fuse_norm=None):
        super().__init__(device, dropout, seed, warmup, total, max_norm, betas, eps, weight_decay, grad_scale)
        # fuse_norm: every forward LayerNorm / RMSNorm but layer 0's ln0 runs as the tail of the
        # GEMM that writes its input (vqa_gemm_desc.norm) instead of as a launch of its own;
        # same bits.  Opt-in; None reads the environment (VQA_FUSE_NORM=1).
        self.fuse_norm = (os.environ.get("VQA_FUSE_NORM", "0") == "1") if fuse_norm is None else bool(fuse_norm)
        self.fuse_norm_kept = []          # norms left stand-alone although fuse_norm is on: none (always empty)
        # pipeline: the frozen ResNet (no trainable input) of the NEXT batch runs on its own
        # stream beside this step's T5 / SGA / backward / optimizer (see train_step)
        self.pipeline = bool(pipeline)
        # where the pipelined step issues the next batch's ResNet (_step_pipelined: first | last |
        # interleave | root; bench.py sets both), and how many of its calls lead an interleave
        self.res_order, self.res_head = "first", 4
        self._res_feed = None             # res_order "interleave": [calls left, stream handle] while a step is issued
        self._rstream_handle = None       # set_res_cumask: the CU-masked ResNet stream ...
        self._rstream_plain = None        # ... and the engine's own, put back by reset_res_cumask
        self.EMB_MARK = None              # row marks of the split embedding update (_plan_optimizer)
        self.SQ_CNT = None                # arrival counter of vqa_grad_sqnorm_final (_plan_optimizer)
        self.heat_call = None             # vqa_channel_cam over F4 (_plan_heat)
        self._fpn_plan = None             # faster-rcnn: the pyramid's call list and maps (fpn_maps)
        self.vision, self.B, self.L, self.H = vision, batch, seq_len, image_size
        assert image_size % 2 == 0, "the space-to-depth stem needs an even image size"
        self.NB, self.A = num_blocks, answer_spaces
        # widths: t5-base (the reference) or t5-large (BASELINE configs[4]: the SGA blocks, scaler,
        # pooler and classifier at the language model's width, synthetic.LM_DIMS)
        self.dims = dm = S.lm_dims(language_model)
        self.D, self.nl, self.h5, self.dkv, self.dff = dm.d_model, dm.t5_layers, dm.t5_heads, dm.t5_dkv, dm.t5_dff
        self.sga_heads, self.sga_dh = dm.sga_heads, dm.sga_dhead
        assert self.h5 * self.dkv == self.D and self.sga_heads * self.sga_dh == self.D
        # fp8: the forward weight GEMMs of the T5 layers and SGA blocks on e4m3 operands (BASELINE
        # configs[4] "fp8 MFMA weights"): weights and their input activations quantised row-wise
        # (vqa_quant_rows_fp8), the backward on the bf16 shadows / saved bf16 activations
        self.fp8 = bool(fp8)
        # the answer head's log-softmax keeps one sample's answer logits in registers (head.hip:
        # A <= 1024; DAQUAR has 170) and the pooler one sample's tokens (L <= 64)
        if not 1 <= answer_spaces <= 1024:
            raise ValueError(f"answer_spaces={answer_spaces}: the fused answer head supports 1..1024 answers")
        if not 1 <= seq_len <= 64:
            raise ValueError(f"seq_len={seq_len}: the attention / pooler kernels support 1..64 question tokens")
        # dX + dW of a layer as one paired GEMM launch (pair_bwd=False: separate launches)
        self.pair_bwd = bool(pair_bwd)
        # T5 weight gradients: per weight ONE launch batched over a group of layers (the
        # layers' activations / gradients stacked at constant strides).  `t5_dw_group` is a
        # group size (1: dX + dW paired per layer; 12: one group) or a sequence of group sizes,
        # top layer first.  Default (single GPU): groups of 9 and 3 layers (3/4 and 1/4 of the
        # stack: 18 and 6 for t5-large), the batched weight
        # gradients on a side stream beside the remaining input-gradient chain (measured 6.66 vs
        # 6.78-6.84 ms per step against one group of 12 on the chain; tools/gpu/ab_env.sh).
        # DP passes (4, 4, 3, 1): the buckets become final, and are all-reduced, while the
        # backward runs, and the last, exposed bucket is one layer.
        if t5_dw_group is None:
            t5_dw_group = (3 * self.nl // 4, self.nl - 3 * self.nl // 4)
        # Kept in one form: the list of group sizes (a size G: [G, G, ..., remainder]), or None
        # for the paired per-layer form.
        if isinstance(t5_dw_group, (list, tuple)):
            self.t5_dw_groups = [int(x) for x in t5_dw_group]
        elif int(t5_dw_group) == 1:
            self.t5_dw_groups = None
        else:
            G = int(t5_dw_group)
            assert G > 1, "t5_dw_group: a group size >= 1 or a sequence of sizes"
            self.t5_dw_groups = [G] * (self.nl // G) + [self.nl % G] * (self.nl % G > 0)
        assert self.t5_dw_groups is None or (sum(self.t5_dw_groups) == self.nl and min(self.t5_dw_groups) >= 1)
        # SGA blocks' q2 / m2 / fc1 / fc2 weight gradients batched over the blocks
        self.sga_dw_batch = bool(sga_dw_batch)
        # the SGA blocks' self-attentions as ONE launch forward and ONE backward
        # (vqa_attn_desc.groups; False: one launch per block)
        self.sga_attn_group = bool(sga_attn_group)
        # AdamW of step k applied inside step k+1's forward (see _plan_optimizer)
        self.defer_opt = bool(defer_optimizer)
        # weight-gradient GEMMs (calls tagged `side`) on a stream of their own beside the
        # input-gradient chain (single GPU and DP alike; dp.DataParallelStep keeps the placement)
        self.dw_stream = True if dw_stream is None else bool(dw_stream)
        self.T = batch * seq_len
        self.rows = batch                 # real rows of the loaded batch (a short last batch is padded)
        self.lay = ParamLayout(vision, answer_spaces, num_blocks, dm)
        sd = S.upgrade_fpn_keys({k: np.asarray(v) for k, v in state_dict.items()})
        self._frozen = {k: v for k, v in sd.items() if k not in set(self.lay.trainable_keys)}
        with torch.cuda.device(self.dev):
            self._alloc_params(sd)
            self._plan_resnet(sd)
            self._alloc_activations()
            self.fwd_calls, self.bwd_calls, self.opt_calls, self.zero_calls = [], [], [], []
            self._plan_forward()
            self._plan_backward()
            self._plan_optimizer()
            self._run(self.quant_all)                     # e4m3 weights of the initial parameters
        self.allreduce = None            # set by the DP trainer: fn(G32 tensor) on the current stream
        self._side = torch.cuda.Stream(self.dev)
        self._wside = torch.cuda.Stream(self.dev)
        self._rstream = torch.cuda.Stream(self.dev)
        self.res_external = False        # set_res_cumask: the ResNet launched eagerly beside the graph
        self.allow_empty_rows = False     # use_global_rows (DP): a rank may get 0 rows
        self._img_rows_next = None        # pipelined: rows of the images whose features the next batch uses
        self.count_call = None
        # gradient accumulation (use_accumulation): micro-batches per optimizer step, the calls that
        # end a micro-batch (accumulate, advance), the launch that ends the step, rows of the last one
        self.accum, self.accum_calls, self.accum_finish, self.accum_rows = 1, [], None, 0

    @classmethod
    def from_state_dict(cls, sd, **kw):
        return cls(sd, **kw)

    # ------------------------------------------------------------------ allocation
    def _alloc_params(self, sd):
        self._alloc_arenas(sd)
        self.bucket = torch.from_numpy(t5_bucket_map(self.L, self.L)).reshape(-1).to(self.dev)

    def _alloc_shadow_arenas(self):
        if self.fp8:
            # e4m3 weight shadow and its row scales, at the fp32 arena's element offsets: row r of
            # segment s is W8[s.offset + r*K :] with scale WSC[s.offset + r] (constant strides
            # between the blocks' segments, as the batched launches need)
            self.W8 = torch.empty(self.lay.total, dtype=torch.uint8, device=self.dev)
            self.WSC = torch.ones(self.lay.total, dtype=F32, device=self.dev)
            self._xq = {}

    def _plan_resnet(self, sd):
        """Frozen torchvision ResNet (eval BN folded) as a list of implicit-GEMM convs; for
        faster-rcnn the FPN backbone's body and, behind it, the two convs of its 'pool' level."""
        self.res_calls = []
        self._res_keep = []
        self._res_body(sd, self.res_calls)

    def _res_body(self, sd, calls, pyramid=False):
        """The vision branch's calls appended to `calls`.  pyramid=False: the plan of the training
        and evaluation steps, which allocates IMG, the ping-pong buffers and F4 / F4N.
        pyramid=True (faster-rcnn, fpn_maps): a second list over the same IMG with buffers of its
        own -- the body with dedicated outputs for C2..C4, then the whole FPN; returns the five
        levels' NHWC bf16 maps."""
        B, H = self.B, self.H
        frcnn = self.vision == S.FASTER_RCNN
        assert frcnn or not pyramid
        self._conv_calls = calls                     # where _conv appends
        vm = S.vision_prefix(self.vision)
        fpn = "vision_model.fpn."

        def up(w, b):
            w16 = torch.from_numpy(np.ascontiguousarray(w)).to(self.dev).to(BF16)
            b32 = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(self.dev)
            self._res_keep += [w16, b32]
            return w16, b32

        def fpn_w(name):                             # a biased conv without a norm: [Cout, kh, kw, Cin]
            return up(sd[fpn + name + ".0.weight"].astype(np.float32).transpose(0, 2, 3, 1), sd[fpn + name + ".0.bias"])

        def conv_w(cname, bname, s2d=False):
            w = sd[vm + cname + ".weight"].astype(np.float32)
            wf, bf = fold_bn(w, sd[vm + bname + ".weight"], sd[vm + bname + ".bias"],
                             sd[vm + bname + ".running_mean"], sd[vm + bname + ".running_var"])
            wf = wf.transpose(0, 2, 3, 1)            # [Cout, kh, kw, Cin]
            if s2d:
                wf = stem_s2d_weight(wf)
            w16 = torch.from_numpy(np.ascontiguousarray(wf)).to(self.dev).to(BF16)
            b32 = torch.from_numpy(bf).to(self.dev)
            self._res_keep += [w16, b32]
            return w16, b32

        # geometry walk to size the ping-pong buffers
        arch = S.body_arch(self.vision)
        layers = S.RESNET_LAYERS[arch]
        bottleneck = arch == "resnet50"
        h1 = (H + 2 * 3 - 7) // 2 + 1
        h2 = (h1 + 2 - 3) // 2 + 1
        plan = []                                     # (kind, args)
        maxel = B * h1 * h1 * 64
        hh, cin = h2, 64
        for li, (planes, nblk) in enumerate(zip((64, 128, 256, 512), layers)):
            for bi in range(nblk):
                stride = (1 if li == 0 else 2) if bi == 0 else 1
                out = planes * 4 if bottleneck else planes
                ho = (hh + 2 - 3) // stride + 1
                maxel = max(maxel, B * hh * hh * planes, B * ho * ho * out)
                if bottleneck and bi == 0:            # the fused conv3 + downsample's [conv2 | x] rows
                    maxel = max(maxel, B * ho * ho * (planes + cin))
                plan.append((li, bi, stride, hh, ho, cin, planes, out))
                hh, cin = ho, out
        h5, c5 = hh, cin                              # layer4 spatial size / channels
        if frcnn:
            # the vision map is the FPN's 'pool' level: max_pool2d(P5, 1, 2) = P5[:, :, ::2, ::2]
            # = the 3x3 pad-1 conv of the lateral map at stride 2 (DESIGN: "Faster-RCNN backbone")
            hh, cin = (h5 - 1) // 2 + 1, S.FPN_CHANNELS
        bufs = [self._t(maxel, BF16) for _ in range(5)]
        hz = H // 2 + 1                               # space-to-depth stem image (vqa_image_to_s2d16)
        if pyramid:
            out_map = self._t((B, hh, hh, cin), BF16)
        else:
            self.fh, self.fc = hh, cin                # the vision map's spatial size / channels
            self.V_TOK = B * hh * hh
            self.IMG = self._t((B, 3, H, H))
            self.res_bufs = bufs
            self.F4 = self._t((B, hh, hh, cin), BF16)
            # pipelined: the ResNet writes the next batch's vision map here; each step first
            # moves it into F4 (read by the ConvTranspose2d forward and weight gradient)
            self.F4N = self._t((B, hh, hh, cin), BF16) if self.pipeline else self.F4
            # F4 <- F4N as a library kernel (a torch copy_ would put a runtime memcpy node in the graph)
            self.copy_f4 = ops.Call("vqa_copy", self.F4.data_ptr(), self.F4N.data_ptr(), self.F4.numel() * 2,
                                    keep=(self.F4, self.F4N))
            out_map = self.F4N

        # stem: conv7x7/2 + BN + ReLU, then maxpool 3x3/2
        # (as a 4x4 stride-1 conv over the space-to-depth image: K 256 instead of 7*7*8 = 392)
        w16, b32 = conv_w("conv1", "bn1", s2d=True)
        g = ops.conv_geom(B, hz, hz, 16, h1, h1, 4, 4, 1, 1)
        # the shape alone chooses the form: the fused kernel's tiles need H % 32 == 0 (then, H being
        # even, hz == h1 + 1 and h2 == h1 // 2 hold too)
        fused_img = H % 32 == 0
        # the space-to-depth image only exists for the form that reads it (B x hz x hz x 16 bf16)
        if not pyramid:
            self.IMG8 = None if fused_img else self._t((B, hz, hz, 16), BF16)
        if fused_img:
            # space-to-depth + stem + maxpool in one pass (csrc/stem.hip): patches staged from the
            # fp32 image, only the pooled map written; bit-identical to the three-kernel form below
            calls.append(ops.Call("vqa_stem_pool_img", self.IMG.data_ptr(), w16.data_ptr(), b32.data_ptr(),
                                  bufs[1].data_ptr(), B, H, keep=(self.IMG, w16, b32, bufs[1])))
        else:
            calls.append(ops.Call("vqa_image_to_s2d16", self.IMG.data_ptr(), self.IMG8.data_ptr(), B, H, H,
                                  keep=(self.IMG, self.IMG8)))
            self._gemm(calls, self.IMG8, w16, B * h1 * h1, 64, 256, lda=256, ldb=256, ga=g,
                       c16=bufs[0], ldc16=64, bias=b32, relu=True)
            calls.append(ops.Call("vqa_maxpool3x3s2_nhwc", bufs[0].data_ptr(), bufs[1].data_ptr(), B, h1,
                                  h1, 64, h2, h2, keep=(bufs[0], bufs[1])))
        x = bufs[1]
        free = [bufs[0], bufs[2], bufs[3], bufs[4]]
        nblocks_total = len(plan)
        own = []                                      # outputs with a buffer of their own: never recycled
        levels = []                                   # pyramid: (C2..C5 map, its size, its channels)
        for idx, (li, bi, stride, hi, ho, ci, planes, out) in enumerate(plan):
            p = f"layer{li + 1}.{bi}."
            pool = list(free)
            t1, t2, ds, y = pool[0], pool[1], pool[2], pool[3]
            end_of_layer = bi == layers[li] - 1
            if idx == nblocks_total - 1 and not frcnn:
                y = out_map
                own.append(y)
            elif pyramid and end_of_layer and li < 3:
                y = self._t((B, ho, ho, out), BF16)
                own.append(y)
            if pyramid and end_of_layer:
                levels.append((y, ho, out))

            def advance():                            # y becomes x; x and the unused buffers are free again
                return [b_ for b_ in [x] + pool if b_ is not y and not any(b_ is o for o in own)], y
            if bottleneck and (vm + p + "downsample.0.weight") in sd:
                # conv3 and the 1x1 downsample as ONE GEMM over the concatenated K (r05):
                # [conv2 out | x subsampled] . [W3 | Wd]^T + (b3 + bd), ReLU -- conv2 writes the
                # first `planes` columns of the `ds` buffer, vqa_subsample_nhwc the other `ci`;
                # the downsample's output never goes to HBM and one launch goes away
                kc = planes + ci
                w, b = conv_w(p + "conv1", p + "bn1")
                self._conv(x, (B, hi, hi, ci), w, b, 1, 0, t1, relu=True)
                w, b = conv_w(p + "conv2", p + "bn2")
                self._conv(t1, (B, hi, hi, planes), w, b, stride, 1, ds, relu=True, ldc16=kc)
                calls.append(ops.Call("vqa_subsample_nhwc", x.data_ptr(), B, hi, hi, ci, stride,
                                      ops.addr(ds, planes), kc, keep=(x, ds)))
                w3, b3 = conv_w(p + "conv3", p + "bn3")
                wd, bd = conv_w(p + "downsample.0", p + "downsample.1")
                wcat = torch.cat([w3.reshape(out, planes), wd.reshape(out, ci)], dim=1).contiguous()
                bcat = b3 + bd
                self._res_keep += [wcat, bcat]
                assert B * ho * ho * kc <= ds.numel(), "fused downsample: the [conv2 | x] rows exceed the buffer"
                self._gemm(calls, ds, wcat, B * ho * ho, out, kc, lda=kc, ldb=kc, c16=y, ldc16=out,
                           bias=bcat, relu=True)
                free, x = advance()
                continue
            if bottleneck:
                w, b = conv_w(p + "conv1", p + "bn1")
                self._conv(x, (B, hi, hi, ci), w, b, 1, 0, t1, relu=True)
                w, b = conv_w(p + "conv2", p + "bn2")
                self._conv(t1, (B, hi, hi, planes), w, b, stride, 1, t2, relu=True)
                last_in, last_c, last_h = t2, planes, ho
                w3, b3 = conv_w(p + "conv3", p + "bn3")
            else:
                w, b = conv_w(p + "conv1", p + "bn1")
                self._conv(x, (B, hi, hi, ci), w, b, stride, 1, t1, relu=True)
                last_in, last_c, last_h = t1, planes, ho
                w3, b3 = conv_w(p + "conv2", p + "bn2")
            res = x
            if (vm + p + "downsample.0.weight") in sd:
                w, b = conv_w(p + "downsample.0", p + "downsample.1")
                self._conv(x, (B, hi, hi, ci), w, b, stride, 0, ds, relu=False)
                res = ds
            k3 = 1 if bottleneck else 3
            self._conv(last_in, (B, last_h, last_h, last_c), w3, b3, 1, 1 if k3 == 3 else 0, y, relu=True,
                       res16=res)
            free, x = advance()
        if not frcnn:
            return None
        # FPN (torchvision FeaturePyramidNetwork.forward): x is C5.  last = inner3(C5); its 'pool'
        # level, read by the model, is layer3's 3x3 conv taken at stride 2
        fc_ = S.FPN_CHANNELS
        lat = free[0] if not pyramid else self._t((B, h5, h5, fc_), BF16)
        w, b = fpn_w("inner_blocks.3")
        self._conv(x, (B, h5, h5, c5), w, b, 1, 0, lat, relu=False)
        w3, b3 = fpn_w("layer_blocks.3")
        self._conv(lat, (B, h5, h5, fc_), w3, b3, 2, 1, out_map, relu=False)
        if not pyramid:
            return None
        maps = {"pool": out_map, "3": self._t((B, h5, h5, fc_), BF16)}
        self._conv(lat, (B, h5, h5, fc_), w3, b3, 1, 1, maps["3"], relu=False)
        last, hl = lat, h5
        for i in (2, 1, 0):
            # last = inner_i(C_{i+2}) + nearest-2x(last): the upsampled map is the lateral GEMM's
            # bf16 residual, so the sum is taken in fp32 and rounded once
            c, hc, cc = levels[i]
            assert hc == 2 * hl, "the FPN's top-down path is planned for exact 2x upsamples (image_size % 32 == 0)"
            ups, nxt = self._t((B, hc, hc, fc_), BF16), self._t((B, hc, hc, fc_), BF16)
            self._call(calls, "vqa_upsample2x_nhwc", last, ups, B, hl, hl, fc_)
            w, b = fpn_w(f"inner_blocks.{i}")
            self._conv(c, (B, hc, hc, cc), w, b, 1, 0, nxt, relu=False, res16=ups)
            w, b = fpn_w(f"layer_blocks.{i}")
            maps[str(i)] = self._t((B, hc, hc, fc_), BF16)
            self._conv(nxt, (B, hc, hc, fc_), w, b, 1, 1, maps[str(i)], relu=False)
            last, hl = nxt, hc
        return maps

    def _conv(self, x, shape, w16, b32, stride, pad, out, relu, res16=None, ldc16=None):
        n, h, w, c = shape
        cout, kh, kw, _ = w16.shape
        oh = (h + 2 * pad - kh) // stride + 1
        g = ops.conv_geom(n, h, w, c, oh, oh, kh, kw, stride, pad)
        if kh == 1 and kw == 1 and stride == 1 and pad == 0:
            g = None                                   # a 1x1/1 conv is a plain GEMM over the NHWC rows
        # 3x3 / stride 1: the LDS-patch convolution (a_conv = 2), weights reordered to
        # [Cout][C/64][9][64]; any W <= 64 has a patch tile that fits (conv_patch.inl patch_fits)
        patch = kh == 3 and kw == 3 and stride == 1 and pad == 1 and c % 64 == 0 and 14 <= w <= 64
        if patch:
            w16 = w16.reshape(cout, 9, c // 64, 64).permute(0, 2, 1, 3).contiguous().reshape(cout, kh, kw, c)
            self._res_keep.append(w16)
        self._gemm(self._conv_calls, x, w16, n * oh * oh, cout, kh * kw * c, lda=kh * kw * c, ldb=kh * kw * c, ga=g,
                   c16=out, ldc16=ldc16 or cout, bias=b32, relu=relu, res16=res16, ldres=cout, a_patch=patch)

    def _alloc_activations(self):
        D = self.D
        B, Lq, T, V = self.B, self.L, self.T, self.V_TOK
        t = self._t
        # inputs
        self.IDS = t((B, Lq), I64, zero=True)
        self.IDS_PREV = t((B, Lq), I64, zero=True)     # ids whose embedding-gradient rows are nonzero
        self.MASK = t((B, Lq), I64, zero=True)
        self.TGT = t((B,), I64, zero=True)
        # vision tokens
        self.VIS32, self.VIS16 = t((V, D)), t((V, D), BF16)
        # T5 encoder: the GEMM inputs its weight gradients read are stacked in backward order (slot =
        # 11 - layer) so a group of consecutive layers' dW is one batched launch with constant strides
        self.t5 = T5Stack(self, "t5.", T, Lq, self.nl, self.h5, self.dkv, self.dff, D, self.IDS, self.MASK,
                          self.bucket, t5_site, (2, 3), SITE_EMBED, SITE_FINAL, embed="t5.embed", stacked=True)
        self.TXT32, self.TXT16 = self.t5.OUT32, self.t5.OUT16
        # arrival counters of the norm-carrying GEMMs (zero-filled, left zero by every launch): one
        # block for the T5 encoder's chain and one for the SGA blocks'.  Each chain is serial on
        # its stream; the two never overlap (the fusion segment starts after the text branch has
        # joined), and neither the vision branch beside the encoder nor the pipelined ResNet of
        # the next batch has a norm-carrying GEMM
        self.NORM_WS = [torch.zeros(65536 // 4, dtype=torch.int32, device=self.dev) for _ in range(2)] \
            if self.fuse_norm else (None, None)
        self.sga_stack = SGAStack(self, self.TXT32, self.TXT16, self.VIS16, self.NORM_WS[1])
        self.sga, self.P1A, self.O1A = self.sga_stack.blocks, self.sga_stack.P1A, self.sga_stack.O1A
        # head
        self.ATT, self.POOLED = t((B, Lq)), t((B, D))
        self.LOGP, self.NLL, self.LOSS = t((B, self.A)), t(B), t(1)
        self.ROWTOT = t(1, zero=True)     # DP: valid rows summed over the ranks (use_global_rows)
        # backward temporaries (reused layer to layer)
        self.dY = [t((T, D)), t((T, D))]
        self.dA32 = t((T, D))
        self.dC32 = t((T, D))
        self.dO16 = t((T, D), BF16)
        self.dTXT = t((T, D))
        self.dVIS32, self.dVIS16 = t((V, D)), t((V, D), BF16)
        self.dVIS9 = t((9, V, D), BF16)                 # its 3x3 tap-shifted copies (scaler dW)
        self.dH32 = t((T, D))
        self.dHM32 = t((T, D))
        self.WS_EMB = t(3 * T, torch.int32)
        lib = L.load()
        self.WS_COL2 = t(lib.vqa_colsum_workspace_floats(V, D))
        self.WS_HEAD = t(lib.vqa_head_workspace_floats(B, Lq, D, self.A))
        self.SQ_PARTS = 1024                              # per sqnorm range (three ranges, §3.7)
        self.WS_SQ = t(3 * self.SQ_PARTS, torch.float64)

    # ------------------------------------------------------------------ fp8 (config 5)
    FP8_T5 = ("qkv_w", "o_w", "wi", "wo")
    FP8_SGA = ("qkv1_w", "m1_w", "q2_w", "kv2_w", "m2_w", "fc1_w", "fc2_w")

    def _is_fp8(self, wname):
        return self.fp8 and wname.rsplit(".", 1)[-1] in (self.FP8_T5 + self.FP8_SGA)

    def _quant_weight(self, lst, wname, rows=None):
        """Row-wise e4m3 copy of weight `wname` (its fp32 master, `rows` rows from its offset:
        several side-by-side segments quantised as one matrix)."""
        sg = self.lay[wname]
        k = sg.shape[1]
        rows = sg.shape[0] if rows is None else rows
        self._call(lst, "vqa_quant_rows_fp8", ops.addr(self.P32, sg.offset), 0, k, rows, k, ops.addr(self.W8, sg.offset),
                   k, ops.addr(self.WSC, sg.offset), extra=(self.P32, self.W8, self.WSC))

    def _quant_act(self, lst, key, x16, rows):
        """e4m3 copy (+ row scales) of a bf16 GEMM input, into a buffer private to call site `key`."""
        k = x16.shape[-1]
        if key not in self._xq:
            self._xq[key] = (torch.empty(rows, k, dtype=torch.uint8, device=self.dev), self._t(rows))
        x8, xs = self._xq[key]
        self._call(lst, "vqa_quant_rows_fp8", x16, 1, k, rows, k, x8, k, xs)
        return x8, xs

    # ------------------------------------------------------------------ forward plan
    def _plan_forward(self):
        D = self.D
        f = self.fwd_calls
        B, Lq = self.B, self.L
        if self.p_drop > 0.0:                                # fresh dropout masks every step
            self._call(f, "vqa_rng_advance", self.RNG)
        self._fsplit = [len(f)]                              # [pre | vision | text | fusion]
        if not self.pipeline:                                # pipelined: res_calls run beside the step
            f += self.res_calls
        self._fvis_param = len(f)                            # first vision-branch call reading parameters
        # ConvTranspose2d scaler as implicit GEMM over the layer4 map (+bias) -> vision tokens
        cin, fh = self.fc, self.fh
        g = ops.conv_geom(B, fh, fh, cin, fh, fh, 3, 3, 1, 1)
        self._gemm(f, self.F4, self.p16["scaler_w"], self.V_TOK, D, 9 * cin, lda=9 * cin, ldb=9 * cin, ga=g,
                   c32=self.VIS32, ldc32=D, c16=self.VIS16, ldc16=D, bias=self.p32["scaler_b"])
        # SGA block 0's key/value projection reads only the vision tokens: it runs here, on the
        # vision branch beside the T5 encoder, instead of on the chain after it
        self.sga_stack.plan_kv0(self, f)
        self.sga_vision_calls = [f[-1]]                    # SGA work outside the fusion segment (bench)
        # T5 encoder (independent of the vision branch until the SGA blocks)
        self._fsplit.append(len(f))
        self.t5.plan_forward(self, f, fuse=self.NORM_WS[0])
        self._t5_layer_start = self.t5.layer_start
        self._fsplit.append(len(f))
        self.sga_stack.plan_forward(self, f)             # x = text always, y chained
        last = self.sga[-1]["OUT"]
        self._call(f, "vqa_head_fwd", last, self.p32["pool_w"], self.p32["pool_b"], self.p32["cls_w"],
                   self.p32["cls_b"], self.TGT, self.ATT, self.POOLED, self.LOGP, self.NLL, self.LOSS, B, Lq, D, self.A)

    # ------------------------------------------------------------------ backward plan
    def _plan_backward(self):
        D = self.D
        b = self.bwd_calls
        B, Lq, T, NB = self.B, self.L, self.T, self.NB
        # the dense embedding gradient only ever gets the touched rows written: re-zero the rows
        # the previous step wrote (IDS_PREV) instead of all 32128 x 768 floats (DP: dp.py swaps in
        # the gathered ids of every rank)
        z = self.g32["t5.embed"]
        self._call(self.zero_calls, "vqa_embedding_zero_rows", self.IDS_PREV, self.IDS, T, z, D, S.T5_VOCAB)
        b += self.zero_calls
        # head: log_softmax + NLL + classifier + attention pooler
        last = self.sga[-1]["OUT"]
        self._call(b, "vqa_head_bwd", last, self.ATT, self.POOLED, self.LOGP, self.TGT, self.p32["pool_w"],
                   self.p32["cls_w"], self.dY[(NB - 1) & 1], None, self.g32["pool_w"], self.g32["pool_b"],
                   self.g32["cls_w"], self.g32["cls_b"], self.WS_HEAD, B, Lq, D, self.A, self.NLL, self.LOSS,
                   None, 1.0)
        # ready marks: (number of backward calls issued, end of the gradient prefix now final).
        # The flat layout is in backward-completion order, so finished gradients always form
        # a prefix of G32: DP all-reduces bucket [prev_end, end) as soon as it is final.
        self.ready_marks = []
        self._sq_split = None        # (call index, prefix end) where the grad-norm pass can start early

        def mark(seg):
            self._flush(b)                          # finish this segment's deferred reductions first
            sg = self.lay[seg]
            self.ready_marks.append((len(b), sg.offset + (sg.numel + 63) // 64 * 64))
        mark("pool_b")
        self.sga_stack.plan_backward(self, b, SGAGrads(self.dY, self.dA32, self.dC32, self.dO16, self.dTXT,
                                                       self.dVIS32, self.dVIS16), mark)
        mark(f"sga{NB - 1}.m1_b")
        # ConvTranspose2d scaler weight/bias gradient (vision branch: independent of the T5
        # backward below; its own colsum workspace).  The flipped-conv weight column t*C + c
        # (tap t = ky*3 + kx) is sum_pos dVIS[pos] * F4[pos shifted by tap t]; shifting dVIS
        # the other way instead makes the 9 taps ONE batched GEMM over plain operands:
        # dW[:, t*C:(t+1)*C] = shift_t(dVIS)^T @ F4 (vqa_tap_shift; no implicit im2col gather)
        self._bsplit = [len(b)]
        cin, fh = self.fc, self.fh
        self._call(b, "vqa_tap_shift", self.dVIS16, self.dVIS9, B, fh, fh, D, 3, 3, 1)
        self._gemm(b, self.dVIS9, self.F4, D, cin, self.V_TOK, lda=D, ldb=cin, a_trans=True, b_trans=True,
                   c32=self.g32["scaler_w"], ldc32=9 * cin, batch=9, stride_a=self.V_TOK * D, stride_b=0,
                   stride_c32=cin, keep=(self.G32,))
        self.scaler_dw_call = b[-1]                       # bench roofline_gemm: the step's largest launch
        self._call(b, "vqa_colsum", self.dVIS32, 0, self.V_TOK, D, D, self.g32["scaler_b"], 0.0, self.WS_COL2)
        mark("scaler_b")
        self._bsplit.append(len(b))
        # T5 encoder backward.  dH32 is the gradient of the residual stream h_i; dH16 the
        # dropout-masked gradient of the FF branch that produced it (T5LayerFF :140).
        nl = self.nl
        # per-layer bf16 gradients the weight gradients read, stacked like the inputs (slot 11 - i)
        self.dH16S, self.dHMS = self._t((nl, T, D), BF16), self._t((nl, T, D), BF16)
        self.dFS, self.dQKVS = self._t((nl, T, self.dff), BF16), self._t((nl, T, 3 * D), BF16)
        grads = T5Grads(*([s[nl - 1 - i] for i in range(nl)] for s in (self.dH16S, self.dFS, self.dHMS, self.dQKVS)),
                        self.dTXT, self.dH32, self.dHM32, self.dC32, self.dO16)
        # grouped: the layers' input gradients chain alone and after every group of layers ONE
        # batched launch per weight (wo, wi, o, qkv) computes the group's weight gradients (4 x G
        # GEMMs of K = 2048 as 4 launches); else each layer's dX + dW as paired launches
        groups = self.t5_dw_groups
        size_at = {int(e): g for e, g in zip(np.cumsum(groups), groups)} if groups else {}   # layers done -> group

        def after_layer(i):
            if i == nl:                                     # the final norm
                mark("t5.final_ln")
            elif groups is None:
                mark(f"t5.{i}.ln1")
            elif nl - i in size_at:
                self._t5_group_dw(b, i + size_at[nl - i] - 1, i)
                mark(f"t5.{i}.ln1")
                if self._sq_split is None and i > 0:      # the first T5 dW group is final
                    self._sq_split = self.ready_marks[-1]
        self.t5.plan_backward(self, b, grads, self._dxdw if groups is None else self._dx_only, after_layer)
        mark("t5.relbias")
        self._flush(b)
        # embedding rows last (DP replaces this call by an all-gather of (id, dH row) pairs)
        self._call(b, "vqa_embedding_bwd", self.IDS, self.dH32, self.g32["t5.embed"], T, D, S.T5_VOCAB, self.WS_EMB)
        self.emb_call = b[-1]

    def _t5_group_dw(self, lst, i_hi, i_lo):
        """Weight gradients of T5 layers i_hi >= .. >= i_lo: per weight one launch batched over
        the layers (stack slot 11 - i, consecutive gradient segments at a constant stride)."""
        st = self.t5
        for w, dys, xs in (("wo", self.dH16S, st.FFS), ("wi", self.dFS, st.N1S), ("o_w", self.dHMS, st.OS),
                           ("qkv_w", self.dQKVS, st.N0S)):
            self._dw_batched(lst, dys, xs, [f"t5.{i}.{w}" for i in range(i_hi, i_lo - 1, -1)], self.T,
                             slot=self.nl - 1 - i_hi)

    # ------------------------------------------------------------------ optimizer plan
    def embed_mark_call(self, ids, rows):
        """vqa_embed_mark of `rows` token ids: EMB_MARK[id] = the step counter (the engine's own ids;
        dp.DataParallelStep: every rank's, gathered)."""
        return ops.Call("vqa_embed_mark", ids.data_ptr(), rows, S.T5_VOCAB, self.EMB_MARK.data_ptr(),
                        self.opt_state.data_ptr(), keep=(ids, self.EMB_MARK, self.opt_state))

    def _plan_optimizer(self):
        """Plans every call of the step's tail once, under a name on self.tail (StepTail, DESIGN
        §3.7 "step tail"), and sets the lists the steps run from its compositions."""
        n = self.lay.total
        # squared-norm partials: [0, a) is final once the first T5 weight-gradient group is (graph
        # steps run that part beside the backward's last layers), [a, rel-bias) once the deferred
        # column sums are flushed, the rel-bias + embedding-table range after the scatter
        e0 = self.lay["t5.relbias"].offset
        a = self._sq_split[1] if self._sq_split is not None else e0
        assert a % 4 == 0 and e0 % 4 == 0 and (n - e0) % 4 == 0 and a <= e0
        K = self.SQ_PARTS
        G = self.G_OPT                    # G32, or the accumulator (use_accumulation)
        sq = [ops.Call("vqa_grad_sqnorm", ops.addr(G, lo), hi - lo, ops.addr(self.WS_SQ, i * K), K,
                       keep=(G, self.WS_SQ)) for i, (lo, hi) in enumerate(((0, a), (a, e0), (e0, n)))]
        self.tail = t = StepTail(*sq, self._finalize_call(self.WS_SQ, 3 * K))
        self._adam_desc = self._adam_desc_full()
        self.adam_full = self._adam_call(self._adam_desc)
        # Deferred update (defer_opt): step k's AdamW runs inside step k+1's forward, one
        # parameter range at a time on its own stream, each range just before its first use
        # (the forward reads the layout back to front: T5 layers 0..11, then the scaler / SGA /
        # head).  The embedding table + rel-bias range is read by the forward's very first
        # calls, so it is applied at the end of step k instead (the T5 chain would otherwise
        # start behind its 0.9 GB pass).  Same arithmetic, same order of updates vs uses.
        # (With fuse_norm a T5 layer's wo GEMM reads the next layer's ln0 gain, so the layer
        # also waits for the next layer's range: _t5_waits.)
        lay = self.lay
        cuts = [("embed", e0, n)]
        for i in range(self.nl):
            lo = lay[f"t5.{i}.qkv_w"].offset if i < self.nl - 1 else lay["t5.final_ln"].offset
            hi = lay[f"t5.{i - 1}.qkv_w"].offset if i > 0 else e0
            cuts.append((f"t5.{i}", lo, hi))
        cuts.append(("scaler", lay["scaler_w"].offset, lay["t5.final_ln"].offset))
        cuts.append(("head", 0, lay["scaler_w"].offset))     # classifier, pooler, SGA
        assert sum(hi - lo for _, lo, hi in cuts) == n
        self.adam_cuts = {name: (lo, hi) for name, lo, hi in cuts}     # flat-arena range of each update
        # fp8: the e4m3 copies of the range's weights follow every AdamW range (and the whole
        # update when it is not deferred)
        quant = {name: [] for name, _, _ in cuts}
        self.quant_all = []
        if self.fp8:
            jobs = [(f"t5.{i}.{w}", None) for i in range(self.nl) for w in self.FP8_T5]
            jobs.append(("sga0.qkv1_w", self.NB * 3 * self.D))          # the blocks' side-by-side q|k|v
            jobs += [(f"sga{n}.{w}", None) for n in range(self.NB) for w in self.FP8_SGA if w != "qkv1_w"]
            for wname, rows in jobs:
                off = self.lay[wname].offset
                nm = next(name for name, lo, hi in cuts if lo <= off < hi)
                self._quant_weight(quant[nm], wname, rows)
                self.quant_all += quant[nm][-1:]
        self.adam_segs = []
        for name, lo, hi in cuts:
            c = self.adam_range_call(lo, hi)
            if quant[name]:
                c = _Seq([c] + quant[name])
            if name == "embed":
                self.adam_embed = c
            else:
                self.adam_segs.append((name, c))
        self.clear_pending = ops.Call("vqa_zero", ops.addr(self.opt_state, L.ST_PENDING), 16, keep=(self.opt_state,))
        t.after = [self.adam_embed] if self.defer_opt else [self.adam_full] + self.quant_all
        # The embedding table's update split by rows (vqa_adamw_rows): the rows no
        # token of the step touched have a zero gradient, so their update runs beside the
        # backward (mark the step's ids, then those rows), and the step's exposed tail keeps
        # only the rel-bias range and the touched rows.  Bit-identical to the dense range.
        self.embed_split = self.defer_opt
        T, emb = self.T, lay["t5.embed"]
        self.fused_tail = self.embed_split and T <= 16384          # one sort slice
        if self.embed_split:
            assert emb.offset + emb.numel == n
            if self.EMB_MARK is None:
                self.EMB_MARK = torch.full((S.T5_VOCAB,), -1, dtype=torch.int32, device=self.dev)
            lo = emb.offset
            self._emb_desc = dt = self._adam_range_desc(lo, n)       # the table's rows
            keep = self._adam_keep() + (self.EMB_MARK,)
            rows_call = lambda touched: ops.Call("vqa_adamw_rows", ctypes.byref(dt), self.EMB_MARK.data_ptr(),  # noqa: E731
                                                 S.T5_VOCAB, self.D, touched, int(self.warmup), int(self.total),
                                                 desc=dt, keep=keep)
            t.mark = self.embed_mark_call(self.IDS, T)
            # the untouched rows' pass as 256 workgroups striding over the rows: a 32k-block grid
            # beside the chain cost what it saved at the tail (A/B: 6.47-6.48 ms either way), 256
            # measured 6.44-6.47
            t.rows_rest = rows_call(256)
            t.relbias, t.rows_touched = self.adam_range_call(e0, lo), rows_call(1)
        # The graph / stream step's shorter tail (needs the row marks): the scatter's id sort can run
        # beside the T5 backward (it reads IDS alone and nothing else writes WS_EMB), and ONE launch
        # sums [a, rel-bias) and [rel-bias, n) and finalizes; of the table it loads the marked rows
        # only -- every other row is exactly zero (vqa_embedding_zero_rows): the dense partials.
        if self.fused_tail:
            if self.SQ_CNT is None:
                self.SQ_CNT = torch.zeros(L.SQNORM_FINAL_COUNTER_WORDS, dtype=torch.int32,
                                          device=self.dev)        # arrival counters, left at zero
            lead = emb.offset - e0
            assert lead >= 0 and lead % 4 == 0 and emb.numel == S.T5_VOCAB * self.D and self.D % 4 == 0
            t.sq_final = ops.Call("vqa_grad_sqnorm_final", ops.addr(G, a), e0 - a, ops.addr(G, e0), n - e0,
                                  self.WS_SQ.data_ptr(), K, 3 * K, self.EMB_MARK.data_ptr(), lead, self.D,
                                  self.SQ_CNT.data_ptr(), *self._optim_scalars(), self.opt_state.data_ptr(),
                                  keep=(G[a:], self.WS_SQ, self.EMB_MARK, self.SQ_CNT, self.opt_state))
            ids, ws = self.IDS.data_ptr(), self.WS_EMB.data_ptr()
            t.sort = ops.Call("vqa_embedding_sort", ids, T, S.T5_VOCAB, ws, keep=(self.IDS, self.WS_EMB))
            t.scatter = ops.Call("vqa_embedding_bwd_sorted", self.dH32.data_ptr(), self.g32["t5.embed"].data_ptr(), T,
                                 self.D, S.T5_VOCAB, ws, keep=(self.dH32, self.G32, self.WS_EMB))
        self.opt_calls, self.tail_calls_unfused, self.tail_calls = t.dense, t.split, t.short
        self.emb_pre = [t.mark, t.rows_rest] if self.embed_split else []
        self.emb_sort_call, self.emb_scatter_call = t.sort, t.scatter

    def _adam_groups(self):
        ends, lrs = self.lay.group_of_element()
        return ends, [self.group_lr.get(g, lr) for g, lr in zip(self.lay.groups, lrs)]

    def flush_optimizer(self):
        """Apply a deferred AdamW update now (before reading the parameters outside a step)."""
        if self.defer_opt:
            self._run([c for _, c in self.adam_segs] + [self.clear_pending])

    def set_grad_scale(self, s):
        """DP: grads are summed over ranks; the average enters as a scale."""
        self.grad_scale = float(s)
        self._replan_optimizer()

    # ------------------------------------------------------------------ execution
    def load_batch(self, batch, next_images=None):
        """Copy a batch dict (numpy or torch, host or device) into the static input buffers.
        Pipelined engines take the batch's text and targets, and `next_images` = the image
        tensors of the batch that the FOLLOWING step trains on (this batch's images went
        in one step earlier, or through prime())."""
        ae = self.allow_empty_rows
        n = batch_rows(batch, "question_input_ids", self.B, ae)
        items = []                                         # (buffer, source, load_rows arguments) of n rows
        if self.pipeline:
            # this batch's images went in one step earlier (or through prime()): their row count
            # must be the text's, else the rows past the shorter one would pair other samples'
            # features with real targets
            if self._img_rows_next is not None and self._img_rows_next != n:
                raise ValueError(f"pipelined engine: this batch has {n} question rows but its images "
                                 f"(loaded one step earlier) had {self._img_rows_next}")
            if next_images is not None:
                ni = batch_rows({"image_tensors": next_images}, "image_tensors", self.B, ae)
                if ni == n:
                    items.append((self.IMG, next_images, {}))
                else:
                    load_rows(self.IMG, next_images, ni)
                self._img_rows_next = ni
            else:
                self._img_rows_next = None
        else:
            items.append((self.IMG, batch["image_tensors"], {}))
        self.rows = n
        items += [(self.IDS, batch["question_input_ids"], {}),
                  (self.MASK, batch["question_attention_masks"], {"empty_fill": 1}),
                  (self.TGT, batch.get("annotation_ids"), {"fill": IGNORE_INDEX})]
        load_rows_multi(items, n)                          # full device batches: one launch for all four

    def prime(self, images):
        """Pipelined engines: compute the layer4 features of the first batch's images, so
        that the first train_step has them (later steps produce their successor's).
        Accumulating engines (use_accumulation): `images` are the first B rows of the first global
        batch; inside accum_step micro-batch j's next images are micro-batch j + 1's, and the last
        micro-batch takes the caller's `next_images` = the first B rows of the NEXT global batch."""
        assert self.pipeline, "prime() is for pipelined engines"
        ni = batch_rows({"image_tensors": images}, "image_tensors", self.B, self.allow_empty_rows)
        load_rows(self.IMG, images, ni)
        self._img_rows_next = ni
        self._run(self.res_calls)

    def use_global_rows(self, world):
        """Data parallel (dp.DataParallelStep): the head backward divides by the valid-row count
        summed over the `world` ranks (ROWTOT, which the DP step fills each step: count_call, then
        an all-reduce) over `world` instead of by the rank's own count, and rewrites LOSS as the
        rank's share (vqa_head_bwd, ABI 18), so the summed, 1/world-scaled gradients are the
        global batch's NLL mean however the global batch is split -- unequal rows per rank, or a
        rank with none (allowed from here on: its gradient is zero).  The reference's mean is
        over the whole batch (resnet_vqa_model.py:159, loaders without drop_last,
        trainer/faster_rcnn_vqa_trainer.py:172-197)."""
        i = next(k for k, c in enumerate(self.bwd_calls) if c.name == "vqa_head_bwd")
        old = self.bwd_calls[i]
        if self.count_call is not None:
            assert old.args[-1] == float(world), "use_global_rows: already set for another world size"
            return
        new = ops.Call("vqa_head_bwd", *old.args[:-2], ops.addr(self.ROWTOT), float(world),
                       keep=tuple(old.keep) + (self.ROWTOT,))
        new.side = old.side
        self.bwd_calls[i] = new
        self.count_call = ops.Call("vqa_count_targets", ops.addr(self.TGT), self.B, ops.addr(self.ROWTOT),
                                   keep=(self.TGT, self.ROWTOT))
        self.allow_empty_rows = True
        self.graph = None

    # ------------------------------------------------------------------ gradient accumulation
    def use_accumulation(self, k):
        """One optimizer step = k micro-batches of the planned B rows (accum_step): the global batch
        of up to k x B rows trains like one engine planned for k x B rows -- data parallelism laid
        out in time.  Call it before the first capture.  k = 1 does nothing at all.  For k > 1:
          * GACC (fp32, the arena's size) and LOGP_ALL [k B, A] are allocated, and 16 bytes of
            device state ACC = {double loss sum, int32 micro-batches done};
          * the head backward takes the global-rows form of use_global_rows(k): ROWTOT is the valid
            rows of the whole global batch, counted once per optimizer step from TGT_ALL (one
            vqa_count_targets launch, hence k x B <= 1024), so the k gradients summed and scaled by
            1/k are the global batch's NLL mean however its rows fall into micro-batches (an empty
            micro-batch gives a zero gradient and loss share 0);
          * the optimizer is re-planned over GACC with grad_scale / k (one plan: squared norms,
            finalize, every AdamW range and the row-split table update, flush_optimizer's ranges).
        The step is k replays of ONE micro-batch graph -- forward, backward without the tail,
        vqa_embed_mark of its ids, then on the main stream vqa_grad_accumulate(GACC, G32) and
        vqa_accum_advance; the device counter makes the first replay copy and the others add --
        and one finish graph: the untouched table rows' update, the squared norms of GACC, finalize,
        the rel-bias range and the touched rows, vqa_accum_finish; the other AdamW ranges stay
        deferred into the next step's first forward (they are no-ops in micro-batches 2..k:
        VQA_ST_PENDING is clear by then)."""
        k = int(k)
        if k < 1:
            raise ValueError(f"use_accumulation: k={k} must be >= 1")
        if self.accum != 1 or k == 1:
            if k != self.accum:
                raise ValueError(f"use_accumulation: already set for k={self.accum}")
            return
        if self.fp8:
            raise ValueError("use_accumulation: fp8 engines do not accumulate")
        if k * self.B > 1024:
            raise ValueError(f"use_accumulation: k x batch = {k * self.B} > 1024 rows (vqa_count_targets)")
        if self.allreduce is not None or self.count_call is not None or self.res_external:
            raise ValueError("use_accumulation: not together with data parallel or an external ResNet stream")
        with torch.cuda.device(self.dev):
            self.GACC = self._t(self.lay.total, zero=True)
            self.LOGP_ALL = self._t((k * self.B, self.A), zero=True)
            self.TGT_ALL = torch.full((k * self.B,), IGNORE_INDEX, dtype=I64, device=self.dev)
            self.ACC = self._t(4, torch.int32, zero=True)
        self.use_global_rows(k)
        self.count_call = ops.Call("vqa_count_targets", ops.addr(self.TGT_ALL), k * self.B, ops.addr(self.ROWTOT),
                                   keep=(self.TGT_ALL, self.ROWTOT))
        loss_sum, micro = ops.addr(self.ACC), ops.addr(self.ACC, 2)
        self.accum_calls = [
            ops.Call("vqa_grad_accumulate", ops.addr(self.GACC), ops.addr(self.G32), self.lay.total, micro,
                     keep=(self.GACC, self.G32, self.ACC)),
            ops.Call("vqa_accum_advance", ops.addr(self.LOGP), ops.addr(self.LOGP_ALL), self.B, self.A, k,
                     ops.addr(self.LOSS), loss_sum, micro, keep=(self.LOGP, self.LOGP_ALL, self.LOSS, self.ACC))]
        self.accum_finish = ops.Call("vqa_accum_finish", ops.addr(self.LOSS), loss_sum, micro, k,
                                     keep=(self.LOSS, self.ACC))
        self.accum = k
        self.set_grad_scale(self.grad_scale / k)          # re-plans over GACC (G_OPT), drops the graph

    def _finish_calls(self):
        """The finish graph of an accumulated step, the tail over GACC: the untouched table rows
        (before finalize; the marks are the union of the k micro-batches', all stamped with the one
        step counter), the squared-norm partials, finalize, the rel-bias range and the touched rows
        -- without defer_optimizer the whole AdamW pass -- then vqa_accum_finish."""
        t = self.tail
        rest = [t.rows_rest] if self.embed_split else []
        return rest + [t.sq_a, t.sq_b] + t.split + [self.accum_finish]

    def _micro_backward(self):
        """A micro-batch's backward: no tail.  The untouched-rows pass and the squared-norm overlap
        belong to the finish graph (here they would update rows early and sum G32); the ids are
        marked per micro-batch.  run_backward_streams ends with `side` and `wside` joined into the
        main stream, and the previous step's deferred AdamW ranges, which read GACC, were issued
        on the main stream by this micro-batch's forward: the accumulate, which overwrites GACC in
        micro-batch 0, follows all of them in stream order."""
        if self.embed_split:
            self._run([self.tail.mark])
        self.run_backward_streams()
        self._run(self.accum_calls)

    def accum_step(self, batch, next_images=None, use_graph=True, on_micro=None):
        """One optimizer step over a global batch of 1 .. k x B rows (use_accumulation(k), k > 1):
        the rows split contiguously (accum_spans), all k micro-batches run, then the finish graph.
        Afterwards LOSS is the global batch's mean NLL, LOGP_ALL[:rows] its log-probs and
        last_grad_norm() the norm of its gradient.  use_graph=False issues the same calls without
        capture.  on_micro(j) is called after micro-batch j has been issued (tests).
        Pipelined engines: micro-batch j's next images are micro-batch j + 1's rows of
        batch["image_tensors"]; the last micro-batch takes `next_images`, the FIRST B rows of the
        next global batch (prime() takes the first B rows of the first one)."""
        k, B = self.accum, self.B
        if k == 1:
            raise RuntimeError("accum_step: call use_accumulation(k) with k > 1 first")
        tgt = batch.get("annotation_ids")
        if tgt is None:
            raise ValueError("accum_step: the batch has no annotation_ids")
        n = int(torch.as_tensor(batch["question_input_ids"]).shape[0])
        spans = accum_spans(n, B, k)
        load_rows(self.TGT_ALL, tgt, n, fill=IGNORE_INDEX)
        self._run([self.count_call])                       # ROWTOT: the valid rows of all k x B
        for j, (lo, hi) in enumerate(spans):
            sub = {key: batch[key][lo:hi] for key in ("question_input_ids", "question_attention_masks",
                                                      "image_tensors", "annotation_ids") if batch.get(key) is not None}
            if self.pipeline:
                a, b = spans[j + 1] if j + 1 < k else (0, 0)
                self.load_batch(sub, next_images=batch["image_tensors"][a:b] if j + 1 < k else next_images)
            else:
                self.load_batch(sub)
            if use_graph and self.graph is None:
                self.capture()
            if not use_graph:
                self._step_pipelined() if self.pipeline else self._run_step_streams()
            else:
                if self.pipeline and self.res_order == "root":
                    self.copy_f4(L.stream_handle(torch.cuda.current_stream(self.dev)))
                self.graph[0].replay()
            if on_micro is not None:
                on_micro(j)
        if use_graph:
            self.graph[1].replay()
        else:
            self._run(self._finish_calls())
        self.accum_rows = n

    def forward(self):
        self.flush_optimizer()                          # the previous step's deferred update, then the forward
        super().forward()

    def _run_step_streams(self):
        """One step with graph-level concurrency: the frozen-ResNet + ConvTranspose2d
        branch and the T5 encoder run on two streams in the forward (they meet at
        SGA block 0), and the scaler weight gradient overlaps the T5 backward.
        Buffers of the two branches are disjoint, so the result is the same as
        the sequential order (and bit-identical: no cross-branch reductions)."""
        self.run_forward_streams()
        self._backward_and_tail()

    def _backward_and_tail(self):
        """The backward and optimizer tail of a full stream / graph step (an accumulating engine:
        the micro-batch's backward, accumulate and advance; the tail is the finish graph's)."""
        if self.accum > 1:
            self._micro_backward()
            return
        self.run_backward_streams(sq_overlap=True)
        self._run(self.tail_calls)

    def run_forward_streams(self):
        main = torch.cuda.current_stream(self.dev)
        side = self._side
        f = self.fwd_calls
        p0, p1, p2 = self._fsplit
        self._run(f[:p0])                                  # rng advance
        _after(side, main)
        vis, txt = f[p0:p1], f[p1:p2]
        if self.defer_opt:
            self._forward_branches_deferred(main, side, vis, txt)
        else:
            self._forward_branches(main, side, vis, txt)
        self._run(f[p2:])                                  # SGA + head

    def _forward_branches(self, main, side, vis, txt):
        """Issue the two branches interleaved (ResNet + ConvTranspose2d on `main`,
        T5 encoder on `side`, which already waits for the fork), then join: a replayed
        graph submits its nodes in capture order, so capturing one branch whole would
        hold the other back until all of its nodes were submitted (measured: the ResNet
        branch started ~1 ms into the step).  Shared by the training step without a
        deferred update and by the evaluation graph (_run_eval_streams)."""
        hm, hs = L.stream_handle(main), L.stream_handle(side)
        j = 0
        for i, c in enumerate(vis):
            c(hm)
            upto = (i + 1) * len(txt) // len(vis)
            while j < upto:
                txt[j](hs)
                j += 1
        for c in txt[j:]:
            c(hs)
        _after(main, side)

    def _t5_waits(self, i):
        """The deferred AdamW ranges T5 layer i's calls must find applied, beyond those of the
        layers before it: its own, and with fuse_norm also layer i+1's -- the layer's `wo` GEMM
        then carries the NEXT layer's ln0 and reads that gain, which lies in range t5.{i+1}
        (layout.py: a layer's range runs from its q|k|v weight to its ln1)."""
        w = [f"t5.{i}"]
        if self.fuse_norm and i + 1 < self.nl:
            w.append(f"t5.{i + 1}")
        return w

    def _forward_branches_deferred(self, main, side, vis, txt):
        """The two forward branches with the previous step's AdamW ranges on a third stream.
        Capture order is submission order for a replayed graph, so the ranges are issued
        two T5 layers ahead of the layer calls that wait for them (issuing all of them
        first held the T5 chain back ~0.47 ms; with fuse_norm a layer also waits for the next
        layer's range, _t5_waits); the vision branch's parameter-reading
        calls wait for the scaler range, the SGA / head for the last range."""
        hm, hs = L.stream_handle(main), L.stream_handle(side)
        # the ranges run on the vision-branch stream: a fourth concurrent stream shares a
        # hardware queue with one of the others anyway (measured 6.85 vs 6.81 ms)
        ost = main
        hs_o = L.stream_handle(ost)
        segs = dict(self.adam_segs)
        order = [n for n, _ in self.adam_segs]
        ev = {}

        def issue(name):
            segs[name](hs_o)
            ev[name] = torch.cuda.Event()
            ev[name].record(ost)
        p0, p1 = self._fsplit[0], self._fsplit[1]
        starts = [at - p1 for at in self._t5_layer_start]
        nl = len(starts)
        # ranges in issue order: layers 0, 1, the scaler, the SGA / head range (the vision
        # branch's SGA block-0 k/v projection reads it), then layer i+2 at layer i
        ahead = 2                                          # layers a range runs ahead of its use
        for i in range(min(ahead, nl)):
            issue(f"t5.{i}")
        issue("scaler")
        issue("head")
        vpre = vis[:self._fvis_param - p0]                 # frozen ResNet calls (unpipelined engines)
        vpost = vis[self._fvis_param - p0:]                # ConvTranspose2d + SGA block 0 k/v
        bounds = starts + [len(txt)]
        j = 0
        feed = self._res_feed                              # the next batch's ResNet (res_order interleave)
        nres = len(feed[0]) if feed else 0
        head = min(nres, self.res_head)

        def res_upto(n):
            while feed and feed[0] and nres - len(feed[0]) < n:
                feed[0].pop(0)(feed[1])
        res_upto(head)
        for t in range(bounds[0]):                         # embedding + rel-bias
            txt[t](hs)
        for i in range(nl):
            if i + ahead < nl:
                issue(f"t5.{i + ahead}")
            for name in self._t5_waits(i):                 # (fuse_norm: one layer of slack, not two)
                side.wait_event(ev[name])
            for t in range(bounds[i], bounds[i + 1]):
                txt[t](hs)
            res_upto(head + (i + 1) * (nres - head) // nl)
            # the ResNet calls spread over the layers (as in the plain interleave); the
            # parameter-reading vision calls follow the last of them (they read its output)
            while j < (i + 1) * len(vpre) // nl:
                vpre[j](hm)
                j += 1
            if j == len(vpre) and vpost:
                main.wait_event(ev["scaler"])
                main.wait_event(ev["head"])
                for c in vpost:
                    c(hm)
                vpost = []
        _after(main, side)
        main.wait_event(ev[f"t5.{nl - 1}"])               # the last range issued (stream order)
        self.clear_pending(hm)                             # the update is applied: once only
        assert set(ev) == set(order)

    def run_backward_streams(self, sq_overlap=False):
        """sq_overlap (a full step): also run the tail's early parts beside the backward, on `side`:
        the untouched embedding rows' update (emb_pre), the squared-norm partials of [0, a), final
        once the first T5 weight-gradient group is, and of [a, rel-bias), final before the embedding
        scatter; the caller then runs tail_calls.
        With fused_tail the embedding scatter's id sort also runs here on `side`, ahead of emb_pre
        and beside the T5 backward (it reads IDS alone), and the [a, rel-bias) partials are left to
        the caller's tail_calls (vqa_grad_sqnorm_final) -- the scatter is then the only launch
        issued behind the chain, beside the trailing weight-gradient GEMMs on `wside`."""
        t = self.tail
        fused = sq_overlap and self.fused_tail
        main = torch.cuda.current_stream(self.dev)
        side, wside = self._side, self._wside
        b = self.bwd_calls
        q0, q1 = self._bsplit
        self._run_tagged(b[:q0], main, wside)              # head + SGA backward
        _after(side, main)
        with torch.cuda.stream(side):
            self._run(b[q0:q1])                            # scaler dW / db
            if fused:
                t.sort(L.stream_handle(side))
                sorted_ev = torch.cuda.Event()
                sorted_ev.record(side)
            if sq_overlap:
                self._run(self.emb_pre)
        if sq_overlap:
            assert b[-1] is self.emb_call

            def to_side(calls):                            # after everything issued so far on main / wside
                for st in ((main, wside) if self.dw_stream else (main,)):
                    _after(side, st)
                with torch.cuda.stream(side):
                    self._run(calls)
            late = [] if fused else [t.sq_b]
            m1 = self._sq_split[0] if self._sq_split is not None else None
            if m1 is not None and q1 < m1 < len(b) - 1:
                self._run_tagged(b[q1:m1], main, wside)    # T5 backward up to the first dW group
                to_side([t.sq_a])                          # beside the rest
                self._run_tagged(b[m1:-1], main, wside)
            else:
                self._run_tagged(b[q1:-1], main, wside)    # T5 backward (+ deferred column sums)
                late = [t.sq_a] + late
            if fused:
                main.wait_event(sorted_ev)
                self._run([t.scatter])
            if late:
                to_side(late)
            if not fused:
                self._run(b[-1:])                          # embedding rows
        else:
            self._run_tagged(b[q1:], main, wside)          # T5 backward + embedding
        for st in (side, wside):
            _after(main, st)

    def _run_tagged(self, calls, main, wside):
        """Run `calls` in order on `main`, except runs of side-tagged calls (weight
        gradients), which go to `wside` after an event on `main` at that point
        (`dw_stream`, on by default): the batched T5 dW launches trail the input-gradient chain
        (6.66 vs 6.78-6.84 ms per step).  dp.DataParallelStep keeps this placement across its
        stage graphs (dp.plan_stages: a segment's side-tagged calls forked beside the next
        chain segment, its gradient bucket all-reduced once that stage has ended).  Every
        bf16 gradient a side-tagged call reads has its own buffer, so no later chain
        call overwrites it (tests: test_dw_stream_matches_single_stream_bitwise)."""
        if not self.dw_stream:
            self._run(calls)
            return
        i, n = 0, len(calls)
        while i < n:
            j = i
            while j < n and calls[j].side == calls[i].side:
                j += 1
            if calls[i].side:
                _after(wside, main)
                with torch.cuda.stream(wside):
                    self._run(calls[i:j])
            else:
                self._run(calls[i:j])
            i = j

    def set_res_cumask(self, words):
        """Experiment (bench.py --res-cumask): run the next batch's ResNet on a stream restricted
        to the CUs whose bits are set in `words` (hipExtStreamCreateWithCUMask, 32 CUs per word),
        launched eagerly beside the step graph, which then holds the chain only.  Call before
        capture().  Ordering as in the graph: F4 <- F4N, then the ResNet may overwrite F4N; the
        next step's inputs wait for it."""
        hip = L.hip_runtime()
        s = ctypes.c_void_p()
        arr = (ctypes.c_uint32 * len(words))(*words)
        with torch.cuda.device(self.dev):
            rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(s), ctypes.c_uint32(len(words)), arr)
        if rc != 0:
            raise RuntimeError(f"hipExtStreamCreateWithCUMask failed ({rc})")
        self.reset_res_cumask()                       # one masked stream at a time
        self._rstream_plain = self._rstream           # restored by reset_res_cumask
        self._rstream_handle = s
        self._rstream = torch.cuda.ExternalStream(s.value, device=self.dev)
        self.res_external = True

    def reset_res_cumask(self, destroy=True):
        """End the set_res_cumask experiment: the ResNet goes back to the engine's own stream and
        into the captured step (re-capture needed: the graph is dropped).  destroy=False keeps the
        masked stream alive and returns it (tools/queue_probe.py times the step while it exists);
        the caller then owns the handle (hipStreamDestroy)."""
        h = self._rstream_handle
        if h is None:
            return None
        torch.cuda.synchronize(self.dev)
        masked = self._rstream
        self._rstream = self._rstream_plain
        self._rstream_handle = None
        if self.res_external:
            self.res_external = False
            self.graph = None
        if destroy:
            rc = L.hip_runtime().hipStreamDestroy(h)
            if rc != 0:
                raise RuntimeError(f"hipStreamDestroy failed ({rc})")
            return None
        return masked, h

    def _res_external_step(self):
        main = torch.cuda.current_stream(self.dev)
        self.copy_f4(L.stream_handle(main))
        _after(self._rstream, main)                        # the ResNet waits for the copy, not for the chain
        for g in self.graph:
            g.replay()
        with torch.cuda.stream(self._rstream):
            self._run(self.res_calls)
        _after(main, self._rstream)

    def _step_pipelined(self):
        """One pipelined step: F4 <- F4N (features of this batch, made last step), then the
        ResNet of the next batch (IMG -> F4N) on its own stream, concurrently with this
        step's whole chain on the current stream; joined at the end.  The two sides share
        no buffer, so every result equals the unpipelined step's bit for bit."""
        main = torch.cuda.current_stream(self.dev)
        if self.res_external:                              # the chain only (set_res_cumask)
            self.run_forward_streams()
            self._backward_and_tail()
            return
        if not (torch.cuda.is_current_stream_capturing() and self.res_order == "root"):
            self.copy_f4(L.stream_handle(main))            # ("root": issued before the replay, train_step)
        _after(self._rstream, main)

        # the ResNet branch is captured first: a replayed graph submits nodes in capture order,
        # and issuing it after T5 layer 0 / 1 / 3 measured 0.7 ms slower
        # (res_order "last": the same dependencies, the ResNet's nodes created after the chain's)
        last = self.res_order == "last"
        inter = self.res_order == "interleave"
        if inter:                    # issued between the T5 encoder layers (_forward_branches_deferred)
            self._res_feed = [list(self.res_calls), L.stream_handle(self._rstream)]
        elif not last:
            with torch.cuda.stream(self._rstream):
                self._run(self.res_calls)
        self.run_forward_streams()                         # ConvTranspose2d || T5 encoder, then SGA
        if inter:
            assert not self._res_feed[0], "every ResNet call issued"
            self._res_feed = None
        self._backward_and_tail()
        if last:
            with torch.cuda.stream(self._rstream):
                self._run(self.res_calls)
        _after(main, self._rstream)

    def train_step(self):
        """zero_grad -> forward -> backward -> (all-reduce) -> clip -> AdamW -> sched, all on-device."""
        if self.accum > 1:
            raise RuntimeError("this engine accumulates micro-batches (use_accumulation): drive it with accum_step")
        if self.graph is not None and self.res_external:
            self._res_external_step()
            return
        if self.graph is not None and self.pipeline and self.res_order == "root":
            self.copy_f4(L.stream_handle(torch.cuda.current_stream(self.dev)))
        if self.graph is not None:
            for g in self.graph:
                if callable(g):
                    g()
                else:
                    g.replay()
            return
        if self.pipeline:
            assert self.allreduce is None, "pipelined DP steps go through dp.DataParallelStep"
            self._step_pipelined()
            return
        self.forward()
        self.backward()
        if self.allreduce is not None:
            self.allreduce(self.G32)
        self.optimizer_step()

    def capture(self, warm=True, keep_graph=False):
        """Capture the step as hipGraph(s): one graph when single-GPU; with a DP
        all-reduce hook, graph(fwd+bwd) -> eager collective -> graph(optimizer).
        keep_graph: keep the hipGraph_t of each part (torch CUDAGraph keep_graph) so tests can
        walk its nodes (raw_cuda_graph); the exec is instantiated here either way."""
        self._keep_graph = bool(keep_graph)
        self.flush_optimizer()           # the warm-up's backward must not overwrite a pending update's G
        s = torch.cuda.Stream(self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        saved, saved_rng = self.opt_state.clone(), self.RNG.clone()
        with torch.cuda.stream(s):
            if warm:                                    # warm-up launch outside capture (no update)
                self._run(self.fwd_calls)
                self.backward()
        torch.cuda.current_stream(self.dev).wait_stream(s)
        torch.cuda.synchronize(self.dev)
        with no_gc_capture():
            parts = self._capture_parts(s)
        self.opt_state.copy_(saved)
        self.RNG.copy_(saved_rng)                       # the warm-up launch must not consume a dropout draw
        for g in parts:
            if self._keep_graph and not callable(g):
                g.instantiate()
        self.graph = parts

    def _capture_parts(self, s):
        assert self.accum == 1 or (self.allreduce is None and not self.res_external)
        if self.allreduce is None:
            g = self._new_graph()
            with torch.cuda.graph(g, stream=s):
                if self.pipeline:
                    self._step_pipelined()
                else:
                    self._run_step_streams()
            parts = [g]
            if self.accum > 1:
                # graph(micro-batch) x k -> graph(finish): the device counter lets one micro-batch
                # graph serve every position.  Capture runs neither: GACC and ACC stay as they are
                # (the warm-up above is a forward and a backward, no accumulate, no advance)
                parts.append(self._new_graph())
                with torch.cuda.graph(parts[1], stream=s):
                    self._run(self._finish_calls())
        else:
            g1, g2 = self._new_graph(), self._new_graph()
            with torch.cuda.graph(g1, stream=s):
                self.forward()
                self.backward()
            with torch.cuda.graph(g2, stream=s):
                self.optimizer_step()
            ar = self.allreduce
            parts = [g1, lambda: ar(self.G32), g2]
        return parts

    # ------------------------------------------------------------------ evaluation graph
    # (eval_plan / eval_capture / eval_step / eval_result are EngineBase's; the two hooks are here)
    def _eval_setup(self, rollout):
        if self.pipeline:
            raise ValueError("pipelined engines take their images a step early; evaluation has no next batch: "
                             "build the engine with pipeline=False to evaluate")
        super()._eval_setup(rollout)

    def _eval_heat_setup(self, heatmap):
        if heatmap:
            self._plan_heat()

    def _run_eval_streams(self):
        """The evaluation step's calls: the forward without its rng advance -- the vision and
        text branches forked over the current stream and `_side`, interleaved as in the training
        step -- then SGA + head, then vqa_eval_rows."""
        main = torch.cuda.current_stream(self.dev)
        side = self._side
        f = self.fwd_calls
        p0, p1, p2 = self._fsplit
        _after(side, main)
        self._forward_branches(main, side, f[p0:p1], f[p1:p2])
        self._run(f[p2:])
        self.eval_call(L.stream_handle(main))
        if self.eval_heatmap:                              # F4 is final since the branches joined
            self.heat_call(L.stream_handle(main))

    # ------------------------------------------------------------------ readouts (tests / API)
    def _model_specs(self):
        return S.model_specs(self.vision, self.A, self.NB, self.dims)

    def _tune_calls(self):
        return (self.res_calls if self.pipeline else []) + super()._tune_calls()

    def log_probs(self):
        return self.LOGP[:self.rows]

    def loss(self):
        return self.LOSS

    def segment_grad(self, name, accumulated=False):
        """Segment `name`'s gradient view: of G32 (the last micro-batch's), or with `accumulated`
        of GACC (the global batch's sum, before the 1/k of the update)."""
        if not accumulated:
            return self.g32[name]
        if self.GACC is None:
            raise RuntimeError("segment_grad(accumulated=True): this engine does not accumulate (use_accumulation)")
        s = self.lay[name]
        return self.GACC[s.offset:s.offset + s.numel].view(s.shape)

    def accum_log_probs(self):
        """The log-probs of the last accum_step's global batch, [rows, A]."""
        return self.LOGP_ALL[:self.accum_rows]

    def refresh_shadow(self):
        super().refresh_shadow()
        self._run(self.quant_all)                       # ... and the e4m3 weight copies (fp8)

    def layer4_features(self):
        """The frozen ResNet's layer4 map of the current batch as NCHW fp32 (the kernels keep
        it NHWC bf16): the `features` generate_answers returns (resnet_vqa_model.py:186-203)."""
        return self.F4[:self.rows].permute(0, 3, 1, 2).float()

    def pool_features(self):
        """faster-rcnn: the FPN's 'pool' level of the current batch as NCHW fp32 [rows, 256, ph, ph]
        (the map the model's scaler reads; faster_rcnn_vqa_model.py:102-108)."""
        if self.vision != S.FASTER_RCNN:
            raise ValueError(f"pool_features: vision {self.vision!r} has no FPN (layer4_features is its map)")
        return self.F4[:self.rows].permute(0, 3, 1, 2).float()

    def fpn_maps(self):
        """faster-rcnn: the five FPN levels {'0','1','2','3','pool'} of the loaded images as NCHW
        fp32, the dict FasterRcnnVQAModel.generate_answers returns.  A second call list, planned
        on first use with buffers of its own (the body with C2..C4 kept, then the FPN; the top-down
        sum is the lateral GEMM's residual epilogue over vqa_upsample2x_nhwc's output) and run
        eagerly: the training and evaluation plans and their memory are as without it.  'pool' is
        made by the same two GEMMs as the step's vision map, on the same inputs."""
        if self.vision != S.FASTER_RCNN:
            raise ValueError(f"fpn_maps: vision {self.vision!r} has no FPN")
        if self.H % 32 != 0:
            raise ValueError(f"fpn_maps: image_size={self.H} is not a multiple of 32: the top-down path is planned "
                             "for exact 2x nearest upsamples")
        if self.pipeline:
            raise ValueError("fpn_maps: a pipelined engine holds the next batch's images; build it with pipeline=False")
        if self._fpn_plan is None:
            calls = []
            with torch.cuda.device(self.dev):
                maps = self._res_body(self._frozen, calls, pyramid=True)
            self._fpn_plan = (calls, maps)
        calls, maps = self._fpn_plan
        self._run(calls)
        return {k: maps[k][:self.rows].permute(0, 3, 1, 2).float() for k in ("0", "1", "2", "3", "pool")}

    # ------------------------------------------------------------------ heat map (CNN_vqa_heatmap.py:131-137)
    def _plan_heat(self):
        """HEAT / CAM [B, fh, fh] and the vqa_channel_cam call over the vision map F4."""
        if self.heat_call is None:
            with torch.cuda.device(self.dev):
                self.HEAT, self.CAM = self._t((self.B, self.fh, self.fh)), self._t((self.B, self.fh, self.fh))
                # arrival counters, left at zero by every launch
                self.HEAT_CNT = self._t(self.B * L.CAM_COUNTER_STRIDE, torch.int32, zero=True)
            lst = []
            self._call(lst, "vqa_channel_cam", self.F4, self.B, self.fh * self.fh, self.fc, self.CAM, self.HEAT,
                       self.HEAT_CNT)
            self.heat_call = lst[0]
        return self.heat_call

    def feature_heatmap(self, normalize=True):
        """The heat map of the current vision map (after a forward): per image the channel mean,
        min-max normalised (normalize=False: the channel mean itself), [rows, fh, fh] fp32."""
        self._run([self._plan_heat()])
        return (self.HEAT if normalize else self.CAM)[:self.rows].clone()
