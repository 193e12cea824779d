"""`VitVQAEngine` -- one training step of BASELINE config 4, the reference's
`VitVQAModel` (model/vit_vqa_model.py:127-227) trained by the ViT trainer
(trainer/vit_vqa_trainer.py:450-464: zero_grad -> forward -> backward ->
clip_grad_norm_ -> AdamW(amsgrad) -> sched), as a static schedule of the C-ABI
kernels over flat fp32 arenas, replayed as one hipGraph.

Forward (:166-225):
  * frozen ViT-base under no_grad (:183-186): patch im2col + GEMM (+ bias, + position
    embeddings as a broadcast residual) into rows 1..196 of each image, the CLS +
    position row scattered into row 0; 12 pre-LN layers (LayerNorm eps 1e-12,
    q|k|v GEMM with bias, the long-sequence MFMA attention, output GEMM + residual,
    LayerNorm, GELU GEMM, GEMM + residual); final LayerNorm and tanh pooler on the
    CLS rows only (the pooler reads nothing else);
  * T5 encoder: the ResNet path's plan (t5_stack.T5Stack); its CLS rows (encoder_outputs[:, 0, :], :189)
    and the pooled ViT output are the fusing layer's concat (:192-195);
  * fusing_layer: Linear(1536, 768) + ReLU + Dropout(0.5), one GEMM (:198);
  * T5 decoder (:199-205) over the ONE fused token: causal self-attention with the
    decoder's unidirectional relative bias (bucket -1 = finfo.min), cross-attention
    whose softmax over a single key is 1 (context = dropout(1) * v: vqa_xattn1_fwd;
    the 12 layers' value projections of the fused token are one GEMM), ReLU FF;
  * answer token = the last position with decoder mask 1 (:208-212), classifier +
    log_softmax + NLL (the head kernel with a length-1 pooler, whose softmax is 1).
Backward: the reverse schedule; the cross-attention q / k projections and the cross
layer norm get exactly zero gradients (softmax over one key is constant), computed as
such (the norm backward runs with dy = 0); the shared embedding table gets the encoder
and decoder token rows in one deterministic scatter.
Dropout: the counter-hash masks of the ResNet path (p = 0.1 at the T5 sites, 0.5 at
the fusing layer); the oracle (oracle/vit_oracle.py) restates the same sites.

This module holds the config-4 plan only: the frozen-ViT weights, the activations, the
forward / backward / optimizer schedules, batch loading, the single-stream step and its
capture.  The T5 encoder and decoder are two t5_stack.T5Stack, planned by the code that plans
the ResNet engine's encoder; the decoder's cross-attention sub-layer (_cross_forward /
_cross_backward) and the one-GEMM value projection stay here.  On purpose, not by omission, the
two stacks keep in-line weight gradients (_dx then _dw through shared scratch, ping-pong dH16)
and stand-alone norms: the ResNet engine's grouped weight gradients or fuse_norm would be a
performance change with measurements of its own.  The C ABI stays at 22.  Arenas, call
builders, the AdamW descriptor, the tuner entry and the state-dict / optimizer-state readouts, and the evaluation graph (eval_plan ... eval_result) are inherited from
engine_base.EngineBase; the evaluation step here is the forward without its rng advance on one
stream, optionally with the attention rollout of the frozen ViT (vqa_attn_headmean after every
layer's q|k|v projection, one vqa_rollout_cls: the reference's ViT_vqa_heatmap.py:104-137).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import lib as L
from . import ops
from . import synthetic as S
from . import vit_model as VM
from .engine_base import (BF16, F32, I64, IGNORE_INDEX, SITE_EMBED, SITE_FINAL, EngineBase, batch_rows, load_rows,
                          no_gc_capture, t5_site)
from .layout import t5_bucket_map
from .t5_stack import T5Grads, T5Stack

D = S.D_MODEL
NL, H5, DKV, DFF = S.T5_LAYERS, S.T5_HEADS, S.T5_DKV, S.T5_DFF
SITE_DEC_EMBED, SITE_DEC_FINAL, SITE_FUSE = 3, 4, 5


def dec_site(layer, kind):
    """kind 0 self probs, 1 self branch, 2 cross probs, 3 cross branch, 4 FF inner, 5 FF branch."""
    return 256 + 8 * layer + kind


class VitVQAEngine(EngineBase):
    TIED = {k: "lang_model.shared.weight" for k in VM.TIED}        # the encoder / decoder embed_tokens

    def __init__(self, state_dict, batch=64, seq_len=32, dec_len=VM.DEC_LEN, image_size=VM.VIT_IMAGE,
                 device="cuda:0", warmup=10, total=100, answer_spaces=170, max_norm=1.0, betas=(0.9, 0.999),
                 eps=1e-8, weight_decay=0.1, dropout=0.1, seed=0, group_lr=None):
        super().__init__(device, dropout, seed, warmup, total, max_norm, betas, eps, weight_decay, group_lr=group_lr)
        if not 1 <= answer_spaces <= 1024:
            raise ValueError(f"answer_spaces={answer_spaces}: the fused answer head supports 1..1024 answers")
        if not (1 <= seq_len <= 32 and 1 <= dec_len <= 32):
            raise ValueError("seq_len and dec_len must be in 1..32 (one 32-query MFMA attention tile)")
        if image_size % VM.VIT_PATCH:
            raise ValueError(f"image_size must be a multiple of {VM.VIT_PATCH}")
        self.B, self.L, self.Ld, self.H, self.D = batch, seq_len, dec_len, image_size, D
        self.T, self.TD = batch * seq_len, batch * dec_len
        self.rows = batch                 # real rows of the loaded batch (a short last batch is padded)
        self.NV = VM.vit_tokens(image_size)
        self.TV = batch * self.NV
        self.A = answer_spaces
        self.lay = VM.VitLayout(answer_spaces)
        sd = {k: np.asarray(v) for k, v in state_dict.items()}
        self._frozen = {k: v for k, v in sd.items() if k.startswith("vision_model.")}
        with torch.cuda.device(self.dev):
            self._alloc_params(sd)
            self._alloc_vit(sd)
            self._alloc_activations()
            self.fwd_calls, self.bwd_calls, self.opt_calls = [], [], []
            self._plan_forward()
            self._plan_backward()
            self._plan_optimizer()

    def _model_specs(self):
        return VM.model_specs(self.A, self.H)

    def _adam_groups(self):
        return self.lay.group_of_element(self.group_lr)

    # ------------------------------------------------------------------ allocation
    def _alloc_params(self, sd):
        self._alloc_arenas(sd)
        self.bucket_e = torch.from_numpy(t5_bucket_map(self.L, self.L)).reshape(-1).to(self.dev)
        self.bucket_d = torch.from_numpy(VM.causal_bucket_map(self.Ld)).reshape(-1).to(self.dev)

    def _alloc_vit(self, sd):
        """Frozen ViT weights: bf16 GEMM operands, fp32 biases / norms (not in the arena)."""
        dev = self.dev
        f32 = lambda k: torch.from_numpy(np.ascontiguousarray(sd["vision_model." + k], np.float32)).to(dev)
        b16 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).to(BF16)
        e = "embeddings."
        self.vw = {"patch_w": b16(sd["vision_model." + e + "patch_embeddings.projection.weight"].reshape(D, -1)),
                   "patch_b": f32(e + "patch_embeddings.projection.bias")}
        cls = np.asarray(sd["vision_model." + e + "cls_token"], np.float32).reshape(D)
        pos = np.asarray(sd["vision_model." + e + "position_embeddings"], np.float32).reshape(self.NV, D)
        self.vw["clspos"] = torch.from_numpy((cls + pos[0]).astype(np.float32)).to(dev)   # torch adds in fp32
        self.vw["pos"] = torch.from_numpy(np.ascontiguousarray(pos[1:])).to(dev)
        for i in range(VM.VIT_LAYERS):
            p = f"encoder.layer.{i}."
            a = p + "attention.attention."
            self.vw[f"{i}.qkv_w"] = b16(np.concatenate([sd["vision_model." + a + n + ".weight"]
                                                        for n in ("query", "key", "value")]))
            self.vw[f"{i}.qkv_b"] = torch.cat([f32(a + n + ".bias") for n in ("query", "key", "value")])
            self.vw[f"{i}.o_w"] = b16(sd["vision_model." + p + "attention.output.dense.weight"])
            self.vw[f"{i}.o_b"] = f32(p + "attention.output.dense.bias")
            self.vw[f"{i}.fc1_w"] = b16(sd["vision_model." + p + "intermediate.dense.weight"])
            self.vw[f"{i}.fc1_b"] = f32(p + "intermediate.dense.bias")
            self.vw[f"{i}.fc2_w"] = b16(sd["vision_model." + p + "output.dense.weight"])
            self.vw[f"{i}.fc2_b"] = f32(p + "output.dense.bias")
            for n, k in (("ln1", "layernorm_before"), ("ln2", "layernorm_after")):
                self.vw[f"{i}.{n}_g"], self.vw[f"{i}.{n}_b"] = f32(p + k + ".weight"), f32(p + k + ".bias")
        self.vw["lnf_g"], self.vw["lnf_b"] = f32("layernorm.weight"), f32("layernorm.bias")
        self.vw["pool_w"] = b16(sd["vision_model.pooler.dense.weight"])
        self.vw["pool_b"] = f32("pooler.dense.bias")

    def _alloc_activations(self):
        B, Lq, Ld, T, TD, TV = self.B, self.L, self.Ld, self.T, self.TD, self.TV
        t = self._t
        self.PIX = t((B, 3, self.H, self.H), zero=True)
        self.IDS_ALL = t(T + TD, I64, zero=True)                   # encoder then decoder token ids
        self.IDS_PREV = t(T + TD, I64, zero=True)
        self.IDS, self.DIDS = self.IDS_ALL[:T].view(B, Lq), self.IDS_ALL[T:].view(B, Ld)
        self.MASK, self.DMASK = t((B, Lq), I64, zero=True), t((B, Ld), I64, zero=True)
        self.TGT = t((B,), I64, zero=True)
        # ViT
        self.XP16 = t((B * (self.NV - 1), D), BF16)
        self.VH32, self.VLN16 = t((TV, D)), t((TV, D), BF16)
        self.VMU, self.VRS = t(TV), t(TV)
        self.VQKV16, self.VO16, self.VFF16 = t((TV, 3 * D), BF16), t((TV, D), BF16), t((TV, VM.VIT_FF), BF16)
        self.VCLS32, self.VCLSN16, self.VCMU, self.VCRS = t((B, D)), t((B, D), BF16), t(B), t(B)
        self.CAT16, self.FUSED16 = t((B, 2 * D), BF16), t((B, D), BF16)
        self.VALL16 = t((B, NL * D), BF16)
        # T5 encoder and decoder (t5_stack.T5Stack: per-layer activations)
        self.enc = T5Stack(self, "enc.", T, Lq, NL, H5, DKV, DFF, D, self.IDS, self.MASK, self.bucket_e, t5_site,
                           (2, 3), SITE_EMBED, SITE_FINAL)
        self.dec = T5Stack(self, "dec.", TD, Ld, NL, H5, DKV, DFF, D, self.DIDS, self.DMASK, self.bucket_d, dec_site,
                           (4, 5), SITE_DEC_EMBED, SITE_DEC_FINAL, ff_norm="ln2", decoder=True)
        self.TXT32, self.TXT16, self.DEC32 = self.enc.OUT32, self.enc.OUT16, self.dec.OUT32
        # read by tools/vit_trained_diag.py
        self.HS_d, self.HM_d, self.HX_d, self.O_d = self.dec.HS, self.dec.HM, self.dec.HX, self.dec.O
        # answer gather + head (the pooler of the head kernel over a length-1 sequence: identity)
        self.LASTIDX, self.ANS32 = t(B, I64, zero=True), t((B, D))
        self.DUMMY_PW, self.DUMMY_PB = t(D, zero=True), t(1, zero=True)
        self.DUMMY_GPW, self.DUMMY_GPB = t(D, zero=True), t(1, zero=True)
        self.ATT, self.POOLED = t((B, 1)), t((B, D))
        self.LOGP, self.NLL, self.LOSS = t((B, self.A)), t(B), t(1)
        # backward
        mx = max(T, TD)
        self.dH32_ALL = t((T + TD, D), zero=True)                  # embedding-row gradients, enc then dec
        self.dH32_e, self.dH32_d = self.dH32_ALL[:T], self.dH32_ALL[T:]
        self.dANS32, self.dDEC32, self.dTXT32 = t((B, D)), t((TD, D), zero=True), t((T, D), zero=True)
        self.dC32, self.dR32, self.dX32 = t((mx, D)), t((mx, D)), t((mx, D))
        self.ZERO32 = t((TD, D), zero=True)
        self.dH16 = [t((mx, D), BF16), t((mx, D), BF16)]
        self.dB16, self.dF16, self.dO16 = t((mx, D), BF16), t((mx, DFF), BF16), t((mx, D), BF16)
        self.dQKV16 = t((mx, 3 * D), BF16)
        self.dVALL16, self.dPRE16, self.dCLS32 = t((B, NL * D), BF16), t((B, D), BF16), t((B, D))
        lib = L.load()
        self.WS_EMB = t(3 * min(T + TD, 16384), torch.int32)
        self.WS_HEAD = t(lib.vqa_head_workspace_floats(B, 1, D, self.A))
        self.SQ_PARTS = 1024
        self.WS_SQ = t(self.SQ_PARTS, torch.float64)

    # ------------------------------------------------------------------ forward
    def _plan_forward(self):
        f = self.fwd_calls
        self._vit_attn_at, self.ATT_MAPS, self._probs_calls, self._roll_calls = [], None, None, None
        B, Lq, Ld, TV, NV = self.B, self.L, self.Ld, self.TV, self.NV
        vw = self.vw
        if self.p_drop > 0.0:
            self._call(f, "vqa_rng_advance", self.RNG)
        # ---- frozen ViT (ViTEmbeddings + 12 ViTLayer + layernorm + pooler)
        self._call(f, "vqa_vit_patchify", self.PIX, self.XP16, B, self.H, self.H, VM.VIT_PATCH)
        npch = NV - 1
        self._gemm(f, self.XP16, vw["patch_w"], npch, D, D, lda=D, ldb=D, c32=ops.addr(self.VH32, D), ldc32=D,
                   bias=vw["patch_b"], res32=vw["pos"], ldres=D, batch=B, stride_a=npch * D, stride_b=0,
                   stride_c32=NV * D, stride_res=0, keep=(self.VH32,))
        self._call(f, "vqa_scatter_rows", vw["clspos"], 0, None, NV, 0, self.VH32, D, B, D, 4)
        for i in range(VM.VIT_LAYERS):
            self._call(f, "vqa_layernorm_fwd", self.VH32, vw[f"{i}.ln1_g"], vw[f"{i}.ln1_b"], None, self.VLN16,
                       self.VMU, self.VRS, TV, D, VM.VIT_EPS)
            self._gemm(f, self.VLN16, vw[f"{i}.qkv_w"], TV, 3 * D, D, lda=D, ldb=D, c16=self.VQKV16, ldc16=3 * D,
                       bias=vw[f"{i}.qkv_b"])
            q = self.VQKV16
            self._attn(f, "vqa_attn_fwd", q=q, ldq=3 * D, k=ops.addr(q, D), ldk=3 * D, v=ops.addr(q, 2 * D),
                       ldv=3 * D, o=self.VO16, ldo=D, batch=B, heads=VM.VIT_HEADS, lq=NV, lk=NV, dh=VM.VIT_DH,
                       scale=VM.VIT_DH ** -0.5, keep=(q,))
            self._vit_attn_at.append(len(f))               # where forward_with_attentions reads layer i's P
            self._gemm(f, self.VO16, vw[f"{i}.o_w"], TV, D, D, lda=D, ldb=D, c32=self.VH32, ldc32=D,
                       bias=vw[f"{i}.o_b"], res32=self.VH32, ldres=D)
            self._call(f, "vqa_layernorm_fwd", self.VH32, vw[f"{i}.ln2_g"], vw[f"{i}.ln2_b"], None, self.VLN16,
                       self.VMU, self.VRS, TV, D, VM.VIT_EPS)
            self._gemm(f, self.VLN16, vw[f"{i}.fc1_w"], TV, VM.VIT_FF, D, lda=D, ldb=D, c16=self.VFF16,
                       ldc16=VM.VIT_FF, bias=vw[f"{i}.fc1_b"], relu=2)
            self._gemm(f, self.VFF16, vw[f"{i}.fc2_w"], TV, D, VM.VIT_FF, lda=VM.VIT_FF, ldb=VM.VIT_FF,
                       c32=self.VH32, ldc32=D, bias=vw[f"{i}.fc2_b"], res32=self.VH32, ldres=D)
        # the pooler reads only the CLS rows: final LayerNorm of those rows, then dense + tanh
        self._call(f, "vqa_gather_rows", self.VH32, D, None, NV, 0, self.VCLS32, D, B, D, 4)
        self._call(f, "vqa_layernorm_fwd", self.VCLS32, vw["lnf_g"], vw["lnf_b"], None, self.VCLSN16, self.VCMU,
                   self.VCRS, B, D, VM.VIT_EPS)
        self._gemm(f, self.VCLSN16, vw["pool_w"], B, D, D, lda=D, ldb=D, c16=self.CAT16, ldc16=2 * D,
                   bias=vw["pool_b"], relu=3)
        self.vit_calls = len(f)
        # ---- T5 encoder (the ResNet path's plan: t5_stack.T5Stack)
        self.enc.plan_forward(self, f)
        # encoder_outputs[:, 0, :] -> right half of the fusing layer's input
        self._call(f, "vqa_gather_rows", self.TXT16, D, None, Lq, 0, ops.addr(self.CAT16, D), 2 * D, B, D, 2,
                   extra=[self.CAT16])
        # fusing_layer: dropout(0.5)(relu(W [pooled | cls] + b))
        self._gemm(f, self.CAT16, self.p16["fuse_w"], B, D, 2 * D, lda=2 * D, ldb=2 * D, c16=self.FUSED16, ldc16=D,
                   bias=self.p32["fuse_b"], relu=True)
        if self.p_drop > 0.0:
            f[-1].desc.drop = L.Dropout(VM.FUSE_P, SITE_FUSE, self.RNG.data_ptr())
            f[-1].keep = f[-1].keep + (self.RNG,)
        # the 12 decoder layers' cross-attention values of the single fused token: one GEMM
        self._gemm(f, self.FUSED16, self.p16["dec.xv_w"], B, NL * D, D, lda=D, ldb=D, c16=self.VALL16,
                   ldc16=NL * D)
        # ---- T5 decoder
        self.dec.plan_forward(self, f, cross=self._cross_forward)
        # the answer token (last position of the decoder mask), classifier, log_softmax, NLL
        self._call(f, "vqa_last_index", self.DMASK, B, Ld, self.LASTIDX)
        self._call(f, "vqa_gather_rows", self.DEC32, D, self.LASTIDX, 0, 0, self.ANS32, D, B, D, 4)
        self._call(f, "vqa_head_fwd", self.ANS32, self.DUMMY_PW, self.DUMMY_PB, self.p32["cls_w"], self.p32["cls_b"],
                   self.TGT, self.ATT, self.POOLED, self.LOGP, self.NLL, self.LOSS, B, 1, D, self.A)

    def _cross_forward(self, f, st, i):
        """The decoder's cross sub-layer (T5Stack.plan_forward's `cross`): hx = hm + drop(xo(ctx)),
        ctx = drop(1) * v, v = layer i's columns of the one value projection VALL16."""
        kp = []
        self._call(f, "vqa_xattn1_fwd", ops.addr(self.VALL16, i * D), NL * D, st.CTX[i], D, self.B, self.Ld, H5, DKV,
                   self._dptr(dec_site(i, 2), kp), extra=kp + [self.VALL16, self.RNG])
        self._linear(f, st.CTX[i], f"dec.{i}.xo_w", self.TD, out32=st.HX[i], bias=False, res32=st.HM[i],
                     drop=dec_site(i, 3))

    # ------------------------------------------------------------------ backward
    def _plan_backward(self):
        b = self.bwd_calls
        B, Lq, T, TD = self.B, self.L, self.T, self.TD
        z = self.g32["embed"]
        self._call(b, "vqa_embedding_zero_rows", self.IDS_PREV, self.IDS_ALL, T + TD, z, D, S.T5_VOCAB)
        self._call(b, "vqa_head_bwd", self.ANS32, self.ATT, self.POOLED, self.LOGP, self.TGT, self.DUMMY_PW,
                   self.p32["cls_w"], self.dANS32, None, self.DUMMY_GPW, self.DUMMY_GPB, self.g32["cls_w"],
                   self.g32["cls_b"], self.WS_HEAD, B, 1, D, self.A, None, None, None, 1.0)
        # the answer rows move with the batch's decoder masks: clear last step's rows first
        self._call(b, "vqa_zero", self.dDEC32, TD * D * 4)
        self._call(b, "vqa_scatter_rows", self.dANS32, D, self.LASTIDX, 0, 0, self.dDEC32, D, B, D, 4)
        # ---- decoder (reverse): dH32 = gradient of the residual stream, dH16 the FF-branch gradient
        self.dec.plan_backward(self, b, self._t5_grads(TD, self.dDEC32, self.dH32_d), self._dxdw,
                               cross=self._cross_backward)
        # ---- the fused token: all layers' value projections, then the fusing layer
        ksf = (1.0 / (1.0 - VM.FUSE_P)) if self.p_drop > 0.0 else 1.0
        self._gemm(b, self.dVALL16, self.p16["dec.xv_w"], B, D, NL * D, lda=NL * D, ldb=D, b_trans=True,
                   c16=self.dPRE16, ldc16=D, mask16=self.FUSED16, ldmask=D, alpha=ksf)
        self._gemm(b, self.dVALL16, self.FUSED16, NL * D, D, B, lda=NL * D, ldb=D, a_trans=True, b_trans=True,
                   c32=self.g32["dec.xv_w"], ldc32=D)
        self._gemm(b, self.dPRE16, ops.addr(self.p16["fuse_w"], D), B, D, D, lda=D, ldb=2 * D, b_trans=True,
                   c32=self.dCLS32, ldc32=D, keep=(self.P16,))
        self._dw(b, self.dPRE16, self.CAT16, "fuse_w", B, bias_from=self.dPRE16)
        # ---- encoder: the CLS rows' gradient, final norm, layers
        self._call(b, "vqa_scatter_rows", self.dCLS32, D, None, Lq, 0, self.dTXT32, D, B, D, 4)
        self.enc.plan_backward(self, b, self._t5_grads(T, self.dTXT32, self.dH32_e), self._dxdw)
        self._flush(b)
        self._call(b, "vqa_embedding_bwd", self.IDS_ALL, self.dH32_ALL, self.g32["embed"], T + TD, D, S.T5_VOCAB,
                   self.WS_EMB)

    def _t5_grads(self, rows, dout, dh32):
        """T5Grads of a stack of `rows` rows: both stacks run their backward through the one shared
        scratch (the layers are serial and their weight gradients in line), the FF-branch gradient
        ping-pongs between the two dH16."""
        per_layer = lambda buf: [buf[:rows]] * NL                 # noqa: E731
        return T5Grads([self.dH16[(NL - 1 - i) & 1][:rows] for i in range(NL)], per_layer(self.dF16),
                       per_layer(self.dB16), per_layer(self.dQKV16), dout, dh32, self.dR32[:rows], self.dC32[:rows],
                       self.dO16[:rows], self.dX32[:rows])

    def _cross_backward(self, b, st, i, g):
        """The decoder's cross sub-layer (T5Stack.plan_backward's `cross`): xo, the value columns'
        gradient; q, k and the cross norm get exactly zero gradients, so its backward runs with
        dy = 0 and only carries the residual gradient and the self-attention branch's dropout."""
        self._dxdw(b, g.dHM[i], st.CTX[i], f"dec.{i}.xo_w", self.TD, out16=g.dO16)
        kp = []
        self._call(b, "vqa_xattn1_bwd", g.dO16, D, None, ops.addr(self.dVALL16, i * D), NL * D, self.B, self.Ld, H5,
                   DKV, self._dptr(dec_site(i, 2), kp), extra=kp + [self.dVALL16, self.RNG])
        st.norm_bwd(self, b, self.ZERO32, st.HM[i], st.R0[i], f"dec.{i}.ln1", g.dHX32, g.dHM32, g.dHM[i],
                    (None, None, dec_site(i, 1)))

    # ------------------------------------------------------------------ optimizer
    def _plan_optimizer(self):
        o = self.opt_calls
        n = self.lay.total
        self._call(o, "vqa_grad_sqnorm", self.G32, n, self.WS_SQ, self.SQ_PARTS)
        o.append(self._finalize_call(self.WS_SQ, self.SQ_PARTS))
        self._adam_desc = self._adam_desc_full()
        # AdamW at the end of the step (a no-op unless the finalize flagged a pending update).
        # Deferring it into the next step beside the frozen ViT, which reads no trained
        # parameter, measured slower (15.1-15.4 vs 14.2 ms per step: HBM / CU contention)
        o.append(self._adam_call(self._adam_desc))
        self._call(o, "vqa_zero", ops.addr(self.opt_state, L.ST_PENDING), 16, extra=[self.opt_state])

    # ------------------------------------------------------------------ execution
    def load_batch(self, batch):
        """The ViT collate's batch dict (pixel_values, question / decoder ids and masks,
        annotation_ids), numpy or torch, host or device."""
        n = self.rows = batch_rows(batch, "question_input_ids", self.B)
        load_rows(self.PIX, batch["pixel_values"], n)
        load_rows(self.IDS, batch["question_input_ids"], n)
        load_rows(self.MASK, batch["question_attention_masks"], n)
        load_rows(self.DIDS, batch["decoder_question_input_ids"], n)
        load_rows(self.DMASK, batch["decoder_question_attention_masks"], n)
        load_rows(self.TGT, batch.get("annotation_ids"), n, fill=IGNORE_INDEX)

    def forward_with_attentions(self):
        """forward() that also writes the frozen ViT's attention probabilities, HF
        ViTModel(output_attentions=True) (vit_vqa_model.py:238-240): a tuple of 12
        [B, 12, NV, NV] fp32 tensors (vqa_attn_probs after each layer's q|k|v projection; the
        buffer is allocated on the first call).  Eval readout for generate_answers."""
        B, NV = self.B, self.NV
        if self.ATT_MAPS is None:
            self.ATT_MAPS = torch.empty((VM.VIT_LAYERS, B, VM.VIT_HEADS, NV, NV), dtype=F32, device=self.dev)
            q = self.VQKV16
            self._probs_calls = []
            for i in range(VM.VIT_LAYERS):
                d = L.AttnDesc()
                d.q, d.ldq, d.k, d.ldk = ops.addr(q), 3 * D, ops.addr(q, D), 3 * D
                d.p = ops.addr(self.ATT_MAPS[i])
                d.batch, d.heads, d.lq, d.lk, d.dh, d.scale = B, VM.VIT_HEADS, NV, NV, VM.VIT_DH, VM.VIT_DH ** -0.5
                self._probs_calls.append(ops.Call("vqa_attn_probs", ctypes.byref(d), desc=d, keep=(q, self.ATT_MAPS)))
        s = L.stream_handle()
        at = {k: i for i, k in enumerate(self._vit_attn_at)}
        for idx, c in enumerate(self.fwd_calls):
            c(s)
            if idx + 1 in at:
                self._probs_calls[at[idx + 1]](s)
        return tuple(self.ATT_MAPS[i] for i in range(VM.VIT_LAYERS))

    # ------------------------------------------------------------------ attention rollout
    # The heat map of the reference's ViT script (ViT_vqa_heatmap.py:104-137) from each layer's
    # q | k, without the [12, B, 12, NV, NV] maps: vqa_attn_headmean after every layer's q|k|v
    # projection writes (mean over heads + I) / rowsum into ROLL_A[i] ([B, NV, ld] fp32, ld = NV
    # rounded up to 4), one vqa_rollout_cls after the forward chains row 0 through the layers.
    def _rollout_plan(self):
        """The rollout's prepared calls (12 head-mean calls, the chain); buffers on first use."""
        if self._roll_calls is None:
            B, NV = self.B, self.NV
            if NV > 256:
                raise ValueError(f"attention rollout: {NV} tokens; vqa_attn_headmean supports up to 256 "
                                 f"(image_size <= {15 * VM.VIT_PATCH})")
            ld = (NV + 3) // 4 * 4
            with torch.cuda.device(self.dev):
                self.ROLL_A = self._t((VM.VIT_LAYERS, B, NV, ld))
                self.ROLL_MASK, self.ROLL_UNIT = self._t((B, NV - 1)), self._t((B, NV - 1))
            q = self.VQKV16
            hm = []
            for i in range(VM.VIT_LAYERS):
                d = L.AttnDesc()
                d.q, d.ldq, d.k, d.ldk = ops.addr(q), 3 * D, ops.addr(q, D), 3 * D
                d.batch, d.heads, d.lq, d.lk, d.dh, d.scale = B, VM.VIT_HEADS, NV, NV, VM.VIT_DH, VM.VIT_DH ** -0.5
                hm.append(ops.Call("vqa_attn_headmean", ctypes.byref(d), ops.addr(self.ROLL_A[i]), ld, desc=d,
                                   keep=(q, self.ROLL_A)))
            chain = ops.Call("vqa_rollout_cls", ops.addr(self.ROLL_A), VM.VIT_LAYERS, B, NV, ld, B * NV * ld,
                             ops.addr(self.ROLL_MASK), ops.addr(self.ROLL_UNIT),
                             keep=(self.ROLL_A, self.ROLL_MASK, self.ROLL_UNIT))
            self._roll_calls = (hm, chain)
        return self._roll_calls

    def _forward_rollout(self, start=0):
        """fwd_calls[start:] with layer i's head-mean call behind its attention, then the chain."""
        hm, chain = self._rollout_plan()
        s = L.stream_handle()
        at = {k: i for i, k in enumerate(self._vit_attn_at)}
        for idx in range(start, len(self.fwd_calls)):
            self.fwd_calls[idx](s)
            if idx + 1 in at:
                hm[at[idx + 1]](s)
        chain(s)

    def attention_rollout(self):
        """forward() that also computes the attention rollout of the loaded images: (mask,
        mask_unit), each [rows, NV - 1] fp32 -- row 0 of the chained maps without the CLS column,
        and the same divided by its maximum (the script's mask / mask.max()).  The views are
        overwritten by the next rollout."""
        self._forward_rollout()
        return self.ROLL_MASK[:self.rows], self.ROLL_UNIT[:self.rows]

    # ------------------------------------------------------------------ evaluation (EngineBase's hooks)
    def _eval_setup(self, rollout):
        if rollout:
            self._rollout_plan()

    def _run_eval_streams(self):
        """The evaluation step on one stream: the forward without its leading vqa_rng_advance
        (an evaluation does not move the dropout counter), with the rollout's calls when the plan
        carries them, then vqa_eval_rows."""
        start = 1 if self.p_drop > 0.0 else 0
        if self.eval_rollout:
            self._forward_rollout(start)
        else:
            self._run(self.fwd_calls[start:])
        self.eval_call(L.stream_handle())

    def train_step(self):
        if self.graph is not None:
            self.graph.replay()
            return
        self.forward()
        self.backward()
        self.optimizer_step()

    def capture(self, warm=True):
        s = torch.cuda.Stream(self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        saved, saved_rng = self.opt_state.clone(), self.RNG.clone()
        with torch.cuda.stream(s):
            if warm:
                self._run(self.fwd_calls)
                self.backward()
        torch.cuda.current_stream(self.dev).wait_stream(s)
        torch.cuda.synchronize(self.dev)
        with no_gc_capture():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                self._run(self.fwd_calls)
                self.backward()
                self.optimizer_step()
        self.opt_state.copy_(saved)
        self.RNG.copy_(saved_rng)
        self.graph = g

    # ------------------------------------------------------------------ readouts
    def vit_pooled(self):
        """pooler_output of the frozen ViT for the current batch ([rows, 768], from its bf16 copy)."""
        return self.CAT16[:self.rows, :D].float()
