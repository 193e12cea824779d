"""T5Stack: one description and one plan of a T5 layer stack (TF/models/t5/modeling_t5.py:
640-751), shared by the ResNet model's encoder (engine.VQAEngine) and the ViT model's encoder
and decoder (vit_engine.VitVQAEngine).

A stack holds what the three differ in -- parameter names, row count and sequence length,
inputs, dropout sites -- and the forward activations, which it allocates itself.  Its two
methods append to an engine's call list through the engine's builders (engine_base.EngineBase):
  forward   embedding lookup, rel-bias, per layer  rmsnorm -> q|k|v GEMM -> attention (rel-bias,
            key mask, probability dropout) -> o GEMM + residual + dropout -> [cross] -> rmsnorm
            -> wi GEMM + ReLU + dropout -> wo GEMM + residual + dropout,  final rmsnorm + dropout;
  backward  the forward mirrored, vqa_rmsnorm_bwd carrying the residual gradient and the dropout
            of the layer below, down to the rel-bias gradient.
Where the gradients land (T5Grads), how a layer's dX / dW are issued (`dxdw`), what happens
between layers (`after_layer`) and a decoder's cross-attention sub-layer (`cross`) are the
engine's.
"""
from __future__ import annotations

from collections import namedtuple

from . import lib as L
from . import ops
from . import synthetic as S
from .engine_base import BF16

# Where a stack's backward writes.  Per layer (lists of nl): dH16 the FF-branch gradient a layer
# starts from, dF the wi output's, dHM the attention branch's, dQKV the q|k|v's (bf16: the GEMM
# operands).  Running (fp32 unless named 16): dOUT the gradient of the stack's output (read), dH32
# the residual stream's (at the end: the embedding rows'), dHM32 the stream's between attention
# and FF, dC32 and dO16 scratch; a decoder's dHX32 the stream's between cross-attention and FF.
T5Grads = namedtuple("T5Grads", "dH16 dF dHM dQKV dOUT dH32 dHM32 dC32 dO16 dHX32", defaults=(None,))


class T5Stack:
    def __init__(self, eng, prefix, rows, seq, nl, heads, dkv, dff, D, ids, mask, bucket, site, ff_kinds, embed_site,
                 final_site, embed="embed", ff_norm="ln1", decoder=False, stacked=False):
        """prefix: of the parameter names ("t5." / "enc." / "dec."); embed: the table's segment;
        ff_norm: the FF norm's name (a decoder's ln1 is its cross-attention's, its FF norm ln2;
        N1 / R1 are the FF norm's output and statistics either way).  site(layer, kind): dropout
        site of kind 0 attention probabilities, 1 attention branch, ff_kinds = (FF inner, FF
        branch); a decoder's kinds 2 / 3 are its cross-attention's probabilities / branch.
        stacked: N0 / O / N1 / FF as [nl, rows, *] tensors N0S / OS / N1S / FFS with layer i at slot
        nl-1-i (backward order), so that consecutive layers' weight gradients can be one batched
        launch; else one tensor per layer."""
        self.pre, self.embed, self.ff_norm = prefix, embed, ff_norm
        self.rows, self.L, self.nl, self.heads, self.dkv, self.dff, self.D = rows, seq, nl, heads, dkv, dff, D
        self.ids, self.mask, self.bucket = ids, mask, bucket
        self.site, (self.k_inner, self.k_branch) = site, ff_kinds
        self.embed_site, self.final_site = embed_site, final_site
        t, B = eng._t, eng.B
        self.PB = t((heads, seq, seq))
        self.HS = [t((rows, D)) for _ in range(nl + 1)]
        if stacked:
            self.N0S, self.OS, self.N1S = (t((nl, rows, D), BF16) for _ in range(3))
            self.FFS = t((nl, rows, dff), BF16)
            self.N0, self.O, self.N1, self.FF = ([s[nl - 1 - i] for i in range(nl)]
                                                 for s in (self.N0S, self.OS, self.N1S, self.FFS))
        else:
            self.N0, self.O, self.N1 = ([t((rows, D), BF16) for _ in range(nl)] for _ in range(3))
            self.FF = [t((rows, dff), BF16) for _ in range(nl)]
        self.QKV = [t((rows, 3 * D), BF16) for _ in range(nl)]
        self.PT = [t((B, heads, seq, seq)) for _ in range(nl)]
        self.HM = [t((rows, D)) for _ in range(nl)]
        self.R0, self.R1 = [t(rows) for _ in range(nl)], [t(rows) for _ in range(nl)]    # R1: the FF norm's
        self.RF, self.OUT32, self.OUT16 = t(rows), t((rows, D)), t((rows, D), BF16)
        # a decoder's cross-attention context and the residual stream behind it (the FF's input)
        self.CTX = [t((rows, D), BF16) for _ in range(nl)] if decoder else None
        self.HX = [t((rows, D)) for _ in range(nl)] if decoder else self.HM
        self.dSB = t((nl, B, heads, seq, seq))        # per-layer, per-sample attention dS (rel-bias grad)
        self.dPB = t((heads, seq, seq))
        self.layer_start = []                         # index of each layer's first forward call

    # ------------------------------------------------------------------ forward
    def _norm_fwd(self, eng, f, x, wname, y32, y16, rstd, site=None):
        kp = []
        d = eng._dptr(site, kp) if site is not None else None
        eng._call(f, "vqa_rmsnorm_fwd", x, eng.p32[wname], y32, y16, rstd, self.rows, self.D, 1e-6, d,
                  extra=(kp + [eng.RNG]) if site is not None else ())

    def _rms_kw(self, eng, wname, y16, rstd, ws, y32=None, drop=None):
        """ops.gemm_desc keywords of an RMSNorm fused behind the GEMM that writes its input."""
        kw = dict(norm=L.NORM_RMS, norm_w=eng.p32[wname], norm_eps=1e-6, norm_y32=y32, norm_y16=y16, norm_rstd=rstd,
                  workspace=ws)
        d = eng._drop(drop) if drop is not None else None
        if d is not None:
            kw.update(norm_drop=d, keep=(eng.RNG,))
        return kw

    def _attn_kw(self, i):
        q, D, Lq = self.QKV[i], self.D, self.L
        return dict(q=q, ldq=3 * D, k=ops.addr(q, D), ldk=3 * D, v=ops.addr(q, 2 * D), ldv=3 * D, p=self.PT[i],
                    bias=self.PB, key_mask=self.mask, heads=self.heads, lq=Lq, lk=Lq, dh=self.dkv, scale=1.0,
                    drop=self.site(i, 0))

    def plan_forward(self, eng, f, fuse=None, cross=None):
        """The embedding, the rel-bias, the layers and the final norm.  fuse: the zero-filled
        arrival-counter block of norm-carrying GEMMs -- every norm but layer 0's ln0 then runs as
        the tail of the GEMM that writes its input (vqa_gemm_desc.norm; same bits) -- or None:
        stand-alone norms.  cross(f, stack, i): a decoder's cross-attention sub-layer, HM[i] ->
        HX[i]."""
        assert fuse is None or cross is None
        T, D, nl, pre = self.rows, self.D, self.nl, self.pre
        kp = []
        eng._call(f, "vqa_embedding_fwd", self.ids, eng.p32[self.embed], self.HS[0], T, D, S.T5_VOCAB,
                  eng._dptr(self.embed_site, kp), extra=kp + [eng.RNG])
        eng._call(f, "vqa_t5_relbias_fwd", eng.p32[pre + "relbias"], self.bucket, self.PB, self.heads, self.L, self.L)
        final = dict(wname=pre + "final_ln", y32=self.OUT32, y16=self.OUT16, rstd=self.RF)
        for i in range(nl):
            p = f"{pre}{i}."
            self.layer_start.append(len(f))
            if i == 0 or fuse is None:                       # fused: the previous layer's wo wrote N0 / R0
                self._norm_fwd(eng, f, self.HS[i], p + "ln0", None, self.N0[i], self.R0[i])
            eng._linear(f, self.N0[i], p + "qkv_w", T, out16=self.QKV[i], bias=False)
            eng._attn(f, "vqa_attn_fwd", o=self.O[i], ldo=D, batch=eng.B, **self._attn_kw(i))
            # h + dropout(attention output)   (T5LayerSelfAttention :400)
            nrm = None if fuse is None else self._rms_kw(eng, p + self.ff_norm, self.N1[i], self.R1[i], fuse)
            eng._linear(f, self.O[i], p + "o_w", T, out32=self.HM[i], bias=False, res32=self.HS[i],
                        drop=self.site(i, 1), norm=nrm)
            if cross is not None:
                cross(f, self, i)
            # dropout(relu(wi h)) (T5DenseActDense :86), then h + dropout(wo .) (T5LayerFF :140)
            if fuse is None:
                self._norm_fwd(eng, f, self.HX[i], p + self.ff_norm, None, self.N1[i], self.R1[i])
            eng._linear(f, self.N1[i], p + "wi", T, out16=self.FF[i], bias=False, relu=True,
                        drop=self.site(i, self.k_inner))
            nrm = None
            if fuse is not None and i + 1 < nl:              # wo carries the next layer's ln0 ...
                nrm = self._rms_kw(eng, f"{pre}{i + 1}.ln0", self.N0[i + 1], self.R0[i + 1], fuse)
            elif fuse is not None:                           # ... the last one the final norm and its dropout
                nrm = self._rms_kw(eng, ws=fuse, drop=self.final_site, **final)
            eng._linear(f, self.FF[i], p + "wo", T, out32=self.HS[i + 1], bias=False, res32=self.HX[i],
                        drop=self.site(i, self.k_branch), norm=nrm)
        if fuse is None:
            self._norm_fwd(eng, f, self.HS[-1], site=self.final_site, **final)

    # ------------------------------------------------------------------ backward
    def norm_bwd(self, eng, b, dy, x, rstd, wname, dres, dx32, dx16, sites=(None, None, None)):
        """vqa_rmsnorm_bwd of norm `wname` over x: dx32 = dres + the norm's input gradient, dx16 its
        bf16 copy; sites: the dropouts masking dy, dx32 and dx16.  The gain's gradient is deferred."""
        kp = []
        ws = eng._norm_ws(self.rows)
        ds = [eng._dptr(s, kp) if s is not None else None for s in sites]
        eng._call(b, "vqa_rmsnorm_bwd", dy, x, rstd, eng.p32[wname], dres, dx32, dx16, None, 0.0, ws, self.rows, self.D,
                  *ds, extra=kp + [eng.RNG])
        eng._defer(ws, L.load().vqa_norm_bwd_parts(self.rows), self.D, self.D, eng.g32[wname])

    def plan_backward(self, eng, b, g, dxdw, after_layer=None, cross=None):
        """From the final norm's backward down to vqa_t5_relbias_bwd.  g: T5Grads.
        dxdw(b, dy16, x16, wname, rows, **dx keywords) issues a GEMM's input gradient and, if the
        engine wants it in line, its weight gradient.  after_layer(i) runs after layer i's calls,
        and as after_layer(nl) after the final norm's.  cross(b, stack, i, g): a decoder's
        cross-attention sub-layer, g.dHX32 -> g.dHM32 with the attention branch's gradient in
        g.dHM[i]."""
        T, D, nl, pre = self.rows, self.D, self.nl, self.pre
        after_layer = after_layer or (lambda i: None)
        ks = eng.drop_scale if eng.p_drop > 0.0 else 1.0      # relu-mask dX: kept elements carry 1/(1-p)
        self.norm_bwd(eng, b, g.dOUT, self.HS[-1], self.RF, pre + "final_ln", None, g.dH32, g.dH16[-1],
                      (self.final_site, None, self.site(nl - 1, self.k_branch)))
        after_layer(nl)
        for i in reversed(range(nl)):
            p = f"{pre}{i}."
            dq = g.dQKV[i]
            dxdw(b, g.dH16[i], self.FF[i], p + "wo", T, out16=g.dF[i], mask16=self.FF[i], alpha=ks)
            dxdw(b, g.dF[i], self.N1[i], p + "wi", T, out32=g.dC32)
            # the FF norm's bf16 gradient carries the dropout of the branch below it: the attention's,
            # in a decoder the cross-attention's
            self.norm_bwd(eng, b, g.dC32, self.HX[i], self.R1[i], p + self.ff_norm, g.dH32,
                          g.dHM32 if cross is None else g.dHX32, g.dHM[i],
                          (None, None, self.site(i, 1 if cross is None else 3)))
            if cross is not None:
                cross(b, self, i, g)
            dxdw(b, g.dHM[i], self.O[i], p + "o_w", T, out16=g.dO16)
            eng._attn(b, "vqa_attn_bwd", batch=eng.B, dout=g.dO16, lddo=D, dq=dq, lddq=3 * D, dk=ops.addr(dq, D),
                      lddk=3 * D, dv=ops.addr(dq, 2 * D), lddv=3 * D, dbias=self.dSB[i], **self._attn_kw(i))
            dxdw(b, dq, self.N0[i], p + "qkv_w", T, out32=g.dC32)
            # layer 0: dH32 becomes the embedding gradient (masked by the embedding dropout :725);
            # otherwise dH16 is the FF branch gradient of layer i-1
            self.norm_bwd(eng, b, g.dC32, self.HS[i], self.R0[i], p + "ln0", g.dHM32, g.dH32,
                          g.dH16[i - 1] if i > 0 else None,
                          (None, self.embed_site, None) if i == 0 else (None, None, self.site(i - 1, self.k_branch)))
            after_layer(i)
        # the relative-position bias is shared by all layers: dPB = sum over (layer, sample) of dS,
        # one fixed-order reduction after the last layer instead of one per layer
        eng._call(b, "vqa_batch_sum", self.dSB, nl * eng.B, self.heads * self.L * self.L, self.dPB, 0.0)
        eng._call(b, "vqa_t5_relbias_bwd", self.dPB, self.bucket, eng.g32[pre + "relbias"], self.heads, self.L, self.L,
                  S.T5_BUCKETS)
