"""SGAStack: the one plan of the SGA blocks (model/multi_head_vision_text_attn.py:145-158), the
fusion segment of engine.VQAEngine, beside t5_stack.T5Stack.

A block is  x1 = norm1(x + drop(mhatt1(x, x, x))),  x2 = norm2(x1 + drop(mhatt2(y, y, x1))),
out = norm3(x2 + drop(ffn(x2))),  with x the T5 output for every block and y chained.
The stack allocates the blocks' forward and backward buffers and appends, through the engine's
builders (engine_base.EngineBase):
  kv0       block 0's k|v projection, which reads only the vision tokens (the vision branch);
  forward   the self-attention halves of all blocks first -- they read only x: one q|k|v GEMM
            over the side-by-side weights, the attentions (one grouped launch), one merge batched
            over the blocks with norm1 -- then one batched q2 GEMM and per block k|v, cross-attention,
            merge + norm2, fc1, fc2 + norm3;
  backward  the blocks' chains of input gradients top down, then per weight ONE gradient launch
            batched over the blocks (sga_dw_batch), then the self-attention halves batched.
Buffers that one batched launch reads or writes are stacked at a constant stride: the inputs of
the q2 / m2 / fc1 / fc2 weight gradients in backward order (slot NB-1-n, the arena's order:
layout.ParamLayout.stride), the self-attention halves in block order.  Where the gradients land
(SGAGrads), the head, the ready marks and the norm-carrying GEMMs' counter block are the engine's.
"""
from __future__ import annotations

import math
from collections import namedtuple

from . import lib as L
from . import ops
from .engine_base import BF16

# Where the backward reads and writes (the engine's; the T5 backward reuses the scratch): dY the
# ping-pong pair of block output gradients (dY[(NB-1) & 1] is the head's), dA32 / dC32 / dO16
# scratch, dTXT the text gradient, dVIS32 / dVIS16 the vision tokens'.
SGAGrads = namedtuple("SGAGrads", "dY dA32 dC32 dO16 dTXT dVIS32 dVIS16")

_NORM_OUT = {1: ("X1", "X1h"), 2: ("X2", "X2h"), 3: ("OUT", "OUTh")}      # norm k's fp32 / bf16 outputs
_NORM_BIAS = {1: "m1_b", 2: "m2_b", 3: "fc2_b"}     # the bias of the GEMM below norm k (its gradient: ln_bwd)


def sga_site(block, kind):
    """kind 0 mhatt1 probs, 1 dropout1, 2 mhatt2 probs, 3 dropout2, 4 MLP inner, 5 dropout3
    (multi_head_vision_text_attn.py:84, 146, 84, 150, 99, 154)"""
    return 128 + 8 * block + kind


class SGAStack:
    def __init__(self, eng, txt32, txt16, vis16, norm_ws=None):
        """txt32 / txt16: the T5 output (every block's x); vis16: the vision tokens (block 0's
        y).  norm_ws: the zero-filled arrival-counter block of norm-carrying GEMMs -- every norm
        then runs as the tail of the GEMM that writes its input (fuse_norm; same bits) -- or
        None: stand-alone norms."""
        self.txt32, self.txt16, self.vis16, self.ws = txt32, txt16, vis16, norm_ws
        self.NB, self.T, self.L, self.D, self.heads, self.dh = eng.NB, eng.T, eng.L, eng.D, eng.sga_heads, eng.sga_dh
        NB, T, D, B, Lq, V, t = eng.NB, eng.T, eng.D, eng.B, eng.L, eng.V_TOK, eng._t
        fuse = norm_ws is not None
        # the self-attention halves of all blocks share batched buffers: q|k|v of block n in
        # columns [n*3D, (n+1)*3D) of QKV1A, merge in / out in [n]
        self.QKV1A = t((T, NB * 3 * D), BF16)
        self.O1A, self.S1A = t((NB, T, D), BF16), t((NB, T, D))
        self.P1A = t((NB, B, self.heads, Lq, Lq))          # their attention probabilities, stacked
        # inputs of the blocks' q2 / m2 / fc1 / fc2 weight gradients and the cross-attention
        # queries, stacked in backward order (slot NB-1-n) for the batched launches
        self.X1hS, self.O2S, self.X2hS, self.FFhS, self.Q2S = (t((NB, T, D), BF16) for _ in range(5))
        if fuse:
            # the batched merge writes every block's norm1 outputs: one signed stride per output
            # kind, so X1 is stacked like X1hS, the statistics in block order
            self.X1S, self.MU1S, self.RS1S = t((NB, T, D)), t((NB, T)), t((NB, T))
        self.blocks = []
        for n in range(NB):
            ly, lk = (V, eng.fh * eng.fh) if n == 0 else (T, Lq)       # rows / per-sample length of y
            r = NB - 1 - n
            self.blocks.append(dict(
                ly=ly, lk=lk, P1=self.P1A[n], O1=self.O1A[n], S1=self.S1A[n],
                X1=self.X1S[r] if fuse else t((T, D)), X1h=self.X1hS[r],
                MU1=self.MU1S[n] if fuse else t(T), RS1=self.RS1S[n] if fuse else t(T),
                Q2=self.Q2S[r], KV2=t((ly, 2 * D), BF16), P2=t((B, self.heads, Lq, lk)),
                O2=self.O2S[r], S2=t((T, D)), X2=t((T, D)), X2h=self.X2hS[r], MU2=t(T), RS2=t(T),
                FFh=self.FFhS[r], S3=t((T, D)), OUT=t((T, D)), OUTh=t((T, D), BF16), MU3=t(T), RS3=t(T)))
        # backward: every bf16 gradient a weight-gradient GEMM reads has a buffer of its own, so the
        # dW GEMMs can trail the dX chain on another stream without write-after-read hazards
        self.dA3S, self.dBS, self.dA2S, self.dQS = (t((NB, T, D), BF16) for _ in range(4))
        self.dKV = [t((s["ly"], 2 * D), BF16) for s in self.blocks]
        self.dTA = [t((T, D)), t((T, D))]              # running text gradient of the norm1s (ping-pong)
        self.dA1A, self.dO1A = t((NB, T, D), BF16), t((NB, T, D), BF16)
        self.dQKV1A = t((T, NB * 3 * D), BF16)
        # the runs of segments one launch steps over, each at one constant stride: the self-attention
        # halves' side by side in block order (one matrix), the rest in the arena's order, top block first
        lay, self.down = eng.lay, list(reversed(range(NB)))
        for w in ("qkv1_w", "qkv1_b", "m1_w", "m1_b"):
            assert lay.stride(self.names(w)) in (0, lay[f"sga0.{w}"].numel), w
        self.st_q2, self.st_ln1 = lay.stride(self.names("q2_w", self.down)), lay.stride(self.names("ln1_g"))
        assert lay.stride(self.names("q2_b", self.down)) == self.st_q2
        assert lay.stride(self.names("ln1_b")) == self.st_ln1 and self.st_ln1 % 4 == 0
        # vqa_attn_desc group fields of the self-attentions: all NB blocks in one launch (block n:
        # q|k|v columns n*3D of QKV1A, O1A[n] / dO1A[n], P1A[n], dropout site sga_site(n, 0)), or
        # one block per launch (sga_attn_group=False)
        self.grp = dict(groups=1)
        if eng.sga_attn_group and NB > 1:
            self.grp = dict(groups=NB, gstride_qkv=3 * D, gstride_o=T * D, gstride_dout=T * D,
                            gstride_p=self.P1A[0].numel(), gdrop_site_stride=sga_site(1, 0) - sga_site(0, 0))
        self._akw = dict(batch=B, heads=self.heads, lq=Lq, dh=self.dh, scale=1.0 / math.sqrt(self.dh))

    # ------------------------------------------------------------------ the pieces
    def names(self, w, order=None):
        """Segment `w` of every block, in block order or in `order`."""
        return [f"sga{n}.{w}" for n in (range(self.NB) if order is None else order)]

    def _self_kw(self, n):
        """vqa_attn_desc keywords of the self-attention launch that starts at block n."""
        q, D, ld = self.QKV1A, self.D, self.NB * 3 * self.D
        c0 = n * 3 * D
        return dict(q=ops.addr(q, c0), ldq=ld, k=ops.addr(q, c0 + D), ldk=ld, v=ops.addr(q, c0 + 2 * D), ldv=ld,
                    p=self.blocks[n]["P1"], lk=self.L, drop=sga_site(n, 0), **self._akw, **self.grp)

    def _cross_kw(self, n):
        """... of block n's cross-attention (q from x1, k|v from y)."""
        s, D = self.blocks[n], self.D
        return dict(q=s["Q2"], ldq=D, k=s["KV2"], ldk=2 * D, v=ops.addr(s["KV2"], D), ldv=2 * D, p=s["P2"],
                    lk=s["lk"], drop=sga_site(n, 2), **self._akw)

    def _ln(self, eng, n, k):
        """(gamma, beta, y32, y16, mean, rstd) of block n's norm k."""
        s, p = self.blocks[n], f"sga{n}.ln{k}_"
        return (eng.p32[p + "g"], eng.p32[p + "b"], s[_NORM_OUT[k][0]], s[_NORM_OUT[k][1]], s[f"MU{k}"], s[f"RS{k}"])

    def ln_fwd(self, eng, f, n, k, gemm, blocks=1, **strides):
        """The GEMM that writes S{k} of block n (`gemm`: its _wgemm keywords; batched over `blocks`
        blocks) and the LayerNorm k behind it: the GEMM's tail (fuse_norm; strides: the norm's
        strides over a batch) or a launch of its own per block."""
        if self.ws is None:
            eng._wgemm(f, **gemm)
            for j in range(n, n + blocks):
                eng._call(f, "vqa_layernorm_fwd", self.blocks[j][f"S{k}"], *self._ln(eng, j, k), self.T, self.D, 1e-5)
        else:
            g, b, y32, y16, mean, rstd = self._ln(eng, n, k)
            eng._wgemm(f, **gemm, norm=L.NORM_LAYER, norm_w=g, norm_b=b, norm_eps=1e-5, norm_y32=y32, norm_y16=y16,
                       norm_mean=mean, norm_rstd=rstd, workspace=self.ws, **strides)

    def ln_bwd(self, eng, b, n, k, dy, dres, dx32, dx16):
        """vqa_layernorm_bwd of block n's norm k: dx32 = dres + the norm's input gradient, dx16 the
        dropout-masked branch below it, whose column sums are that GEMM's bias gradient.  gamma,
        beta and the bias are deferred: ws = [parts][dgamma | dbeta | dsum]."""
        s, p, D = self.blocks[n], f"sga{n}.", self.D
        kp = []
        ws = eng._norm_ws()
        eng._call(b, "vqa_layernorm_bwd", dy, s[f"S{k}"], s[f"MU{k}"], s[f"RS{k}"], eng.p32[f"{p}ln{k}_g"], dres,
                  dx32, dx16, None, None, ws, self.T, D, eng._dptr(sga_site(n, 2 * k - 1), kp),
                  eng.g32[p + _NORM_BIAS[k]], extra=kp + [eng.RNG])
        for j, nm in enumerate((f"ln{k}_g", f"ln{k}_b", _NORM_BIAS[k])):
            eng._defer(ws, L.load().vqa_norm_bwd_parts(self.T), 3 * D, D, eng.g32[p + nm], offset=j * D)

    # ------------------------------------------------------------------ forward
    def plan_kv0(self, eng, f):
        s = self.blocks[0]
        eng._linear(f, self.vis16, "sga0.kv2_w", s["ly"], out16=s["KV2"])

    def plan_forward(self, eng, f):
        """The fusion segment up to the last block's output (blocks[-1]["OUT"])."""
        NB, T, D = self.NB, self.T, self.D
        eng._wgemm(f, self.txt16, "sga0.qkv1_w", T, n=NB * 3 * D, c16=self.QKV1A, ldc16=NB * 3 * D,
                   bias=eng.p32["sga0.qkv1_b"])
        for n in range(0, NB, self.grp["groups"]):
            eng._attn(f, "vqa_attn_fwd", o=self.blocks[n]["O1"], ldo=D, keep=(self.QKV1A, self.O1A, self.P1A),
                      **self._self_kw(n))
        self.ln_fwd(eng, f, 0, 1, dict(
            x16=self.O1A, wname="sga0.m1_w", m=T, c32=self.S1A, ldc32=D, bias=eng.p32["sga0.m1_b"], res32=self.txt32,
            ldres=D, batch=NB, stride_b=D * D, stride_c32=T * D, stride_res=0, stride_bias=D, drop=sga_site(0, 1),
            drop_site_stride=sga_site(1, 1) - sga_site(0, 1)),
            blocks=NB, stride_norm_w=self.st_ln1, stride_norm_y=-T * D, stride_norm_stat=T)
        # the blocks' cross-attention queries read only their norm1 outputs: one launch batched
        # over the blocks (stack slot NB-1-n = the blocks' order in the arena)
        eng._wgemm(f, self.X1hS, f"sga{NB - 1}.q2_w", T, c16=self.Q2S, ldc16=D, bias=eng.p32[f"sga{NB - 1}.q2_b"],
                   batch=NB, stride_b=self.st_q2, stride_c16=T * D, stride_bias=self.st_q2)
        y16 = self.vis16
        for n, s in enumerate(self.blocks):
            p = f"sga{n}."
            if n > 0:
                eng._linear(f, y16, p + "kv2_w", s["ly"], out16=s["KV2"])
            eng._attn(f, "vqa_attn_fwd", o=s["O2"], ldo=D, **self._cross_kw(n))
            self.ln_fwd(eng, f, n, 2, eng._linear_kw(s["O2"], p + "m2_w", T, out32=s["S2"], res32=s["X1"],
                                                     drop=sga_site(n, 3)))
            eng._linear(f, s["X2h"], p + "fc1_w", T, out16=s["FFh"], relu=True, drop=sga_site(n, 4))
            self.ln_fwd(eng, f, n, 3, eng._linear_kw(s["FFh"], p + "fc2_w", T, out32=s["S3"], res32=s["X2"],
                                                     drop=sga_site(n, 5)))
            y16 = s["OUTh"]

    # ------------------------------------------------------------------ backward
    def plan_backward(self, eng, b, g, mark):
        """From the head's output gradient g.dY[(NB-1) & 1] down to g.dTXT and g.dVIS32 / dVIS16.
        mark(segment): the engine's ready mark, called where a block's gradients are final."""
        NB, T, D = self.NB, self.T, self.D
        ks = eng.drop_scale if eng.p_drop > 0.0 else 1.0      # relu-mask dX: kept elements carry 1/(1-p)
        # the blocks' q2 / m2 / fc1 / fc2 weight gradients (D x D, K = T each) are left out of the
        # sequential block chain and computed after it as one launch per weight batched over the
        # blocks (the block chain then runs its input gradients alone)
        batched = eng.sga_dw_batch
        dxdw = eng._dx_only if batched else eng._dxdw
        for n in reversed(range(NB)):
            s, p, r = self.blocks[n], f"sga{n}.", NB - 1 - n
            dA3, dA2, dB, dQ, dKV = self.dA3S[r], self.dA2S[r], self.dBS[r], self.dQS[r], self.dKV[n]
            # norm3 + FFN: dA32 = grad of x + dropout3(ffn(x)) (the residual), dA3 = its dropout3 branch
            self.ln_bwd(eng, b, n, 3, g.dY[n & 1], None, g.dA32, dA3)
            dxdw(b, dA3, s["FFh"], p + "fc2_w", T, out16=dB, mask16=s["FFh"], alpha=ks)
            dxdw(b, dB, s["X2h"], p + "fc1_w", T, bias_from=dB, out32=g.dC32, res32=g.dA32)
            # norm2 + cross attention (q from x, k/v from y)
            self.ln_bwd(eng, b, n, 2, g.dC32, None, g.dA32, dA2)
            dxdw(b, dA2, s["O2"], p + "m2_w", T, out16=g.dO16)
            eng._attn(b, "vqa_attn_bwd", dout=g.dO16, lddo=D, dq=dQ, lddq=D, dk=dKV, lddk=2 * D,
                      dv=ops.addr(dKV, D), lddv=2 * D, **self._cross_kw(n))
            dxdw(b, dQ, s["X1h"], p + "q2_w", T, bias_from=dQ, out32=g.dC32, res32=g.dA32)
            y16 = self.vis16 if n == 0 else self.blocks[n - 1]["OUTh"]
            out = dict(out32=g.dVIS32, out16=g.dVIS16) if n == 0 else dict(out32=g.dY[(n - 1) & 1])
            eng._dxdw(b, dKV, y16, p + "kv2_w", s["ly"], bias_from=dKV, **out)
            # norm1: its residual input is the T5 output, so the text gradient of the blocks
            # accumulates here (dres = the running sum); the merge branch goes to dA1A[n]
            self.ln_bwd(eng, b, n, 1, g.dC32, None if n == NB - 1 else self.dTA[(n + 1) & 1], self.dTA[n & 1],
                        self.dA1A[n])
            if not batched:
                mark(f"sga{n}.ln3_b")
        if batched:
            for w, dys, xs in (("fc2_w", self.dA3S, self.FFhS), ("fc1_w", self.dBS, self.X2hS),
                               ("m2_w", self.dA2S, self.O2S), ("q2_w", self.dQS, self.X1hS)):
                eng._dw_batched(b, dys, xs, self.names(w, self.down), T)
        # the blocks' self-attention halves, batched: merge dX / dW (batch NB), the attentions,
        # then ONE q|k|v dX GEMM over K = NB * 3D (it also sums the blocks' text gradients, plus
        # the norm1 residual sum as res32) beside ONE q|k|v dW GEMM
        W = NB * 3 * D
        eng._gemm(b, self.dA1A, eng.p16["sga0.m1_w"], T, D, D, lda=D, ldb=D, b_trans=True, c16=self.dO1A,
                  ldc16=D, batch=NB, stride_a=T * D, stride_b=D * D, stride_c16=T * D)
        eng._dw_batched(b, self.dA1A, self.O1A, self.names("m1_w"), T, stride=D * D)
        dq = self.dQKV1A
        for n in reversed(range(0, NB, self.grp["groups"])):
            c0 = n * 3 * D
            eng._attn(b, "vqa_attn_bwd", dout=self.dO1A[n], lddo=D, dq=ops.addr(dq, c0), lddq=W,
                      dk=ops.addr(dq, c0 + D), lddk=W, dv=ops.addr(dq, c0 + 2 * D), lddv=W,
                      keep=(self.QKV1A, dq, self.P1A, self.dO1A), **self._self_kw(n))
        eng._gemm(b, dq, eng.p16["sga0.qkv1_w"], T, D, W, lda=W, ldb=D, b_trans=True, c32=g.dTXT, ldc32=D,
                  res32=self.dTA[0], ldres=D)
        eng._gemm(b, dq, self.txt16, W, D, T, lda=W, ldb=D, a_trans=True, b_trans=True, c32=eng.g32["sga0.qkv1_w"],
                  ldc32=D)
        b[-1].side = True                          # not paired: the K = NB * 3D dX wants split-K
        lib = L.load()
        ws = eng._t(lib.vqa_colsum_workspace_floats(T, W))
        eng._call(b, "vqa_colsum", dq, 1, T, W, W, None, 0.0, ws)
        eng._defer(ws, lib.vqa_colsum_parts(T), W, W, eng.g32["sga0.qkv1_b"], keep=(eng.G32,))   # NB biases in a row
