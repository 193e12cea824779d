"""Plain torch-CPU restatement of the attention kernels (csrc/attention.hip, csrc/attention_mfma.hip),
written from the formulas of include/vqa_hip.h and not from autograd.

  reference(case)      the chain in fp64: what tests/test_attn_parity_gpu.py compares the kernels with.
  model(case, path)    the same chain in fp32 with the roundings that `path`'s kernels perform (read from
                       the kernels; listed at model()).  It is a yardstick, never a reference: what a
                       different but equally long evaluation with the same operand formats loses to fp64.
  normalisers(case)    per output element, the sum of the MAGNITUDES of the terms it is made of.  Errors
                       are measured relative to these and not to a row maximum: dS = P (dP - D) cancels,
                       and a row's largest |dS| says nothing about the rounding its terms carry.
  yardstick(path)      per tensor, the largest |model - reference| / normaliser over the path's case
                       table below.  The GPU bound is FACTOR x the yardstick (bound()); nothing a kernel
                       computed enters it.

Tensors are [B, H, L, dh]; rows() / unrows() convert to the fused-row layout the kernels read, element
(b, i, h, e) at (b*L + i)*ld + h*dh + e.  All of q, k, v, dO are bf16-exact, so every difference between
a kernel and reference() is the kernel's own arithmetic.

`wrong=` applies one deliberate mistake to the chain (MISTAKES); tests/test_attn_ref_cpu.py measures
with it how far a wrong kernel would sit from the reference.  No wrong kernel is ever run."""
import collections
import functools
import math

import torch

from oracle import vqa_oracle as orc

FMIN = float(torch.finfo(torch.float32).min)
FACTOR = 4.0                                   # bound = FACTOR * yardstick, the project's factor
SEED, COUNTER, SITE = 11, 4, 77                # dropout stream of every case (vqa_dropout rng[0], rng[1], site)
MFMA, LONG, VALU = "mfma", "long", "valu"      # vqa_attn_path
PROBS = "probs"                                # vqa_attn_probs: P alone, any lq, lk
TENSORS = ("o", "p", "dq", "dk", "dv", "ds")

# one case: shape, bias kind (None, "rel", "causal": rel-bias with finfo.min where j > i), key lengths per
# sample (None = no key mask; 0 = an all-padded sample), dropout p
Spec = collections.namedtuple("Spec", "path B H lq lk dh bias lens p")


def name(s):
    return (f"{s.path}_b{s.B}h{s.H}_{s.lq}x{s.lk}x{s.dh}" + (f"_{s.bias}" if s.bias else "")
            + ("_mask" + "-".join(map(str, s.lens)) if s.lens else "") + ("_drop" if s.p else ""))


# ------------------------------------------------------------------------------------- case tables
NT_LKS = {1: (1, 4, 31, 32), 2: (33, 64), 3: (65, 96), 4: (97, 128), 5: (129, 160)}    # key tiles -> key lengths
LQS = (1, 20, 31, 32)
DHS = (64, 96, 128)


def _sweep():
    """Every MFMA instantiation (dh x NT key tiles), two key lengths each (all four at NT 1), plain and
    with dropout.  lq cycles through LQS; (batch, heads) alternates between (3, 1) and (1, 3) -- odd pair
    counts, so the second wave of a two-wave block (NT <= 2) is dead in the last block -- in an order
    that gives every lq both; one case is (2, 2)."""
    out, i = {}, 0
    for dh in DHS:
        for nt, lks in NT_LKS.items():
            for lk in lks:
                bh = (2, 2) if i == 7 else ((3, 1), (1, 3))[(i + i // 4) % 2]
                out.setdefault((dh, nt), []).extend(
                    Spec(MFMA, bh[0], bh[1], LQS[i % 4], lk, dh, None, None, p) for p in (0.0, 0.1))
                i += 1
    return out


SWEEP = _sweep()                               # {(dh, NT): [Spec]}
BIAS = (                                       # rel-bias, key mask and causal cases of the MFMA kernels
    Spec(MFMA, 2, 2, 4, 4, 64, "rel", None, 0.0),            # float4 row of one group; lq == lk
    Spec(MFMA, 3, 1, 20, 33, 96, "rel", None, 0.1),          # scalar row loads
    Spec(MFMA, 1, 3, 32, 64, 128, "rel", None, 0.0),
    Spec(MFMA, 3, 1, 31, 68, 64, "rel", None, 0.0),          # NT 3, float4 rows
    Spec(MFMA, 1, 3, 32, 157, 96, "rel", None, 0.1),         # NT 5, scalar rows
    Spec(MFMA, 3, 1, 31, 31, 64, "rel", (31, 17, 0), 0.0),   # ragged, one all-padded sample
    Spec(MFMA, 3, 2, 20, 64, 96, "rel", (64, 1, 40), 0.1),
    Spec(MFMA, 3, 1, 32, 64, 128, None, (64, 40, 1), 0.0),   # a key mask without a bias
    Spec(MFMA, 3, 1, 1, 20, 64, None, (0, 5, 20), 0.1),
    Spec(MFMA, 3, 1, 20, 20, 64, "causal", (0, 5, 20), 0.0),
    Spec(MFMA, 3, 3, 32, 32, 96, "causal", (32, 0, 9), 0.1),
)
VALU_CASES = (                                 # lq > 32 or dh not 64 / 96 / 128: the scalar kernels
    Spec(VALU, 3, 1, 33, 1, 8, None, None, 0.0),
    Spec(VALU, 1, 3, 48, 40, 64, "rel", (33,), 0.1),
    Spec(VALU, 3, 1, 64, 64, 8, "causal", (64, 0, 30), 0.0),
    Spec(VALU, 1, 3, 33, 64, 96, None, None, 0.1),
    Spec(VALU, 3, 1, 64, 40, 96, None, (40, 7, 0), 0.0),
    Spec(VALU, 2, 2, 48, 48, 64, "rel", None, 0.0),
    Spec(VALU, 1, 3, 20, 31, 8, None, None, 0.1),            # an MFMA shape but for its head dim
    Spec(VALU, 1, 1, 63, 63, 64, None, None, 0.0),           # 65,520 B of LDS in the backward: the largest
)
LONG_CASES = tuple(Spec(LONG, b, h, lq, lk, dh, None, None, 0.0)
                   for dh in (64, 96)
                   for (b, h, lq, lk) in ((3, 1, 33, 33), (1, 3, 64, 1), (3, 1, 1, 161), (1, 3, 20, 100),
                                          (2, 2, 70, 97), (1, 1, 5, 1024)))
PROBS_CASES = (
    Spec(PROBS, 1, 3, 197, 197, 64, None, None, 0.0),        # ViT-base's map
    Spec(PROBS, 3, 2, 40, 70, 96, "rel", (70, 0, 33), 0.0),
    Spec(PROBS, 3, 1, 20, 20, 64, "causal", (0, 5, 20), 0.0),    # causal bias over fully padded keys
)


def table(path):
    """Every case the GPU test runs on `path`."""
    if path == MFMA:
        return tuple(s for v in SWEEP.values() for s in v) + BIAS
    return {VALU: VALU_CASES, LONG: LONG_CASES, PROBS: PROBS_CASES}[path]


# ------------------------------------------------------------------------------------------ inputs
def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def rows(t):
    """[B, H, L, dh] -> the fused-row matrix [B*L, H*dh]."""
    B, H, L, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * dh)


def unrows(m, B, H, L, dh):
    return m.reshape(B, L, H, dh).permute(0, 2, 1, 3)


@functools.lru_cache(maxsize=None)
def make_case(s):
    """Seeded inputs of a Spec: q (1.5 randn, so the scores spread over a few units), k, v, dO as
    bf16-exact fp32 [B, H, L, dh]; bias fp32 [H, lq, lk] or None; key mask int64 [B, lk] or None; the
    dropout multipliers [B, H, lq, lk] (ones without dropout); scale 1 / sqrt(dh)."""
    g = torch.Generator().manual_seed((((s.B * 7 + s.H) * 67 + s.lq) * 1031 + s.lk) * 131 + s.dh
                                      + 7919 * (None, "rel", "causal").index(s.bias) + 13 * sum(s.lens or ()))
    r = lambda *shape: torch.randn(*shape, generator=g)
    c = dict(spec=s, scale=1.0 / math.sqrt(s.dh))
    c["q"], c["k"] = _bf(1.5 * r(s.B, s.H, s.lq, s.dh)), _bf(r(s.B, s.H, s.lk, s.dh))
    c["v"], c["do"] = _bf(r(s.B, s.H, s.lk, s.dh)), _bf(r(s.B, s.H, s.lq, s.dh))
    c["bias"] = c["mask"] = None
    if s.bias:
        c["bias"] = r(s.H, s.lq, s.lk)
        if s.bias == "causal":
            c["bias"][:, torch.triu(torch.ones(s.lq, s.lk, dtype=torch.bool), 1)] = FMIN
    if s.lens:
        assert len(s.lens) == s.B
        c["mask"] = (torch.arange(s.lk)[None, :] < torch.tensor(s.lens)[:, None]).long()
    n = s.B * s.H * s.lq * s.lk
    c["mult"] = (torch.from_numpy(orc.dropout_multiplier(s.p, SEED, COUNTER, SITE, n)) if s.p
                 else torch.ones(n)).view(s.B, s.H, s.lq, s.lk)
    return c


# ------------------------------------------------------------------------------------------- chain
MISTAKES = (
    "no_fwd_scale",        # 1  S = Q K^T + bias
    "extra_key",           # 2  a zero-score key past lk counted in the softmax
    "last_key_dropped",    # 3
    "bias_T",              # 4  bias[h, j, i]
    "bias_by_batch",       # 5  bias[b] for bias[h]
    "o_pre_dropout",       # 6  O = P V
    "dp_no_mult",          # 7  dP = dO V^T
    "ds_from_dropped",     # 8  dS = drop(P) (dP - D)
    "d_post_dropout",      # 9  D = rowsum(drop(P) dP)
    "ds_no_d",             # 10 dS = P dP
    "dq_no_scale",         # 11
    "dq_scale_sq",         # 12
    "dk_no_scale",         # 13
    "dv_pre_dropout",      # 14 dV = P^T dO
    "second_fmin",         # 15 finfo.min added to a pair the bias already masks: -inf, a one-hot row
    "v_korder",            # 16 keys 4..7 and 8..11 of each 16 swapped in V only (the X-layout k-order)
    "p_post_dropout",      # 17 saved P = drop(P)
)


def applies(wrong, s):
    """Can the mistake change anything at this case?  One key: P = 1 whatever the scores are and dS = 0
    exactly, so nothing that acts through the scores or through dS shows.  The last key shows only where
    some sample keeps it (or is all padded: its uniform row changes)."""
    drop, many = s.p > 0, s.lk > 1
    return {"no_fwd_scale": many, "dq_no_scale": many, "dq_scale_sq": many, "dk_no_scale": many,
            "bias_T": bool(s.bias) and s.lq == s.lk, "bias_by_batch": bool(s.bias) and s.H > 1,
            "o_pre_dropout": drop, "dp_no_mult": drop and many, "ds_from_dropped": drop and many,
            "d_post_dropout": drop, "dv_pre_dropout": drop, "p_post_dropout": drop,
            "last_key_dropped": many and (not s.lens or any(n in (0, s.lk) for n in s.lens)),
            "second_fmin": s.bias == "causal" and bool(s.lens), "v_korder": s.lk > 4}.get(wrong, True)


def _chain(c, dt, path=None, wrong=None):
    """The attention forward and backward in dtype `dt`.  path = None: no rounding (the reference);
    else the operand and output roundings of that path's kernels."""
    s = c["spec"]
    q, k, v, do, mult = (c[n].to(dt) for n in ("q", "k", "v", "do", "mult"))
    scale = c["scale"]
    rnd = _bf if path == MFMA else (lambda t: t)          # regs_frag: P*mult and dS become bf16 MFMA operands
    out = _bf if path in (MFMA, LONG, VALU) else (lambda t: t)           # O, dQ, dK, dV are stored as bf16
    sc = q @ k.transpose(-1, -2)
    if wrong != "no_fwd_scale":
        sc = sc * scale
    bias = None
    if c["bias"] is not None:
        bias = c["bias"].to(dt)
        if wrong == "bias_T":
            bias = bias.transpose(-1, -2)
        bias = bias[torch.arange(s.B) % s.H][:, None] if wrong == "bias_by_batch" else bias[None]
        sc = sc + bias
    if c["mask"] is not None:
        add = (c["mask"] == 0)[:, None, None, :].expand_as(sc)
        if bias is not None and wrong != "second_fmin":    # one finfo.min per masked pair
            add = add & ~(bias <= 0.5 * FMIN).expand_as(sc)
        sc = torch.where(add, sc + FMIN, sc)
        sc = torch.where(sc < 1.5 * FMIN, torch.full_like(sc, -math.inf), sc)     # fp32 overflows here
    if wrong == "last_key_dropped" and s.lk > 1:
        sc = sc.clone()
        sc[..., -1] = -math.inf
    if wrong == "extra_key":
        sc = torch.cat([sc, torch.zeros_like(sc[..., :1])], -1)
    e = torch.exp(sc - sc.amax(-1, keepdim=True))
    z = e.sum(-1, keepdim=True)
    if wrong == "extra_key":
        e = e[..., :-1]
    if path == LONG:                                       # bf16 exp tile, 1/z in fp32 at the end
        return {"o": out((_bf(e) @ v) * (1.0 / z))}
    P = e * (1.0 / z) if path in (MFMA, PROBS) else e / z
    Pd = P * mult
    po = P if wrong == "o_pre_dropout" else Pd
    if wrong == "v_korder":
        n16 = -(-s.lk // 16) * 16
        perm = torch.arange(n16).view(-1, 4, 4)[:, [0, 2, 1, 3]].reshape(-1)
        pad = lambda t, dim: torch.cat([t, t.new_zeros(*t.shape[:dim], n16 - s.lk, *t.shape[dim + 1:])], dim)
        o = pad(rnd(po), 3) @ pad(v, 2)[:, :, perm]
    else:
        o = rnd(po) @ v
    dp = do @ v.transpose(-1, -2)
    if wrong != "dp_no_mult":
        dp = dp * mult
    D = ((Pd if wrong == "d_post_dropout" else P) * dp).sum(-1, keepdim=True)
    if wrong == "ds_no_d":
        D = torch.zeros_like(D)
    ds = (Pd if wrong == "ds_from_dropped" else P) * (dp - D)
    dq = (rnd(ds) @ k) * {"dq_no_scale": 1.0, "dq_scale_sq": scale * scale}.get(wrong, scale)
    dk = (rnd(ds).transpose(-1, -2) @ q) * (1.0 if wrong == "dk_no_scale" else scale)
    dv = rnd(P if wrong == "dv_pre_dropout" else Pd).transpose(-1, -2) @ do
    return {"o": out(o), "p": Pd if wrong == "p_post_dropout" else P, "dq": out(dq), "dk": out(dk),
            "dv": out(dv), "ds": ds, "dp": dp}


def reference(c, wrong=None):
    """fp64: S = scale Q K^T + bias, + one finfo.min where key_mask == 0 and the bias there is not already
    <= finfo.min / 2; P = softmax(S); O = (P mult) V; dP = (dO V^T) mult; D = rowsum(P dP); dS = P (dP - D);
    dQ = scale dS K; dK = scale dS^T Q; dV = (P mult)^T dO.  {"o", "p", "dq", "dk", "dv", "ds", "dp"}, each
    [B, H, ., .]; ds is the per-sample dS the kernels write to dbias."""
    return _chain(c, torch.float64, None, wrong)


def model(c, path):
    """fp32 with the roundings of `path`, read from the kernels:
      MFMA   P*mult, dS and P*mult again are rounded to bf16 before the P.V, dQ / dK and dV products
             (regs_frag); P = e * (1 / z); O, dQ, dK, dV rounded to bf16.  Saved P and dS stay fp32.
      LONG   the unnormalised exp tile is rounded to bf16, z sums the unrounded values, 1 / z is applied
             in fp32 at the end; O rounded to bf16.  Forward only.
      VALU   no operand rounding; P = e / z; O, dQ, dK, dV rounded to bf16.
      PROBS  P = e * (1 / z) alone."""
    return _chain(c, torch.float32, path)


def normalisers(c, ref=None):
    """Sums of magnitudes behind each output element (fp64), same shapes as the outputs."""
    ref = ref or reference(c)
    s = c["spec"]
    q, k, v, do, mult = (c[n].double() for n in ("q", "k", "v", "do", "mult"))
    P, dp = ref["p"], ref["dp"]
    Pd = P * mult
    n_ds = P * (dp.abs() + (P * dp.abs()).sum(-1, keepdim=True))
    return {"o": Pd @ v.abs(), "p": torch.ones_like(P), "dv": Pd.transpose(-1, -2) @ do.abs(), "ds": n_ds,
            "dq": c["scale"] * (n_ds @ k.abs()), "dk": c["scale"] * (n_ds.transpose(-1, -2) @ q.abs())}


def rel_err(got, ref, norm):
    """Largest |got - ref| / norm (float).  An element whose terms are all zero (a masked key's dK, a
    row dropout emptied) has norm 0 and must be exact."""
    err = (got.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    if bool((err[norm == 0] != 0).any()):
        return math.inf
    return float((err / norm.clamp_min(1e-300)).max()) if err.numel() else 0.0


def checked(path):
    """The tensors the GPU test compares on a path."""
    return {LONG: ("o",), PROBS: ("p",)}.get(path, TENSORS)


@functools.lru_cache(maxsize=None)
def _ref_cached(s):
    c = make_case(s)
    ref = reference(c)
    return ref, normalisers(c, ref)


def errors(s, got):
    """{tensor: largest error of got[tensor] relative to its normaliser} at Spec s."""
    ref, norm = _ref_cached(s)
    return {t: rel_err(got[t], ref[t], norm[t]) for t in checked(s.path) if got.get(t) is not None}


@functools.lru_cache(maxsize=None)
def yardstick(path):
    """{tensor: largest error of model(case, path) over table(path)}.  CPU only."""
    out = dict.fromkeys(checked(path), 0.0)
    for s in table(path):
        for t, e in errors(s, model(make_case(s), path)).items():
            out[t] = max(out[t], e)
    return out


def bound(path, tensor):
    """Relative bound of a kernel output of `path` against reference(), in units of its normaliser."""
    return FACTOR * yardstick(path)[tensor]


def distance(s, wrong):
    """How many bounds the mistaken chain sits from the reference at Spec s: the largest over the
    tensors the GPU test checks there."""
    return max(e / bound(s.path, t) for t, e in errors(s, reference(make_case(s), wrong)).items())
