"""tests/attn_ref.py is the fp64 reference of tests/test_attn_parity_gpu.py.  Here, on the CPU: it
equals torch.autograd of the attention as HF writes it (one combined extended mask); the yardsticks
it defines are of rounding size; and every mistake a kernel could plausibly make moves the reference
at least 5 of the GPU test's bounds (4 x yardstick) in a tensor that test checks, on that test's own
inputs, so the bounds separate right from wrong without a wrong kernel ever being run.

Yardsticks (largest |model - fp64| / normaliser over a path's case table):
  MFMA  o 6.5e-3  dq 4.6e-3  dk 6.2e-3  dv 7.5e-3  (bf16 operand + output rounding)  p 3.0e-7  ds 1.7e-6
  VALU  o 3.7e-3  dq 2.5e-3  dk 2.9e-3  dv 3.2e-3  (bf16 output rounding)            p 2.2e-7  ds 1.3e-6
  long  o 3.7e-3

Least distance of each mistake, in bounds, over the MFMA and VALU cases where it applies
(attn_ref.applies), and the case it is least at:
   1 no_fwd_scale      476558  mfma 20x4x64             10 ds_no_d          52441  mfma 1x97x64
   2 extra_key            408  mfma 32x157x96 rel drop  11 dq_no_scale         89  valu 20x31x8 drop
   3 last_key_dropped   47782  mfma 1x97x128            12 dq_scale_sq         15  mfma 1x97x96
   4 bias_T           1313911  mfma 4x4x64 rel          13 dk_no_scale        103  valu 20x31x8 drop
   5 bias_by_batch    6038674  mfma 20x64x96 rel mask   14 dv_pre_dropout      40  mfma 20x4x96 drop
   6 o_pre_dropout        7.7  mfma 1x97x64 drop        15 second_fmin    1010193  mfma 20x20x64 causal
   7 dp_no_mult        295329  mfma 1x20x64 mask drop   16 v_korder            31  mfma 1x20x64 mask drop
   8 ds_from_dropped    57638  mfma 1x97x64 drop        17 p_post_dropout   27051  mfma 1x97x64 drop
   9 d_post_dropout      6404  mfma 1x97x64 drop
The long forward stores O alone, in bf16, and its table reaches 1024 keys: one key more or less among
161 or 1024 moves O by less than its rounding (0.006 bounds at 5 x 1024), so there the four forward
mistakes are required to be caught by the table (largest distance: no_fwd_scale 258, extra_key 66 at
64 x 1, last_key_dropped 53 at 33 x 33, v_korder 375), not by each of its cases."""
import math

import pytest
import torch

import attn_ref as ar

KINDS = {
    "plain": ar.Spec(ar.MFMA, 2, 3, 20, 33, 64, None, None, 0.0),
    "dropout": ar.Spec(ar.MFMA, 3, 1, 31, 97, 96, None, None, 0.1),
    "rel_bias_mask": ar.Spec(ar.MFMA, 3, 2, 20, 64, 96, "rel", (64, 1, 40), 0.1),
    "mask_all_padded": ar.Spec(ar.MFMA, 3, 1, 32, 64, 128, None, (64, 0, 1), 0.0),
    "causal_mask_padded_row": ar.Spec(ar.MFMA, 3, 3, 32, 32, 96, "causal", (32, 0, 9), 0.1),
    "valu": ar.Spec(ar.VALU, 1, 3, 48, 40, 64, "rel", (33,), 0.1),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_reference_equals_autograd_in_fp64(kind):
    s = KINDS[kind]
    c = ar.make_case(s)
    q, k, v = (c[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    sc = q @ k.transpose(-1, -2) * c["scale"]
    # the HF way: ONE extended mask, finfo.min where the pair is causal OR its key is padded
    ext = torch.zeros(s.B, 1, s.lq, s.lk, dtype=torch.bool)
    rel = None
    if s.bias:
        causal = c["bias"] <= 0.5 * ar.FMIN
        rel = torch.where(causal, torch.zeros_like(c["bias"]), c["bias"]).double().requires_grad_(True)
        sc = sc + rel
        ext = ext | causal[None].any(1, keepdim=True) if s.bias == "causal" else ext
    if s.lens:
        ext = ext | (c["mask"] == 0)[:, None, None, :]
    p = torch.softmax(sc + ext.double() * ar.FMIN, -1)
    p.retain_grad()
    o = (p * c["mult"].double()) @ v
    o.backward(c["do"].double())
    ref = ar.reference(c)
    ds = p * (p.grad - (p * p.grad).sum(-1, keepdim=True))              # softmax backward of autograd's dP
    want = {"o": o.detach(), "p": p.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad, "ds": ds.detach()}
    for t, w in want.items():
        assert float((ref[t] - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), t
    if rel is not None:                                                  # the bias gradient is the batch sum of dS
        live = ~(c["bias"] <= 0.5 * ar.FMIN)
        assert float(((ref["ds"].sum(0) - rel.grad) * live).abs().max()) <= 1e-12
    if s.lens and 0 in s.lens:                                           # an all-padded sample: uniform rows
        assert torch.equal(ref["p"][s.lens.index(0)], torch.full((s.H, s.lq, s.lk), 1.0 / s.lk, dtype=torch.float64))


def test_fused_row_layout():
    s = KINDS["plain"]
    q = ar.make_case(s)["q"]
    m = ar.rows(q)
    for (b, h, i, e) in ((0, 0, 0, 0), (1, 2, 19, 63), (1, 0, 7, 5)):
        assert m[b * s.lq + i, h * s.dh + e] == q[b, h, i, e]
    assert torch.equal(ar.unrows(m, s.B, s.H, s.lq, s.dh), q)
    assert torch.equal(q.to(torch.bfloat16).float(), q)


def test_tables_cover_what_they_claim():
    sweep = [s for v in ar.SWEEP.values() for s in v]
    assert sorted(ar.SWEEP) == [(dh, nt) for dh in (64, 96, 128) for nt in range(1, 6)]
    for (dh, nt), v in ar.SWEEP.items():
        assert all(s.dh == dh and (s.lk + 31) // 32 == nt for s in v) and {s.p for s in v} == {0.0, 0.1}
    assert {s.lk for s in sweep} == {1, 4, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160}
    for lq in ar.LQS:                                                    # every lq with a dead second wave
        assert {(s.B, s.H) for s in sweep if s.lq == lq and s.lk <= 64} >= {(3, 1), (1, 3)}
    assert sum((s.B, s.H) == (2, 2) for s in sweep) == 2
    assert {s.lk for s in ar.BIAS if s.bias == "rel" and not s.lens} == {4, 33, 64, 68, 157}
    assert all(s.lk <= 64 for s in ar.BIAS if s.lens)
    assert {s.lq for s in ar.VALU_CASES} >= {33, 48, 64} and {s.lk for s in ar.VALU_CASES} >= {1, 40, 64}
    assert {s.dh for s in ar.VALU_CASES} == {8, 64, 96}
    assert {(s.lq, s.lk) for s in ar.LONG_CASES} == {(33, 33), (64, 1), (1, 161), (20, 100), (70, 97), (5, 1024)}


def test_yardsticks_are_of_rounding_size():
    for path in (ar.MFMA, ar.VALU, ar.LONG):
        y = ar.yardstick(path)
        print(path, {t: f"{e:.2e}" for t, e in y.items()})
        for t, e in y.items():
            if t in ("p", "ds"):
                assert 2.0 ** -26 <= e < 1e-4, (path, t, e)              # a handful of fp32 roundings
            else:
                assert 2.0 ** -10 <= e < 2.0 ** -6, (path, t, e)         # bf16 operands and outputs
            assert ar.bound(path, t) == 4 * e


def test_every_mistake_sits_5_bounds_away():
    assert len(ar.MISTAKES) == 17
    for n, wrong in enumerate(ar.MISTAKES, 1):
        d = [(ar.distance(s, wrong), ar.name(s)) for path in (ar.MFMA, ar.VALU) for s in ar.table(path)
             if ar.applies(wrong, s)]
        assert len(d) >= 2, wrong
        print(f"{n:2d} {wrong:18s} least {min(d)[0]:10.1f} bounds at {min(d)[1]} ({len(d)} cases)")
        assert min(d)[0] >= 5, (wrong, min(d))
    for wrong in ("no_fwd_scale", "extra_key", "last_key_dropped", "v_korder"):
        d = [(ar.distance(s, wrong), ar.name(s)) for s in ar.LONG_CASES if ar.applies(wrong, s)]
        print(f"long {wrong:18s} least {min(d)[0]:.3g} at {min(d)[1]}, most {max(d)[0]:.1f} at {max(d)[1]}")
        assert max(d)[0] >= 5, (wrong, max(d))


def test_applies_excludes_only_unchanged_cases():
    """applies() may exclude a case only where the mistake changes nothing there."""
    for path in (ar.MFMA, ar.VALU):
        for s in ar.table(path):
            for wrong in ar.MISTAKES:
                if not ar.applies(wrong, s) and wrong not in ("bias_T", "v_korder"):
                    assert ar.distance(s, wrong) < 1e-6, (wrong, ar.name(s))
    assert math.isinf(ar.rel_err(torch.tensor([math.nan]), torch.zeros(1, dtype=torch.float64), torch.ones(1)))
