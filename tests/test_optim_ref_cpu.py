"""tests/optim_ref.py is the fp64 reference of tests/test_optim_parity_gpu.py.  Here, on the CPU:
it equals torch.optim.AdamW(amsgrad=True) + clip_grad_norm_ + LambdaLR(lr_lambda) run in float64
with the descriptor's fp32 hyper-parameters; its fp32 yardsticks are of rounding size; and every
mistake of optim_ref.WRONG moves the reference at least 100 times further than the bound the GPU
test allows (4 x yardstick), on the GPU test's own inputs, so that bound separates right from wrong
without a wrong kernel ever being run.

Two figures are put on record here (printed, loosely asserted):
  * tests/test_kernels_gpu.py::test_adamw_amsgrad_matches_torch barely sees amsgrad: on inputs of
    its kind (4 steps from a zero state, randn x 3 gradients) vmax > v on 4.3 % of the elements, by
    at most 0.3 %, and a kernel dividing by sqrt(v) instead of sqrt(vmax) moves p by less than that
    test's rtol 1e-6 / atol 1e-7 on all but 2.6 % of the elements (worst step), by at most 15
    tolerances there -- against 960 000 bounds on the non-zero state of the new dense case.
  * torch's own constants against the float descriptor's: torch multiplies v by float32(0.999) but
    adds with float32(0.001), where the descriptor's 1.f - b2 is 1.3e-5 smaller.  After the six
    steps of the multi-step case v differs by 1.29e-5 (relative, optim_ref.err_state) and p by
    1.1e-7 of |p| + travel (Adam's update is invariant to the scale of v's increments).  A property
    of the float descriptor, not an error of the kernel."""
import numpy as np
import pytest
import torch

import optim_ref as orf
from oracle import vqa_oracle as orc

F32, F64 = np.float32, np.float64


def _torch_run(c, grads, step0, grad_scale, max_norm, warmup, total):
    """torch's chain in float64 on the CPU from the state of case c at step counter step0."""
    ends = [0] + [min(max(e, 0), c["p"].size) for e in c["ends"]]
    ends[-1] = c["p"].size
    params = [torch.tensor(c["p"][a:b], dtype=torch.float64, requires_grad=True) for a, b in zip(ends, ends[1:])]
    opt = torch.optim.AdamW([{"params": [t], "lr": float(lr)} for t, lr in zip(params, c["lrs"])],
                            betas=(float(orf.B1), float(orf.B2)), eps=float(orf.EPS), weight_decay=float(orf.WD),
                            amsgrad=True, foreach=False)
    for t, a, b in zip(params, ends, ends[1:]):
        opt.state[t] = {"step": torch.tensor(float(step0)),
                        "exp_avg": torch.tensor(c["m"][a:b], dtype=torch.float64),
                        "exp_avg_sq": torch.tensor(c["v"][a:b], dtype=torch.float64),
                        "max_exp_avg_sq": torch.tensor(c["vm"][a:b], dtype=torch.float64)}
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: orc.lr_lambda(s + step0, warmup, total))
    norms = []
    for g in grads:
        for t, a, b in zip(params, ends, ends[1:]):
            t.grad = torch.tensor(g[a:b], dtype=torch.float64) * grad_scale      # the DP average
        if max_norm > 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
        sched.step()
    cat = lambda key: torch.cat([opt.state[t][key] for t in params]).numpy()  # noqa: E731
    return dict(p=torch.cat([t.detach() for t in params]).numpy(), m=cat("exp_avg"), v=cat("exp_avg_sq"),
                vm=cat("max_exp_avg_sq")), norms


@pytest.mark.parametrize("max_norm", [1.0, 0.0])
def test_reference_equals_torch_in_fp64(max_norm):
    """Four steps across the warm-up / decay boundary (steps 1, 2 | 3, 4 of warmup 3, total 10), 7
    groups, the non-zero state of the dense case: vmax > v on half the elements, v about to
    overtake on others."""
    c = orf.dense_case(7)
    rng = np.random.default_rng(5)
    grads = [c["g"]] + [(rng.standard_normal(c["g"].size) * (0.3 if i == 1 else 1.0)).astype(F32) for i in range(3)]
    assert 0.4 < np.mean(c["vm"] > 1.01 * c["v"]) < 0.6
    st = dict(p=c["p"], m=c["m"], v=c["v"], vm=c["vm"], step=1)
    first, sc = orf.step(st, grads[0], c["ends"], c["lrs"], 0.5, max_norm, 3, 10)
    if max_norm > 0:                                                   # (unclipped, the gradient is 20 x the state's size)
        assert 0.3 < np.mean(first["v"] > c["vm"]) < 0.7               # ... and overtakes on the others
    ref = orf.run(st, grads, c["ends"], c["lrs"], 0.5, max_norm, 3, 10)
    got, norms = _torch_run(c, grads, 1, 0.5, max_norm, 3, 10)
    if max_norm > 0:
        assert abs(norms[0] - float(sc["norm"])) <= 1e-12 * norms[0] and float(sc["coef"]) < 0.1
    else:
        assert float(sc["coef"]) == 1.0
    for key in ("p", "m", "v", "vm"):
        err = np.abs(got[key] - ref[key]) / np.maximum(np.abs(ref[key]), 1e-300)
        assert float(err.max()) <= 1e-12, (key, float(err.max()))
    assert ref["step"] == 5


def test_lambda_equals_the_oracle_schedule():
    for w, t, s in orf.schedule_table():
        sc = orf.finalize(1.0, s, 1.0, 1.0, w, t)
        assert float(sc["lam"]) == orc.lr_lambda(s, w, t), (w, t, s)
        assert float(sc["bc1"]) == 1.0 - float(orf.B1) ** (s + 1)
    assert [float(orf.finalize(1.0, s, 1.0, 1.0, 2, 5)["lam"]) for s in range(6)] == [0.0, 0.5, 1.0, 2 / 3, 1 / 3, 0.0]


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, 1.0039063, -1.00390625, 3.3895314e38, 1e-40, 0.0], F32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(orf.bf16_rne(x), want)
    r = np.random.default_rng(0).standard_normal(4096).astype(F32)
    assert np.array_equal(orf.bf16_rne(r), torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_yardsticks_are_of_rounding_size():
    for name, y in (("dense", orf.yardstick_dense()), ("multi", orf.yardstick_multi()), ("rows", orf.yardstick_rows())):
        b = orf.bounds(y)
        print("yardstick", name, {k: f"{v:.3e}" for k, v in y.items()}, "bounds", {k: f"{v:.3e}" for k, v in b.items()})
        for key in ("p", "m", "v", "vm"):
            assert 2.0 ** -26 <= y[key] <= 2.0 ** -20, (name, key, y[key])
            assert b[key] == max(4 * y[key], 2.0 ** -22)


def _effect(got, ref, before, bound):
    e = orf.errors(got, ref, before)
    return max(e[k] / bound[k] for k in e)


def _mutant_effects():
    """{(mutant, case): effect in bounds}: the largest of the four tensors' error / bound, as the
    GPU test asserts all four.  Cases: the dense step at 1, 7 and 8 groups and the six-step run.
    Left out: the boundary mistakes at one group (no boundary), and v-for-vmax on the six-step run
    from a zero state, where v never falls more than 0.5 % below its maximum -- the variant the
    non-zero state of the dense case is there for."""
    out = {}
    b_dense, b_multi = orf.bounds(orf.yardstick_dense()), orf.bounds(orf.yardstick_multi())
    for ng in orf.ENDS4:
        c = orf.dense_case(ng)
        ref = orf.case_ref(c, orf.DENSE)[0]
        for w in orf.WRONG:
            if ng == 1 and w in orf.BOUNDARY_WRONG:
                continue
            for which in (range(ng - 1) if w == "boundary_neighbour" else (0,)):
                name = f"{w}[{which}]" if w == "boundary_neighbour" else w
                with np.errstate(all="ignore"):
                    out[(name, f"dense {ng}")] = _effect(orf.case_ref(c, orf.DENSE, wrong=w, which=which)[0], ref, c["p"], b_dense)
    c, ref = orf.multi_case(), orf.multi_ref()
    for w in orf.WRONG:
        if w == "v_for_vmax":
            continue
        for which in (range(6) if w == "boundary_neighbour" else (0,)):
            name = f"{w}[{which}]" if w == "boundary_neighbour" else w
            with np.errstate(all="ignore"):
                out[(name, "multi")] = _effect(orf.multi_ref(wrong=w, which=which), ref, c["p"], b_multi)
    return out


def test_every_mutant_sits_100_bounds_away():
    eff = _mutant_effects()
    assert {n.split("[")[0] for n, _ in eff} == set(orf.WRONG)
    for (name, case), e in sorted(eff.items(), key=lambda kv: kv[1]):
        print(f"{name:24s} {case:8s} {e:.0f} bounds")
    for key, e in eff.items():
        assert e >= 100, (key, e)


def _ulps(a, b):
    """|a - b| in units of the fp32 spacing at b."""
    return abs(float(a) - float(b)) / float(np.spacing(np.abs(F32(b))) if b != 0 else np.spacing(F32(1.0)))


def test_schedule_mutants_show_in_the_finalize_table():
    """The finalize test asserts LR_SCALE, BC1 and BC2_SQRT within 1 fp32 ulp over
    optim_ref.schedule_table(); each schedule mistake is >= 100 ulps off on many of its entries,
    and each edge of the table is where one of them shows."""
    hits = {w: [] for w in orf.SCHEDULE_WRONG}
    for w_, t_, s_ in orf.schedule_table():
        ref = orf.finalize(1.0, s_, 1.0, 1.0, w_, t_)
        for w in orf.SCHEDULE_WRONG:
            with np.errstate(all="ignore"):
                bad = orf.finalize(1.0, s_, 1.0, 1.0, w_, t_, wrong=w)
            far = max(_ulps(bad[k], ref[k]) if np.isfinite(bad[k]) else np.inf for k in ("lam", "bc1", "bc2s"))
            if far >= 100:
                hits[w].append((w_, t_, s_))
    for w, where in hits.items():
        print(w, len(where), "entries >= 100 ulps")
        assert len(where) >= 8, (w, where)
    assert (2, 10, 2) in hits["lam_next"] and (2, 10, 1) in hits["lam_next"]          # step == warmup, and below it
    assert (10, 100, 11) in hits["decay_over_total"] and (1000, 200000, 99999) in hits["decay_over_total"]
    assert (1000, 200000, 699) in hits["t_is_step"]                                    # b2^t still far from 0 there


def test_existing_torch_test_barely_sees_amsgrad():
    """Inputs of the kind of test_adamw_amsgrad_matches_torch (its own are drawn on the GPU): the
    v-for-vmax variant against the reference, in that test's metric."""
    n, ends, lrs = 4160, (1024, 2048, 4160), (F32(1e-3), F32(5e-4), F32(5e-3))
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=g).numpy()
    grads = [(torch.randn(n, generator=g) * 3).numpy() for _ in range(4)]
    z = np.zeros(n, F32)
    ref = bad = dict(p=p0, m=z, v=z, vm=z, step=0)
    worst_share = worst_ratio = sep = 0.0
    for gr in grads:
        ref, _ = orf.step(ref, gr, ends, lrs, 1.0, 1.0, 2, 10)
        bad, _ = orf.step(bad, gr, ends, lrs, 1.0, 1.0, 2, 10, wrong="v_for_vmax")
        ratio = np.abs(bad["p"] - ref["p"]) / (1e-6 * np.abs(ref["p"]) + 1e-7)
        worst_share, worst_ratio = max(worst_share, float(np.mean(ratio > 1))), max(worst_ratio, float(ratio.max()))
        sep = max(sep, float(np.mean(ref["vm"] > ref["v"])))
        assert float((ref["vm"] / np.maximum(ref["v"], 1e-300)).max()) <= 1.0 / float(orf.B2) ** 3 + 1e-12
    print(f"v-for-vmax on the old test's inputs: vmax > v on {sep:.1%}; beyond its tolerance on {worst_share:.2%} "
          f"of the elements, by at most {worst_ratio:.2f} tolerances")
    assert worst_share < 0.05 and worst_ratio < 50


def test_torch_constants_against_the_float_descriptor():
    c, ref = orf.multi_case(), orf.multi_ref()
    e = orf.errors(orf.multi_ref(consts=orf.TORCH_CONSTS), ref, c["p"])
    low = 1.0 - float(F32(1.0) - orf.B2) / float(F32(1 - 0.999))
    print(f"1.f - b2 is {low:.3e} below float32(0.001); after the six steps v differs by {e['v']:.3e}, "
          f"vmax {e['vm']:.3e}, m {e['m']:.3e}, p {e['p']:.3e}")
    assert 1.2e-5 < low < 1.4e-5
    assert 0.5 * low < e["v"] < 1.5 * low and e["p"] < 1e-6
