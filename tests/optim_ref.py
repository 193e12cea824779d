"""Plain numpy restatement of the optimiser tail (csrc/optim.hip, csrc/adamw.h), written from
include/vqa_hip.h and the formulas of torch.optim.AdamW(amsgrad=True), clip_grad_norm_ and
get_linear_schedule_with_warmup -- not from the kernels.  Every function takes a dtype: float64 is
the reference of tests/test_optim_parity_gpu.py, float32 the yardstick (what an equally long fp32
evaluation of the same formulas loses against fp64).

Hyper-parameters.  The descriptor carries betas, eps, weight decay and LRs as C floats, so the
reference uses exactly those fp32 values widened to double: b2 = float32(0.999), 1 - b2 formed in
the working dtype, bias corrections from that b2.  torch, given the Python double 0.999, multiplies
by float32(0.999) too but adds with float32(0.001); against that, 1.f - b2 is 1.3e-5 low, a property
of the float descriptor that tests/test_optim_ref_cpu.py measures.

Normalisers, each from the reference alone (err_* below):
  m, v, vmax  element-wise relative, the denominator floored at STATE_FLOOR x the tensor's max |ref|
              (an element that small is judged as if it were that large: v spans twelve decades
              in the inputs here, m cancels to nearly nothing where 0.9 m meets -0.1 g).
  p           element-wise, relative to |p_before| + the reference's sum over the steps of |update|
              (`travel`; one step: |p_ref - p_before|), floored at P_FLOOR x that sum's max.  fp32 rounds the decay product and the final subtraction at |p| and the
              update's own chain at |update|, so an honest evaluation errs by about an ulp of that
              sum, while a wrong update shows as its share of it -- not hidden behind p, which at
              real weight size (0.02 randn) is of the updates' own size.

Bound = max(FACTOR x yardstick, FLOOR), the yardstick measured on the CPU on the very inputs the
GPU test uses (yardstick_dense / yardstick_multi / yardstick_rows); nothing of a kernel enters it.

`wrong=` applies one deliberate mistake (WRONG lists them); tests/test_optim_ref_cpu.py measures
with it how far a wrong kernel would sit from the reference.  No wrong kernel is ever run."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
FLOOR = 2.0 ** -22                             # no bound is below a quarter ulp of the normaliser
FACTOR = 4.0                                   # bound = FACTOR * yardstick
STATE_FLOOR = 2.0 ** -4                        # m, v, vmax: denominator >= this x max |ref|
P_FLOOR = 2.0 ** -6                            # p: denominator >= this x max (|p| + |update|)

# what the engines put into the descriptor, as the C floats it carries
B1, B2, EPS, WD = F32(0.9), F32(0.999), F32(1e-8), F32(0.1)
CLIP_EPS = 1e-6                                # clip_grad_norm_'s

# the dense case of the GPU test: 4 x 256 + 37 float4s, group ends in float4 units
N4 = 4 * 256 + 37
ENDS4 = {1: (N4,), 7: (1, 255, 257, 300, 301, 700, N4), 8: (1, 255, 257, 300, 301, 700, 900, N4)}
LRS = (F32(1e-4), F32(5e-4), F32(2e-3), F32(5e-3), F32(2e-2), F32(1e-3), F32(1e-2), F32(3e-3))
DENSE = dict(step=7, warmup=2, total=10, grad_scale=0.5, max_norm=1.0)       # lam 3/8, clip active
MULTI = dict(steps=6, warmup=2, total=5, grad_scale=0.5, max_norm=1.0)       # lam 0, 1/2, 1, 2/3, 1/3, 0
ROWS_CASES = ((37, 4), (37, 64), (37, 768), (37, 772), (37, 1024), (300, 64))
ROWS_SCHED = dict(step=3, warmup=10, total=100, grad_scale=1.0, max_norm=1.0)

WRONG = (
    "v_for_vmax",            # denominator from v instead of the running max
    "t_is_step",             # t = step instead of step + 1 in the bias corrections
    "bc2_no_sqrt",           # bc2 used without its square root
    "eps_before_div",        # (sqrt(vmax) + eps) / sqrt(bc2)
    "eps_in_sqrt",           # sqrt(vmax + eps) / sqrt(bc2)
    "coupled_wd",            # weight decay added to the gradient
    "decay_no_lam",          # decay p (1 - lr wd) with the LR not multiplied by lam
    "no_coef",               # clip coefficient not applied
    "norm_no_gscale",        # grad_scale missing from the norm
    "grad_no_gscale",        # grad_scale missing from the gradient
    "gscale_twice",          # grad_scale applied twice to the gradient
    "lam_next",              # lam taken at step + 1
    "decay_over_total",      # decay phase divided by total instead of total - warmup
    "boundary_gt",           # group boundary compared with > instead of >=
    "boundary_elems",        # float4 index compared with the ends in elements
    "boundary_neighbour",    # the float4 at boundary `which` given its lower neighbour's LR
)
SCHEDULE_WRONG = ("t_is_step", "lam_next", "decay_over_total")
BOUNDARY_WRONG = ("boundary_gt", "boundary_elems", "boundary_neighbour")


def sqnorm(g):
    """Sum of squares of g, squared and summed in fp64."""
    g = np.asarray(g, F64).ravel()
    return float(np.dot(g, g))


def lr_lambda(step, warmup, total, wrong=None):
    """get_linear_schedule_with_warmup's multiplier at scheduler step `step`."""
    if wrong == "lam_next":
        step = step + 1
    if step < warmup:
        return step / max(1, warmup)
    return max(0.0, (total - step) / max(1, total if wrong == "decay_over_total" else total - warmup))


def finalize(ss, step, grad_scale, max_norm, warmup, total, b1=B1, b2=B2, dtype=F64, wrong=None):
    """The step's scalars from the sum of squares ss (fp64) at step counter `step` (the number of
    updates applied so far): norm = sqrt(ss) grad_scale, coef = min(1, max_norm / (norm + 1e-6))
    (1 when max_norm <= 0), lam, bc1 = 1 - b1^t and sqrt(bc2) = sqrt(1 - b2^t) with t = step + 1."""
    T = dtype
    gs = T(1.0) if wrong == "norm_no_gscale" else T(grad_scale)
    norm = T(np.sqrt(F64(ss))) * gs
    coef = T(1.0)
    if max_norm > 0:
        with np.errstate(invalid="ignore"):
            coef = min(T(1.0), T(max_norm) / (norm + T(CLIP_EPS)))
    # lam and the bias corrections are formed in double in either dtype and then rounded to it:
    # 1 - b2^t cancels (at t = 8 an fp32 evaluation is ~125 ulps off), and the state block is
    # documented to hold the fp32 roundings of the double values
    t = F64(step if wrong == "t_is_step" else step + 1)
    lam = lr_lambda(step, warmup, total, wrong)
    bc1 = 1.0 - F64(b1) ** t
    bc2s = np.sqrt(1.0 - F64(b2) ** t)
    return dict(norm=norm, coef=coef, lam=T(lam), bc1=T(bc1), bc2s=T(bc2s))


def group_lrs(n, ends, lrs, wrong=None, which=0):
    """[n] per-element LR: element e is of group #{k < ngroups - 1 : e >= ends[k]}.  `ends` are the
    exclusive ends in ELEMENTS (multiples of 4) and may be negative or beyond n, as in a window of a
    larger range; the last group runs to the end whatever its entry says."""
    ends = [int(e) for e in ends]
    assert all(e % 4 == 0 for e in ends) and n % 4 == 0
    i4 = np.arange(n // 4)
    gi = np.zeros(n // 4, np.int64)
    for k in range(len(ends) - 1):
        if wrong == "boundary_gt":
            gi += i4 > ends[k] // 4
        elif wrong == "boundary_elems":
            gi += i4 >= ends[k]
        else:
            gi += i4 >= ends[k] // 4
    if wrong == "boundary_neighbour":
        b = ends[which] // 4
        if 0 < b < n // 4:
            gi[b] = gi[b - 1]
    return np.repeat(np.asarray(lrs, F32)[gi], 4)


def adamw(p, g, m, v, vm, ends, lrs, sc, grad_scale, b1=B1, b2=B2, eps=EPS, wd=WD, dtype=F64, wrong=None, which=0,
          one_minus=None):
    """One AdamW-amsgrad update with the scalars sc of finalize(): returns new (p, m, v, vmax).
    g' = g grad_scale coef;  p <- p (1 - lr lam wd);  m <- lerp(m, g', 1 - b1);
    v <- b2 v + (1 - b2) g'^2;  vmax <- max(vmax, v);  denom = sqrt(vmax) / sqrt(bc2) + eps;
    p <- p - lr lam / bc1 * m / denom.  one_minus = (1 - b1, 1 - b2) given as constants of their
    own instead of formed from b1, b2 (TORCH_CONSTS: what torch does with Python doubles)."""
    T = dtype
    p, g, m, v, vm = (np.asarray(a).astype(T).ravel() for a in (p, g, m, v, vm))
    b1, b2, eps, wd = T(b1), T(b2), T(eps), T(wd)
    lr0 = group_lrs(p.size, ends, lrs, wrong, which).astype(T)
    lr = lr0 * T(sc["lam"])
    gs = {"grad_no_gscale": T(1.0), "gscale_twice": T(grad_scale) * T(grad_scale)}.get(wrong, T(grad_scale))
    gr = g * (gs if wrong == "no_coef" else gs * T(sc["coef"]))
    if wrong == "coupled_wd":
        gr = gr + wd * p
    else:
        p = p * (T(1.0) - (lr0 if wrong == "decay_no_lam" else lr) * wd)
    omb1, omb2 = (T(1.0) - b1, T(1.0) - b2) if one_minus is None else (T(one_minus[0]), T(one_minus[1]))
    m = m + omb1 * (gr - m)
    v = v * b2 + omb2 * gr * gr
    vm = np.maximum(vm, v)
    root, bc2s = np.sqrt(v if wrong == "v_for_vmax" else vm), T(sc["bc2s"])
    if wrong == "bc2_no_sqrt":
        denom = root / (bc2s * bc2s) + eps
    elif wrong == "eps_before_div":
        denom = (root + eps) / bc2s
    elif wrong == "eps_in_sqrt":
        denom = np.sqrt((v if wrong == "v_for_vmax" else vm) + eps) / bc2s
    else:
        denom = root / bc2s + eps
    p = p - lr / T(sc["bc1"]) * (m / denom)
    return p, m, v, vm


def bf16_rne(x):
    """The bf16 round-to-nearest-even of finite fp32 values, as uint16 bit patterns."""
    u = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# torch.optim.AdamW(betas=(0.9, 0.999)) on fp32 tensors: mul_(beta2) rounds 0.999 to fp32 as the
# descriptor does, but lerp's weight and addcmul's value are the DOUBLES 1 - 0.9 and 1 - 0.999 rounded
# to fp32, and the bias corrections come from the doubles 0.9 / 0.999
TORCH_CONSTS = dict(one_minus=(F32(1 - 0.9), F32(1 - 0.999)), bc_betas=(0.9, 0.999))


def step(state, g, ends, lrs, grad_scale, max_norm, warmup, total, dtype=F64, wrong=None, which=0, consts=None):
    """One whole step of the chain on state = dict(p, m, v, vm, step): clip norm over g, scalars,
    update.  Returns the new state (arrays of `dtype`, step + 1) and the scalars."""
    bb = consts["bc_betas"] if consts else (B1, B2)
    sc = finalize(sqnorm(g), state["step"], grad_scale, max_norm, warmup, total, bb[0], bb[1], dtype=dtype, wrong=wrong)
    p, m, v, vm = adamw(state["p"], g, state["m"], state["v"], state["vm"], ends, lrs, sc, grad_scale,
                        dtype=dtype, wrong=wrong, which=which, one_minus=consts["one_minus"] if consts else None)
    travel = state.get("travel", 0.0) + np.abs(p.astype(F64) - np.asarray(state["p"], F64).ravel())
    return dict(p=p, m=m, v=v, vm=vm, step=state["step"] + 1, travel=travel), sc


def run(state, grads, ends, lrs, grad_scale, max_norm, warmup, total, dtype=F64, wrong=None, which=0, consts=None):
    """step() over a list of gradients, the state carried in `dtype`: a float64 run carries doubles,
    a float32 run rounds its state to fp32 each step as the device does."""
    for g in grads:
        state, _ = step(state, g, ends, lrs, grad_scale, max_norm, warmup, total, dtype, wrong, which, consts)
    return state


# ------------------------------------------------------------------ errors and bounds
def err_state(got, ref):
    """Largest element-wise relative error of m, v or vmax (denominator floored, see above); inf
    for a result that is not finite."""
    got, ref = np.asarray(got, F64).ravel(), np.asarray(ref, F64).ravel()
    if not np.isfinite(got).all():
        return np.inf
    den = np.maximum(np.abs(ref), max(STATE_FLOOR * float(np.abs(ref).max()), 1e-300))
    return float((np.abs(got - ref) / den).max())


def err_p(got, ref, before, travel):
    """Largest error of p relative to |p_before| + travel (floored, see above)."""
    got, ref, before = (np.asarray(a, F64).ravel() for a in (got, ref, before))
    if not np.isfinite(got).all():
        return np.inf
    den = np.abs(before) + travel
    den = np.maximum(den, max(P_FLOOR * float(den.max()), 1e-300))
    return float((np.abs(got - ref) / den).max())


def errors(got, ref, before):
    """{p, m, v, vm: error} of a state `got` against the fp64 state `ref` of step() / run();
    `before` = the p the procedure started from."""
    out = {k: err_state(got[k], ref[k]) for k in ("m", "v", "vm")}
    out["p"] = err_p(got["p"], ref["p"], before, ref["travel"])
    return out


def bounds(yard):
    return {k: max(FACTOR * y, FLOOR) for k, y in yard.items()}


# ------------------------------------------------------------------ the GPU test's inputs
def _scales(rng, n):
    """Per-element gradient scale: a third each at 1, 1e-3 and 1e-6, so that eps (1e-8) is
    nothing, something and most of the denominator."""
    return np.array([1.0, 1e-3, 1e-6])[rng.integers(0, 3, n)]


def _state_for(rng, s, step):
    """A state a run could have reached by `step`, s = the clipped gradient's per-element size:
    m of that size, v of bc2(step) x its square; vmax well above v on half the elements (v cannot
    reach it), a hair above on the rest (the step's v overtakes it on many of them)."""
    n = s.size
    bc2 = 1.0 - float(B2) ** (step + 1)
    m = 0.5 * s * rng.standard_normal(n)
    v = bc2 * s * s * (rng.standard_normal(n) ** 2 + 0.1)
    far = rng.random(n) < 0.5
    vm = np.where(far, v * (1.0 + 2.0 * np.abs(rng.standard_normal(n))), v * (1.0 + 1e-3 * rng.random(n)))
    return m.astype(F32), v.astype(F32), vm.astype(F32)


def _frozen(d):
    for a in d.values():
        for x in (a if isinstance(a, list) else [a]):
            if isinstance(x, np.ndarray):
                x.flags.writeable = False
    return d


def _sized_case(rng, n, sched, scales, gmask=1.0):
    """p = 0.02 randn (real weight size), g = randn x scales, and a state sized for the clipped
    gradient at sched's step."""
    g = (rng.standard_normal(n) * scales * gmask).astype(F32)
    p = (0.02 * rng.standard_normal(n)).astype(F32)
    sc = finalize(sqnorm(g), sched["step"], sched["grad_scale"], sched["max_norm"], sched["warmup"], sched["total"])
    m, v, vm = _state_for(rng, scales * sched["grad_scale"] * float(sc["coef"]), sched["step"])
    return dict(p=p, g=g, m=m, v=v, vm=vm)


@functools.lru_cache(maxsize=None)
def dense_case(ngroups):
    """The dense single-step case: N4 float4s, ngroups in ENDS4, DENSE's schedule point."""
    rng = np.random.default_rng(7100 + ngroups)
    n = 4 * N4
    c = _sized_case(rng, n, DENSE, _scales(rng, n))
    c.update(ends=tuple(4 * e for e in ENDS4[ngroups]), lrs=LRS[:ngroups] if ngroups > 1 else (LRS[4],))
    return _frozen(c)


def case_ref(c, sched, dtype=F64, wrong=None, which=0):
    """(state after one step, scalars) of a single-step case c at sched."""
    st = dict(p=c["p"], m=c["m"], v=c["v"], vm=c["vm"], step=sched["step"])
    return step(st, c["g"], c["ends"], c["lrs"], sched["grad_scale"], sched["max_norm"], sched["warmup"],
                sched["total"], dtype=dtype, wrong=wrong, which=which)


@functools.lru_cache(maxsize=None)
def multi_case():
    """MULTI: six steps from a zero state over the 7-group layout, a fresh gradient each step,
    every second one 30 x smaller so that the running max holds against a falling v."""
    rng = np.random.default_rng(7200)
    n = 4 * N4
    scales = _scales(rng, n)
    grads = [(rng.standard_normal(n) * scales * (1.0 / 30 if i % 2 else 1.0)).astype(F32) for i in range(MULTI["steps"])]
    z = np.zeros(n, F32)
    return _frozen(dict(p=(0.02 * rng.standard_normal(n)).astype(F32), grads=grads, m=z, v=z.copy(), vm=z.copy(),
                        ends=tuple(4 * e for e in ENDS4[7]), lrs=LRS[:7]))


def multi_ref(dtype=F64, wrong=None, which=0, consts=None):
    c = multi_case()
    st = dict(p=c["p"], m=c["m"], v=c["v"], vm=c["vm"], step=0)
    return run(st, c["grads"], c["ends"], c["lrs"], MULTI["grad_scale"], MULTI["max_norm"], MULTI["warmup"],
               MULTI["total"], dtype=dtype, wrong=wrong, which=which, consts=consts)


ROWS_KINDS = ("some", "none", "all")


@functools.lru_cache(maxsize=None)
def rows_case(rows, cols, kind="some"):
    """A [rows, cols] table at ROWS_SCHED, two groups with the boundary inside a row (cols > 4).
    ids: `some` = about a third of the rows with duplicates, plus -1, rows and rows + 7 (mark
    nothing); `none` = those three only; `all` = every row.  mark0 = the mark array before
    vqa_embed_mark: -1, and step - 2 (stale: counts as untouched) on some untouched rows.  The
    gradient is exactly zero on every row no id names (the row-split update's contract)."""
    rng = np.random.default_rng(7300 + 1000 * ROWS_KINDS.index(kind) + 31 * rows + cols)
    n, step_ = rows * cols, ROWS_SCHED["step"]
    oob = np.array([-1, rows, rows + 7], np.int64)
    if kind == "some":
        hit = rng.permutation(rows)[: max(2, rows // 3)]
        ids = np.concatenate([hit, hit[:3], oob, hit[:1]])
    elif kind == "none":
        ids = oob
    else:
        ids = np.concatenate([np.arange(rows, dtype=np.int64), oob, np.arange(0, rows, 5, dtype=np.int64)])
    ids = ids[rng.permutation(ids.size)].astype(np.int64)
    touched = np.zeros(rows, bool)
    touched[ids[(ids >= 0) & (ids < rows)]] = True
    mark0 = np.full(rows, -1, np.int32)
    stale = (~touched) & (rng.random(rows) < 0.3)
    mark0[stale] = step_ - 2
    c = _sized_case(rng, n, ROWS_SCHED, _scales(rng, n), np.repeat(touched, cols))
    end0 = (rows // 2) * cols + 4 * (cols // 8)
    c.update(ids=ids, mark0=mark0, touched=touched, ends=(end0, n), lrs=(F32(5e-3), F32(1e-4)))
    return _frozen(c)


def _yard(pairs):
    out = dict(p=0.0, m=0.0, v=0.0, vm=0.0)
    for got, ref, before in pairs:
        e = errors(got, ref, before)
        out = {k: max(out[k], e[k]) for k in out}
    return out


@functools.lru_cache(maxsize=None)
def yardstick_dense():
    """fp32 against fp64 evaluation of the dense step, the largest over ngroups 1, 7, 8."""
    cs = [dense_case(ng) for ng in ENDS4]
    return _yard((case_ref(c, DENSE, F32)[0], case_ref(c, DENSE)[0], c["p"]) for c in cs)


@functools.lru_cache(maxsize=None)
def yardstick_multi():
    """fp32 against fp64 evaluation of the whole six-step procedure."""
    return _yard([(multi_ref(F32), multi_ref(), multi_case()["p"])])


@functools.lru_cache(maxsize=None)
def yardstick_rows():
    """fp32 against fp64 evaluation of the table step, the largest over ROWS_CASES x ROWS_KINDS."""
    cs = [rows_case(r, c, k) for r, c in ROWS_CASES for k in ROWS_KINDS]
    return _yard((case_ref(c, ROWS_SCHED, F32)[0], case_ref(c, ROWS_SCHED)[0], c["p"]) for c in cs)




def schedule_table():
    """(warmup, total, step) of the finalize test: every edge of the schedule -- step == warmup,
    step >= total, warmup 0 and 1, total - warmup <= 1 -- and bias corrections at a large step."""
    out = []
    for w, t in ((0, 10), (1, 10), (2, 10), (10, 100), (10, 11), (10, 10)):
        out += [(w, t, s) for s in sorted({0, 1, w - 1, w, w + 1, t - 1, t, t + 5}) if s >= 0]
    return out + [(1000, 200000, s) for s in (699, 999, 1000, 99999)]
