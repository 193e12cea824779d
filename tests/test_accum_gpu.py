"""Gradient accumulation on the GPU: k micro-batches of B rows and one optimizer step
(engine.use_accumulation / accum_step, VQATrainer(accumulation_steps=k)) must train like one
engine planned for k x B rows -- data parallelism laid out in time, so the shapes and bounds are
those of the two-rank DP tests (tests/test_a_dp2_gpu.py): B 4, L 32, H 64, warmup 1, total 20,
dropout 0, three steps on make_batch(k B, L, H, seed=40 + i).  The oracle is always one
VQAEngine(batch=k B) (or one trainer on it) on the same rows, never the code under test; it is
computed once per (k B, rows) and shared."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
B, L, H, STEPS = 4, 32, 64, 3
KW = dict(seq_len=L, image_size=H, warmup=1, total=20)
_REF = {}


@pytest.fixture(scope="module")
def torch_():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.fixture(scope="module")
def sd(pkg):
    return pkg.synthetic.make_state_dict("resnet50", seed=0)


def _batches(pkg, torch, rows, steps=STEPS + 1):
    return [{k: torch.as_tensor(v).cuda() for k, v in pkg.synthetic.make_batch(rows, L, H, seed=40 + i).items()
             if v is not None} for i in range(steps)]


def _reference(pkg, torch, sd, planned, rows):
    """One engine planned for `planned` rows on `rows`-row batches (padded): losses, clip norms
    and the final parameters.  Computed once, never changed."""
    key = (planned, rows)
    if key not in _REF:
        ref = pkg.engine.VQAEngine(sd, batch=planned, dropout=0.0, **KW)
        loss, norm = [], []
        for b in _batches(pkg, torch, rows, STEPS):
            ref.load_batch(b)
            ref.train_step()
            torch.cuda.synchronize()
            loss.append(float(ref.LOSS.item()))
            norm.append(ref.last_grad_norm())
        ref.flush_optimizer()
        _REF[key] = (np.array(loss), np.array(norm), ref.P32.cpu().numpy(), ref.lay.pack(sd))
        del ref
    return _REF[key]


def _accum_run(pkg, torch, sd, k, rows, pipe=False, graph=True, **ekw):
    eng = pkg.engine.VQAEngine(sd, batch=B, dropout=0.0, pipeline=pipe, **KW, **ekw)
    eng.use_accumulation(k)
    bs = _batches(pkg, torch, rows)
    if pipe:
        eng.prime(bs[0]["image_tensors"][:B])
    loss, norm = [], []
    for i in range(STEPS):
        eng.accum_step(bs[i], next_images=bs[i + 1]["image_tensors"][:B] if pipe else None, use_graph=graph)
        torch.cuda.synchronize()
        loss.append(float(eng.LOSS.item()))
        norm.append(eng.last_grad_norm())
        assert eng.accum_log_probs().shape == (rows, eng.A)
        assert int(eng.ACC[2].item()) == 0, "the finish resets the micro-batch counter"
    eng.flush_optimizer()
    torch.cuda.synchronize()
    return eng, np.array(loss), np.array(norm), eng.P32.cpu().numpy()


def _check(parity_report, name, got, ref):
    """The DP tests' comparison and bounds (tests/test_a_dp2_gpu.py), every figure recorded first."""
    (loss, norm, p), (gloss, gnorm, p_ref, p0) = got, ref
    dloss = np.abs(loss - gloss) / np.abs(gloss)
    dnorm = np.abs(norm - gnorm) / gnorm
    upd = float(np.linalg.norm(p.astype(np.float64) - p_ref) / np.linalg.norm(p_ref.astype(np.float64) - p0))
    parity_report[name] = {"loss_rel": dloss.tolist(), "grad_norm_rel": dnorm.tolist(), "update_rel_l2": upd}
    print(name, parity_report[name])
    assert dloss[0] <= 1e-5 and dnorm[0] <= 1e-4, (dloss, dnorm)
    assert (dloss <= 2e-3).all() and (dnorm <= 2e-2).all(), (dloss, dnorm)
    assert upd <= 5e-2, upd


@pytest.mark.parametrize("k,pipe,graph", [(2, False, True), (2, True, True), (2, False, False), (4, False, True)])
def test_accum_matches_global_batch(pkg, torch_, sd, parity_report, k, pipe, graph):
    eng, loss, norm, p = _accum_run(pkg, torch_, sd, k, k * B, pipe, graph)
    assert float(eng.opt_state[pkg.lib.ST_STEP].item()) == STEPS, "one optimizer step per accumulated step"
    _check(parity_report, f"accum_k{k}_pipe{int(pipe)}_graph{int(graph)}", (loss, norm, p),
           _reference(pkg, torch_, sd, k * B, k * B))


@pytest.mark.parametrize("rows", [5, 4])
def test_accum_unequal_rows(pkg, torch_, sd, parity_report, rows):
    """Global batches of 5 and 4 rows at k = 2, B = 4: micro-batches (4, 1) and (4, 0), against the
    batch-8 engine on the same rows, padded.  The empty micro-batch: loss share 0, zero gradient."""
    eng, loss, norm, p = _accum_run(pkg, torch_, sd, 2, rows)
    if rows == B:
        # one more step, watched: the empty micro-batch runs last, and its loss share and its whole
        # gradient arena G32 are exactly zero
        shares = []
        eng.accum_step(_batches(pkg, torch_, rows)[0], on_micro=lambda j: shares.append(eng.LOSS.clone()))
        torch_.cuda.synchronize()
        assert float(shares[1].item()) == 0.0
        assert int(torch_.count_nonzero(eng.G32).item()) == 0
    _check(parity_report, f"accum_k2_rows{rows}", (loss, norm, p), _reference(pkg, torch_, sd, 2 * B, rows))


def test_accumulator_is_the_fp32_sum(pkg, torch_, sd):
    """Eager micro-steps, G32 copied after each: GACC equals their fp32 sum in micro order, bit for
    bit, over the whole arena (k = 3: a copy and two adds)."""
    torch = torch_
    eng = pkg.engine.VQAEngine(sd, batch=B, dropout=0.0, **KW)
    eng.use_accumulation(3)
    parts = []
    eng.accum_step(_batches(pkg, torch, 3 * B, 1)[0], use_graph=False, on_micro=lambda j: parts.append(eng.G32.clone()))
    torch.cuda.synchronize()
    assert len(parts) == 3
    want = parts[0].clone()
    want += parts[1]
    want += parts[2]
    assert torch.equal(eng.GACC.view(torch.int32), want.view(torch.int32))
    name = "t5.embed"
    assert torch.equal(eng.segment_grad(name, accumulated=True),
                       want[eng.lay[name].offset:eng.lay[name].offset + eng.lay[name].numel].view(eng.lay[name].shape))


def _disjoint_batch(pkg, torch, step):
    """8 rows whose token ids are pairwise distinct and disjoint from every other step's: 4 rows x
    32 tokens per micro-batch from an id range of its own."""
    b = pkg.synthetic.make_batch(2 * B, L, H, seed=70 + step, full_length=True)
    for j in range(2):
        base = 100 + (2 * step + j) * 200
        b["question_input_ids"][j * B:(j + 1) * B] = base + np.arange(B * L).reshape(B, L)
    return {k: torch.as_tensor(v).cuda() for k, v in b.items() if v is not None}


def test_disjoint_ids_no_stale_rows(pkg, torch_, sd):
    """Three accumulated steps with pairwise disjoint token ids.  After each, the accumulated table
    gradient is exactly zero outside that step's rows.  Every table row the step did not touch --
    the rows of step s - 1 among them -- gets the zero-gradient update: starting step s from the
    accumulating engine's own state, the batch-8 engine leaves those rows of P32, M, V and VMAX
    with the same bits (its untouched-row behaviour: the moments decay, no stale gradient)."""
    torch = torch_
    acc = pkg.engine.VQAEngine(sd, batch=B, dropout=0.0, **KW)
    acc.use_accumulation(2)
    ref = pkg.engine.VQAEngine(sd, batch=2 * B, dropout=0.0, **KW)
    emb = acc.lay["t5.embed"]
    tab = slice(emb.offset, emb.offset + emb.numel)
    D = emb.shape[1]
    for s in range(3):
        b = _disjoint_batch(pkg, torch, s)
        for e in (acc, ref):
            e.flush_optimizer()
        for name in ("P32", "P16", "M", "V", "VMAX", "opt_state"):
            getattr(ref, name).copy_(getattr(acc, name))
        acc.accum_step(b)
        ref.load_batch(b)
        ref.train_step()
        for e in (acc, ref):
            e.flush_optimizer()
        torch.cuda.synchronize()
        touched = torch.zeros(emb.shape[0], dtype=torch.bool, device="cuda")
        touched[b["question_input_ids"].reshape(-1)] = True
        assert int(touched.sum()) == 2 * B * L
        g = acc.segment_grad("t5.embed", accumulated=True)
        assert int(torch.count_nonzero(g[~touched]).item()) == 0, "accumulated table gradient outside the step's rows"
        assert bool((g[touched] != 0).any(dim=1).all()), "a touched row has no gradient"
        for name in ("P32", "M", "V", "VMAX"):
            a = getattr(acc, name)[tab].view(-1, D)[~touched]
            r = getattr(ref, name)[tab].view(-1, D)[~touched]
            assert torch.equal(a.view(torch.int32), r.view(torch.int32)), (s, name)
        if s > 0:                                        # step s - 1's rows are among them, and moved
            prev = torch.zeros_like(touched)
            prev[_disjoint_batch(pkg, torch, s - 1)["question_input_ids"].reshape(-1)] = True
            assert bool((prev & ~touched).sum() == 2 * B * L)
            assert bool((acc.M[tab].view(-1, D)[prev] != 0).any())


def test_update_applied_once(pkg, torch_, sd):
    """k forward replays apply the deferred AdamW ranges once: the same three steps with
    defer_optimizer=False (the whole AdamW pass in the finish graph) end with the same bits."""
    torch = torch_
    e1, l1, n1, p1 = _accum_run(pkg, torch, sd, 2, 2 * B)
    assert float(e1.opt_state[pkg.lib.ST_STEP].item()) == STEPS
    del e1
    e2, l2, n2, p2 = _accum_run(pkg, torch, sd, 2, 2 * B, defer_optimizer=False)
    assert float(e2.opt_state[pkg.lib.ST_STEP].item()) == STEPS
    assert np.array_equal(l1, l2) and np.array_equal(n1, n2)
    assert np.array_equal(p1.view(np.int32), p2.view(np.int32))


def test_deterministic_with_dropout(pkg, torch_, sd):
    torch = torch_
    runs = []
    for _ in range(2):
        eng = pkg.engine.VQAEngine(sd, batch=B, dropout=0.1, seed=3, **KW)
        eng.use_accumulation(2)
        loss, norm = [], []
        for b in _batches(pkg, torch, 2 * B, STEPS):
            eng.accum_step(b)
            loss.append(eng.LOSS.clone())
            norm.append(eng.opt_state[pkg.lib.ST_GRAD_NORM].clone())
        eng.flush_optimizer()
        torch.cuda.synchronize()
        runs.append((eng.P32.clone(), torch.cat(loss), torch.stack(norm), eng.RNG.clone()))
        del eng
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # each micro-batch drew fresh masks: 2 draws per optimizer step
    assert int(runs[0][3][1].item()) == 2 * STEPS


def test_k1_is_todays_step(pkg, torch_, sd):
    torch = torch_
    out = []
    for use in (True, False):
        eng = pkg.engine.VQAEngine(sd, batch=B, dropout=0.1, **KW)
        if use:
            eng.use_accumulation(1)
            assert eng.GACC is None and eng.accum == 1 and eng.count_call is None
        eng.capture()
        for b in _batches(pkg, torch, B, 2):
            eng.load_batch(b)
            eng.train_step()
        eng.flush_optimizer()
        torch.cuda.synchronize()
        out.append(eng.P32.clone())
        del eng
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))


def test_use_accumulation_refusals(pkg, torch_, sd):
    eng = pkg.engine.VQAEngine(sd, batch=B, dropout=0.0, **KW)
    with pytest.raises(ValueError):
        eng.use_accumulation(0)
    with pytest.raises(ValueError):
        eng.use_accumulation(257)                           # k x B > 1024 rows
    with pytest.raises(RuntimeError):
        eng.accum_step(_batches(pkg, torch_, B, 1)[0])      # not set up
    eng.use_accumulation(2)
    eng.use_accumulation(2)
    with pytest.raises(ValueError):
        eng.use_accumulation(3)
    with pytest.raises(RuntimeError):
        eng.train_step()
    with pytest.raises(ValueError):
        eng.accum_step(_batches(pkg, torch_, 2 * B + 1, 1)[0])


# ------------------------------------------------------------------ trainer
def _dp_worker():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import dp_worker
    return dp_worker


def _accum_trainer(pkg, sd, dropout=0.0):
    w = _dp_worker()
    model = pkg.model.ResnetVQAModel("resnet50", "t5-base", 170, batch_size=B, seq_len=L, image_size=H,
                                     state_dict=sd, dropout=dropout, device="cuda:0")
    return model, pkg.trainer.VQATrainer(model, logger=None, accumulation_steps=2, **w.TRAINER_KW)


def test_trainer_refusals_before_device_work(pkg):
    w = _dp_worker()
    resnet = object.__new__(pkg.model.ResnetVQAModel)       # never built: no engine, no device work
    vit = object.__new__(pkg.model.VitVQAModel)
    with pytest.raises(ValueError):
        pkg.trainer.VQATrainer(resnet, accumulation_steps=0, **w.TRAINER_KW)
    with pytest.raises(ValueError):
        pkg.trainer.VQATrainer(resnet, accumulation_steps=2, data_parallel=True, **w.TRAINER_KW)
    with pytest.raises(ValueError):
        pkg.trainer.VQATrainer(vit, accumulation_steps=2, data_parallel=False, **w.TRAINER_KW)


def test_trainer_accumulation_matches_batch8_trainer(pkg, torch_, sd, parity_report):
    torch = torch_
    w = _dp_worker()
    gb = _batches(pkg, torch, 2 * B, STEPS)
    ref = w.trainer_run(pkg, sd, 2 * B, L, H, gb, STEPS, True, data_parallel=False)
    model, tr = _accum_trainer(pkg, sd)
    loss, norm = [], []
    for b in gb:
        ls, lp = tr.train_one_step(b)
        assert lp.shape == (2 * B, 170)
        loss.append(ls)
        norm.append(tr.grad_norm())
    assert tr.scheduler_state_dict()["last_epoch"] == STEPS
    model.engine.flush_optimizer()
    torch.cuda.synchronize()
    p0 = pkg.layout.ParamLayout("resnet50").pack(sd)
    _check(parity_report, "accum_trainer_k2", (np.array(loss), np.array(norm), model.engine.P32.cpu().numpy()),
           (ref["losses"], ref["norms"], ref["p32"], p0))
    # a short last batch: 7 of the 8 rows
    short = {k: v[:7] for k, v in gb[0].items()}
    ls, lp = tr.train_one_step(short)
    assert lp.shape == (7, 170) and np.isfinite(ls) and bool(torch.isfinite(lp).all())
    with pytest.raises(ValueError):
        tr.train_one_step({k: torch.cat([v, v[:1]]) for k, v in gb[0].items()})      # 9 rows
    # the paths between accumulated steps work unchanged
    vloss, vlp = tr.valid_one_step({k: v[:B] for k, v in gb[1].items()})
    assert np.isfinite(vloss) and vlp.shape == (B, 170)
    assert np.isfinite(tr.grad_norm())


def test_trainer_checkpoint_resumes_bitwise(pkg, torch_, sd, tmp_path):
    torch = torch_
    gb = _batches(pkg, torch, 2 * B, STEPS)
    m, tr = _accum_trainer(pkg, sd, dropout=0.1)
    for b in gb[:2]:
        tr.train_one_step(b)
    torch.save(m.state_dict(), tmp_path / "model.pt")
    tr.save_state_dict_checkpoint(tmp_path / "ckpt.pt", epoch=1)
    want_loss = tr.train_one_step(gb[2])[0]
    want = m.state_dict()
    del m, tr
    m2, tr2 = _accum_trainer(pkg, torch.load(tmp_path / "model.pt", weights_only=True), dropout=0.1)
    assert tr2.load_state_dict_checkpoint(tmp_path / "ckpt.pt") == 1
    assert tr2.scheduler_state_dict()["last_epoch"] == 2
    assert tr2.train_one_step(gb[2])[0] == want_loss
    got = m2.state_dict()
    for k in want:
        assert torch.equal(got[k], want[k]), k
