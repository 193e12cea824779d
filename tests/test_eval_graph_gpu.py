"""The evaluation graph (engine.eval_capture / eval_step, model.predict, trainer.evaluate):
a replayed forward-only graph ending in vqa_eval_rows.  Every comparison is exact.

* it computes what the eager eval-mode forward computes (a twin model built from the same
  seed), batch by batch, a short last batch included, and its metrics are the ones numpy
  derives from the eager log-probs;
* an evaluation between two training steps leaves the training run as it is: same losses,
  parameters and dropout RNG state as the run without it (the reference's model.eval()
  forward draws no random numbers, trainer/faster_rcnn_vqa_trainer.py:408-430);
* a deferred AdamW update is applied before the evaluation reads the weights;
* the fuse_norm and ResNet-18 engines, and the refusal of pipelined ones."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
B, L, H, A = 4, 16, 64, 170


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _items(pkg, torch, rows, seed):
    nb = pkg.synthetic.make_batch(rows, L, H, seed=seed)
    return {k: (torch.as_tensor(v).cuda() if v is not None else None) for k, v in nb.items()}


def _model(pkg):
    return pkg.model.ResnetVQAModel("resnet50", "t5-base", A, device="cuda", batch_size=B, seq_len=L, image_size=H,
                                    dropout=0.1)


def _trainer(pkg, m):
    return pkg.trainer.VQATrainer(m, {"kwargs": {"weight_decay": 0.1}}, {"num_warmup_steps": 2},
                                  num_training_steps=20, logger=None)


def _eager(m, items):
    """model.eval(); model(**batch) -> (log-probs, loss) on the host."""
    m.eval()
    lp, loss = m(**items)
    return lp.cpu().numpy(), loss.cpu().numpy()


@pytest.fixture(scope="module")
def batches(torch_cuda, pkg):
    return [_items(pkg, torch_cuda, B, 1), _items(pkg, torch_cuda, B, 2), _items(pkg, torch_cuda, 3, 3)]


@pytest.fixture(scope="module")
def eager(torch_cuda, pkg, batches):
    """The eager eval-mode forward of every batch, on a twin model (computed once)."""
    twin = _model(pkg)
    out = [_eager(twin, it) for it in batches]
    del twin
    return out


def test_graph_equals_eager_forward_and_numpy_metrics(torch_cuda, pkg, batches, eager):
    torch = torch_cuda
    m = _model(pkg)
    tr = _trainer(pkg, m)
    e = m.engine
    assert m.training
    for it, (lp, loss) in zip(batches, eager):
        idx, top = m.predict(it["question_input_ids"], it["question_attention_masks"], it["image_tensors"],
                             it["annotation_ids"], topk=5)
        n = lp.shape[0]
        assert idx.shape == (n, 5) and idx.dtype == torch.int64 and top.dtype == torch.float32
        got = e.LOGP[:n].cpu().numpy()
        assert got.tobytes() == lp.tobytes()
        assert e.LOSS[0].cpu().numpy().tobytes() == loss.tobytes()
        np.testing.assert_array_equal(idx[:, 0].cpu().numpy(), np.argmax(lp, 1))
        order = np.argsort(-lp, kind="stable")[:, :5]
        np.testing.assert_array_equal(idx.cpu().numpy(), order)
        assert top.cpu().numpy().tobytes() == np.take_along_axis(lp, order, 1).tobytes()
    assert int(e.RNG[2].item()) == 1                       # the training flag came back
    sim = np.random.RandomState(5).rand(A, A).astype(np.float32)
    r = tr.evaluate(batches, topk=5, similarity=sim)
    assert m.training
    tgt = np.concatenate([it["annotation_ids"].cpu().numpy() for it in batches])
    lps = np.concatenate([lp for lp, _ in eager])
    order = np.argsort(-lps, kind="stable")[:, :5]
    loss_sum = np.float64(0.0)
    for _, loss in eager:
        loss_sum = loss_sum + np.float64(loss)
    nll_sum, sim_sum = np.float64(0.0), np.float64(0.0)
    for b in range(len(tgt)):
        nll_sum = nll_sum + np.float64(-lps[b, tgt[b]])
        sim_sum = sim_sum + np.float64(sim[order[b, 0], tgt[b]])
    assert (r["rows"], r["steps"]) == (11, 3)
    assert r["avg_loss"] == float(loss_sum / 3)
    assert r["targets"] == tgt.tolist() and r["predictions"] == order[:, 0].tolist()
    assert r["accuracy"] == float((order[:, 0] == tgt).sum()) / 11
    assert r["topk_accuracy"] == float((order == tgt[:, None]).any(1).sum()) / 11
    assert r["wups"] == float(sim_sum / 11)
    assert r["sample_loss"] == float(nll_sum / 11)          # the head's nll is -(logit - lse) = -log-prob
    assert tr.evaluate(batches, topk=5, similarity=sim) == r
    eagerly = tr.evaluate(batches, topk=5, similarity=sim, use_graph=False)
    assert eagerly == r


def _sample(e):
    e.flush_optimizer()
    return e.P32[::9973].cpu().numpy().copy(), e.RNG.cpu().numpy().copy()


def test_evaluation_leaves_training_untouched(torch_cuda, pkg, batches):
    torch = torch_cuda
    a, b = _model(pkg), _model(pkg)
    ta, tb = _trainer(pkg, a), _trainer(pkg, b)
    la = [ta.train_one_step(batches[0])[0], ta.train_one_step(batches[1])[0]]
    lb = [tb.train_one_step(batches[0])[0]]
    r = tb.evaluate([batches[2], batches[1]], topk=3)
    assert r["rows"] == 7 and b.training
    lb.append(tb.train_one_step(batches[1])[0])
    assert b.engine.graph is not None and b.engine.eval_graph is not None     # the two graphs coexist
    assert la == lb
    assert torch.equal(a.engine.LOGP, b.engine.LOGP)
    (pa, ra), (pb, rb) = _sample(a.engine), _sample(b.engine)
    assert pa.tobytes() == pb.tobytes()
    np.testing.assert_array_equal(ra, rb)


def test_deferred_update_is_visible(torch_cuda, pkg, batches, eager):
    c, d = _model(pkg), _model(pkg)
    tc, td = _trainer(pkg, c), _trainer(pkg, d)
    # two steps: the warm-up schedule's first update has learning rate 0, so the weights the
    # second step's forward used are the initial ones (`first`: batch 1 at those weights), and
    # the update pending after it is the first that moves them
    first = eager[1][0]
    for t in (tc, td):
        t.train_one_step(batches[0])
        t.train_one_step(batches[2])
    assert c.engine.defer_opt                               # the update is pending after the step
    tc.evaluate([batches[1]])
    d.engine.flush_optimizer()
    lp, loss = _eager(d, batches[1])
    assert c.engine.LOGP.cpu().numpy().tobytes() == lp.tobytes()
    assert c.engine.LOSS[0].cpu().numpy().tobytes() == loss.tobytes()
    assert lp.tobytes() != first.tobytes()                  # the pending update was applied, not skipped


@pytest.mark.parametrize("vision,kw", [("resnet50", dict(fuse_norm=True)), ("resnet18", {})])
def test_engine_variants(torch_cuda, pkg, vision, kw):
    torch = torch_cuda
    sd = pkg.synthetic.make_state_dict(vision, seed=0)
    eng = pkg.engine.VQAEngine(sd, vision=vision, batch=B, seq_len=L, image_size=H, dropout=0.1, seed=0, **kw)
    nb = pkg.synthetic.make_batch(B, L, H, seed=1)
    eng.load_batch(nb)
    eng.set_training(False)
    eng.forward()                                           # the eager eval-mode forward
    lp, loss = eng.LOGP.clone(), eng.LOSS.clone()
    eng.set_training(True)
    rng = eng.RNG.clone()
    eng.LOGP.zero_()
    eng.LOSS.zero_()
    eng.eval_capture(topk=3)
    eng.eval_step()
    assert torch.equal(eng.LOGP, lp) and torch.equal(eng.LOSS, loss)
    assert torch.equal(eng.RNG, rng)                        # no dropout draw, the flag restored
    r = eng.eval_result()
    assert (r["steps"], r["rows"], r["cursor"]) == (1, B, B)
    assert r["predictions"] == lp.argmax(1).tolist() and r["targets"] == nb["annotation_ids"].tolist()
    assert r["loss_sum"] == float(loss.double().item())
    eng.eval_reset()
    assert eng.eval_result()["rows"] == 0


def test_pipelined_engine_refuses(torch_cuda, pkg):
    sd = pkg.synthetic.make_state_dict("resnet50", seed=0)
    eng = pkg.engine.VQAEngine(sd, vision="resnet50", batch=B, seq_len=L, image_size=H, dropout=0.1, seed=0,
                               pipeline=True)
    with pytest.raises(ValueError, match="pipelin"):
        eng.eval_capture()
    assert eng.eval_graph is None
