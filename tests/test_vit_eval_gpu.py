"""Config 4's inference side (VitVQAModel.predict / attention_rollout, VQATrainer.evaluate on
VitVQAEngine): the replayed evaluation graph computes exactly what the eager eval-mode forward
computes, leaves a training run untouched, and carries the attention rollout of the frozen ViT
(vqa_attn_headmean per layer + vqa_rollout_cls) in place of the [12, B, 12, 197, 197] maps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, L, LD, A = 2, 16, 12, 170
OKW = {"type": "AdamW", "lm_encoder_lr": 1e-4, "classifier_lr": 1e-4, "kwargs": {"weight_decay": 0.1, "amsgrad": True}}


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def sd(pkg):
    return pkg.vit_model.make_state_dict(seed=0)


def _items(pkg, rows, seed, image=224):
    nb = pkg.vit_model.make_batch(rows, L, dec_len=LD, image=image, seed=seed)
    return {k: (torch.as_tensor(v).cuda() if v is not None else None) for k, v in nb.items()}


def _model(pkg, sd, image=224):
    return pkg.model.VitVQAModel(answer_spaces=A, batch_size=B, seq_len=L, dec_len=LD, image_size=image,
                                 state_dict=sd, dropout=0.1)


def _trainer(pkg, m):
    return pkg.trainer.VQATrainer(m, OKW, {"num_warmup_steps": 2}, num_training_steps=20, logger=None)


def _predict(m, it, **kw):
    return m.predict(it["question_input_ids"], it["decoder_question_input_ids"], it["question_attention_masks"],
                     it["decoder_question_attention_masks"], it["pixel_values"], it["annotation_ids"], **kw)


@pytest.fixture(scope="module")
def batches(cuda, pkg):
    return [_items(pkg, 2, 1), _items(pkg, 2, 2), _items(pkg, 1, 3)]


@pytest.fixture(scope="module")
def eager(cuda, pkg, sd, batches):
    """The eager eval-mode forward of every batch on a twin model: (log-probs, loss), computed once."""
    twin = _model(pkg, sd)
    twin.eval()
    out = []
    for it in batches:
        lp, loss = twin(**it)
        out.append((lp.cpu().numpy(), loss.cpu().numpy()))
    del twin
    return out


def _check_predict(m, it, lp, loss, idx, top):
    e = m.engine
    n = lp.shape[0]
    assert idx.shape == (n, 5) and idx.dtype == torch.int64 and top.dtype == torch.float32
    assert e.LOGP[:n].cpu().numpy().tobytes() == lp.tobytes()
    assert e.LOSS[0].cpu().numpy().tobytes() == loss.tobytes()
    order = np.argsort(-lp, kind="stable")[:, :5]
    np.testing.assert_array_equal(idx.cpu().numpy(), order)
    assert top.cpu().numpy().tobytes() == np.take_along_axis(lp, order, 1).tobytes()


def test_graph_equals_eager_forward_and_numpy_metrics(cuda, pkg, sd, batches, eager):
    m = _model(pkg, sd)
    tr = _trainer(pkg, m)
    e = m.engine
    assert m.training
    rng = e.RNG.clone()
    for it, (lp, loss) in zip(batches, eager):
        idx, top = _predict(m, it, topk=5)
        _check_predict(m, it, lp, loss, idx, top)
    assert torch.equal(e.RNG, rng)                          # no dropout draw, the training flag came back
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
    assert (r["rows"], r["steps"]) == (5, 3)
    assert r["avg_loss"] == float(loss_sum / 3)
    assert r["targets"] == tgt.tolist() and r["predictions"] == order[:, 0].tolist()
    assert r["accuracy"] == float((order[:, 0] == tgt).sum()) / 5
    assert r["topk_accuracy"] == float((order == tgt[:, None]).any(1).sum()) / 5
    assert r["wups"] == float(sim_sum / 5)
    assert r["sample_loss"] == float(nll_sum / 5)
    assert tr.evaluate(batches, topk=5, similarity=sim) == r
    assert tr.evaluate(batches, topk=5, similarity=sim, use_graph=False) == r


def _sample(e):
    return e.P32[::9973].cpu().numpy().copy(), e.RNG.cpu().numpy().copy()


def test_evaluation_leaves_training_untouched(cuda, pkg, sd, batches):
    a, b = _model(pkg, sd), _model(pkg, sd)
    ta, tb = _trainer(pkg, a), _trainer(pkg, b)
    la = [ta.train_one_step(batches[0])[0], ta.train_one_step(batches[1])[0]]
    lb = [tb.train_one_step(batches[0])[0]]
    r = tb.evaluate([batches[2], batches[1]], topk=3)
    assert r["rows"] == 3 and b.training
    lb.append(tb.train_one_step(batches[1])[0])
    assert b.engine.graph is not None and b.engine.eval_graph is not None     # the two graphs coexist
    assert la == lb
    assert torch.equal(a.engine.LOGP, b.engine.LOGP)
    (pa, ra), (pb, rb) = _sample(a.engine), _sample(b.engine)
    assert pa.tobytes() == pb.tobytes()
    np.testing.assert_array_equal(ra, rb)


def _torch_rollout(att, dtype):
    """The script's rollout (ViT_vqa_heatmap.py:104-137) from generate_answers' attention tensors
    (12 x [n, 12, T, T]) in `dtype` on the device: [n, T - 1]."""
    t = att[0].shape[-1]
    eye = torch.eye(t, dtype=dtype, device=att[0].device)
    j = None
    for a in att:
        m = a.to(dtype).mean(1) + eye
        m = m / m.sum(-1, keepdim=True)
        j = m if j is None else m @ j
    return j[:, 0, 1:]


def _rel(x, ref):
    return float(((x.double() - ref.double()).abs().amax(1) / ref.double().amax(1)).max())


def test_rollout_in_the_engine(cuda, pkg, sd, batches, parity_report):
    """predict(rollout=True) (the graph) and attention_rollout() (eager) against the existing path:
    the rollout by torch from the same model's generate_answers attention tensors (the same bf16
    q | k).  The fp64 rollout of those tensors is the reference; the bound is test_rollout_chain's
    rule, 4 x the error of the same rollout done by torch in fp32."""
    m = _model(pkg, sd)
    m.eval()
    rec = {}
    for name, it in (("rows2", batches[0]), ("rows1", batches[2])):
        n = it["question_input_ids"].shape[0]
        idx, top, mask = _predict(m, it, topk=5, rollout=True)
        assert mask.shape == (n, 14, 14) and mask.dtype == torch.float32 and idx.shape == (n, 5)
        eager = m.attention_rollout(**it)
        assert eager.shape == (n, 14, 14)
        assert torch.equal(mask.view(torch.int32), eager.view(torch.int32))      # graph == eager, exactly
        unit = m.attention_rollout(**it, normalize=True)
        assert unit.flatten(1).amax(1).tolist() == [1.0] * n
        assert torch.equal(unit, eager / eager.flatten(1).amax(1)[:, None, None])
        _, _, att = m.generate_answers(**it)
        ref = _torch_rollout(att, torch.float64)
        e_ref = _rel(_torch_rollout(att, torch.float32), ref)
        err = _rel(mask.flatten(1), ref)
        print(f"engine rollout {name}: kernels {err:.3e}, torch fp32 from the maps {e_ref:.3e}")
        rec[name] = {"kernels": err, "torch_fp32": e_ref}
        assert err <= 4 * e_ref, (name, err, e_ref)
        if n == 2:                                          # distance to the fp32 oracle's rollout: recorded only
            from oracle import vit_oracle as vo
            tsd = {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in sd.items() if k.startswith("vision_model.")}
            oatt = []
            with torch.no_grad():
                vo.vit_pooled(tsd, it["pixel_values"].float().cpu(), attentions=oatt)
            rec["vs_fp32_oracle"] = _rel(mask.flatten(1).cpu(), _torch_rollout(oatt, torch.float64))
    parity_report["vit_engine_rollout_rel"] = rec


def test_rollout_follows_the_image_size(cuda, pkg, sd):
    """image_size 96: 37 tokens, a 6 x 6 map -- the token count is the engine's, not a literal 197."""
    vm = pkg.vit_model
    sd96 = dict(sd)
    for k, shape in vm.model_specs(A, 96).items():
        if tuple(np.shape(sd96[k])) != tuple(shape):
            sd96[k] = vm.init_param(k, shape, 0)
    m = _model(pkg, sd96, image=96)
    m.eval()
    it = _items(pkg, 2, 4, image=96)
    _, _, mask = _predict(m, it, rollout=True)
    assert mask.shape == (2, 6, 6)
    assert torch.equal(mask, m.attention_rollout(**it))
    _, _, att = m.generate_answers(**it)
    assert att[0].shape == (2, 12, 37, 37)
    ref = _torch_rollout(att, torch.float64)
    e_ref = _rel(_torch_rollout(att, torch.float32), ref)
    err = _rel(mask.flatten(1), ref)
    print(f"engine rollout 96^2: kernels {err:.3e}, torch fp32 from the maps {e_ref:.3e}")
    assert err <= 4 * e_ref, (err, e_ref)


def test_switching_rollout_replans(cuda, pkg, sd, batches, eager):
    m = _model(pkg, sd)
    e = m.engine
    it, (lp, loss) = batches[0], eager[0]
    idx, top, mask = _predict(m, it, rollout=True)
    g1 = e.eval_graph
    assert e.eval_rollout and g1 is not None
    _check_predict(m, it, lp, loss, idx, top)               # the rollout's calls change nothing else
    idx, top = _predict(m, it)
    assert not e.eval_rollout and e.eval_graph is not None and e.eval_graph is not g1
    _check_predict(m, it, lp, loss, idx, top)
    g2 = e.eval_graph
    _predict(m, it)
    assert e.eval_graph is g2                               # same plan: the graph is kept
    out = _predict(m, it, rollout=True)
    assert len(out) == 3 and e.eval_graph is not g2 and torch.equal(out[2], mask)
