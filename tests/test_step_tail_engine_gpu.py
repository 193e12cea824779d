"""The graph step's shorter tail (the id sort beside the T5 backward, the scatter beside the trailing
weight gradients, one vqa_grad_sqnorm_final launch, the inputs in one vqa_copy_multi launch)
against the eager step (vqa_embedding_bwd, three squared-norm launches, vqa_optim_finalize, the
dense embedding update, one copy per input): three steps, every result bit for bit."""
import pytest

pytestmark = pytest.mark.gpu
# 64: the smallest image size this suite runs the stem at
B, L, H = 4, 8, 64
STATE = ("P32", "M", "V", "VMAX", "P16", "opt_state")


@pytest.fixture(scope="module")
def eager_run(pkg):
    """Three eager steps of the plain engine: its per-step loss and log-probs, its final state."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sd = pkg.synthetic.make_state_dict("resnet18", seed=0)
    batches = [pkg.synthetic.make_batch(B, L, H, seed=20 + i) for i in range(4)]
    ref = pkg.engine.VQAEngine(sd, vision="resnet18", batch=B, seq_len=L, image_size=H, warmup=2, total=20,
                               dropout=0.1, seed=0)
    steps = []
    for nb in batches[:3]:
        ref.load_batch(nb)                                   # host arrays: one copy per buffer
        ref.train_step()
        steps.append((ref.LOSS.clone(), ref.LOGP.clone()))
    ref.flush_optimizer()
    torch.cuda.synchronize()
    state = {n: getattr(ref, n).clone() for n in STATE}
    assert [c.name for c in ref.opt_calls[:4]] == ["vqa_grad_sqnorm"] * 3 + ["vqa_optim_finalize"]
    del ref
    return sd, batches, steps, state


@pytest.mark.parametrize("pipeline", [False, True])
def test_graph_step_with_the_short_tail_equals_the_eager_step(pkg, eager_run, pipeline):
    import torch
    sd, batches, steps, state = eager_run
    dev = [{k: torch.as_tensor(v).cuda() for k, v in nb.items() if v is not None} for nb in batches]
    eng = pkg.engine.VQAEngine(sd, vision="resnet18", batch=B, seq_len=L, image_size=H, warmup=2, total=20,
                               dropout=0.1, seed=0, pipeline=pipeline)
    assert eng.fused_tail
    assert [c.name for c in eng.tail_calls] == ["vqa_grad_sqnorm_final", "vqa_adamw_amsgrad", "vqa_adamw_rows"]
    assert [c.name for c in eng.tail_calls_unfused[:2]] == ["vqa_grad_sqnorm", "vqa_optim_finalize"]
    for c in (eng.tail_calls[0], eng.emb_sort_call, eng.emb_scatter_call):
        assert not pkg.ops.uncovered_pointers(c), c.name
    if pipeline:
        eng.prime(dev[0]["image_tensors"])
        eng.F4.copy_(eng.F4N)
        eng.load_batch(dev[0], next_images=dev[1]["image_tensors"])
    else:
        eng.load_batch(dev[0])
    eng.capture()
    if pipeline:
        eng.prime(dev[0]["image_tensors"])
    for i in range(3):
        if pipeline:
            eng.load_batch(dev[i], next_images=dev[i + 1]["image_tensors"])   # device batches: one launch
        else:
            eng.load_batch(dev[i])
        eng.train_step()
        loss, logp = steps[i]
        assert torch.equal(eng.LOSS, loss) and torch.equal(eng.LOGP, logp), i
    eng.flush_optimizer()
    torch.cuda.synchronize()
    assert not bool(eng.SQ_CNT.any())
    for n in STATE:
        assert torch.equal(getattr(eng, n), state[n]), n
    assert torch.isfinite(eng.P32).all()
