"""A/B of the evaluation epoch: the replayed evaluation graph against the eager paths.

  python tools/eval_ab.py [OUT.txt] [--batch 64] [--image 224] [--seq 32] [--batches 20] [--rounds 5]

On one model (R50, t5-base, the benched shape by default) and the same device-resident
batches, alternated a / b / c for `--rounds` rounds in one process after a warm-up round:
  a  VQATrainer.evaluate(use_graph=True)    one graph replay per batch, one host read per epoch
  b  VQATrainer.evaluate(use_graph=False)   the same calls issued eagerly
  c  VQATrainer.valid_one_epoch             the eager forward, float(loss) and argmax(exp) per batch
Host clock around each epoch, ending in a device synchronise; ms per batch, per round, with the
spread (max - min) over the rounds.  Also: the kernel-node count of the evaluation graph and the
time of vqa_eval_rows alone (device events around 200 launches) at 64 x 170 and 1024 x 1024.
The committed result is profiles/eval_graph_ab.txt."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


def kernel_nodes(pkg, graph):
    hip = pkg.lib.hip_runtime()
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), nodes, ctypes.byref(n)) == 0
    kinds = {}
    for i in range(n.value):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t)) == 0
        kinds[t.value] = kinds.get(t.value, 0) + 1
    return kinds                                        # type 0 = kernel


def time_eval_rows(pkg, batch, answers, k, reps=200):
    g = torch.Generator().manual_seed(0)
    lp = torch.log_softmax(torch.randn(batch, answers, generator=g), -1).cuda()
    tgt = torch.randint(0, answers, (batch,), generator=g).cuda()
    nll, loss = torch.rand(batch).cuda(), torch.rand(1).cuda()
    sim = torch.rand(answers, answers).cuda()
    idx = torch.empty(batch, k, dtype=torch.int32, device="cuda")
    val = torch.empty(batch, k, device="cuda")
    cap = batch * (reps + 8)
    buf = torch.zeros(16 + 2 * cap, dtype=torch.int32, device="cuda")
    d = pkg.lib.EvalDesc()
    d.logp, d.targets, d.nll, d.loss, d.similarity = (t.data_ptr() for t in (lp, tgt, nll, loss, sim))
    d.batch, d.answers, d.k = batch, answers, k
    d.topk_idx, d.topk_logp, d.acc = idx.data_ptr(), val.data_ptr(), buf.data_ptr()
    d.pred_log, d.tgt_log, d.capacity = buf.data_ptr() + 64, buf.data_ptr() + 64 + 4 * cap, cap
    call = pkg.ops.Call("vqa_eval_rows", ctypes.byref(d), keep=(lp, tgt, nll, loss, sim, idx, val, buf), desc=d)
    s = pkg.lib.stream_handle()
    for _ in range(8):
        call(s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        call(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps             # us per call (both launches)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    B, H, Lq = arg("--batch", 64), arg("--image", 224), arg("--seq", 32)
    nb, rounds = arg("--batches", 20), arg("--rounds", 5)
    if not torch.cuda.is_available():
        raise SystemExit("eval_ab: needs a GPU (nothing is timed without one)")
    pkg = load_package()
    m = pkg.model.ResnetVQAModel("resnet50", "t5-base", 170, device="cuda", batch_size=B, seq_len=Lq, image_size=H,
                                 dropout=0.1)
    tr = pkg.trainer.VQATrainer(m, {"kwargs": {"weight_decay": 0.1}}, {"num_warmup_steps": 2}, num_training_steps=100,
                                logger=None)
    e = m.engine
    batches = [{k: (torch.as_tensor(v).cuda() if v is not None else None)
                for k, v in pkg.synthetic.make_batch(B, Lq, H, seed=1 + i).items()} for i in range(nb)]
    m.load_items(batches[0])
    e.forward()
    e.backward()
    table = os.path.join(ROOT, "t5-resnet-vqa_amd", "tuning", "gemm_gfx950.json")
    e.autotune(table=table if os.path.exists(table) else None)
    sim = np.random.RandomState(0).rand(170, 170).astype(np.float32)
    e._keep_graph = True                                # keep the hipGraph_t so its nodes can be counted
    e.eval_capture(topk=5, similarity=sim)
    kinds = kernel_nodes(pkg, e.eval_graph)
    paths = {"a": lambda: tr.evaluate(batches, topk=5, similarity=sim, use_graph=True),
             "b": lambda: tr.evaluate(batches, topk=5, similarity=sim, use_graph=False),
             "c": lambda: tr.valid_one_epoch(batches)}
    res = {k: [] for k in paths}
    got = {}
    for r in range(rounds + 1):                         # round 0 warms every path up
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[name] = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3 / nb
            if r:
                res[name].append(dt)
    assert got["a"] == got["b"], "graph and eager evaluation disagree"
    same_c = got["a"]["predictions"] == got["c"]["predictions"] and got["a"]["avg_loss"] == got["c"]["avg_loss"]
    lines = [f"evaluation epoch A/B: resnet50 + t5-base, B {B}, {H}x{H}, L {Lq}, {nb} batches, {rounds} rounds "
             f"after one warm-up round, alternated a/b/c in one process ({torch.cuda.get_device_name(0)})",
             "ms per batch (host clock around the epoch, ending in a device synchronise):"]
    names = {"a": "a evaluate(use_graph=True) ", "b": "b evaluate(use_graph=False)", "c": "c valid_one_epoch          "}
    for k, v in res.items():
        lines.append(f"  {names[k]}  rounds {' '.join(f'{x:.3f}' for x in v)}  median {float(np.median(v)):.3f}  "
                     f"spread {max(v) - min(v):.3f}")
    ma, mc = float(np.median(res["a"])), float(np.median(res["c"]))
    sc = max(res["c"]) - min(res["c"])
    lines.append(f"a - c = {ma - mc:+.3f} ms per batch (c's round-to-round spread: {sc:.3f})")
    lines.append(f"a == b (whole result dict): True; a's predictions and avg_loss == c's: {same_c}")
    lines.append(f"evaluation graph nodes by hipGraphNodeType: {dict(sorted(kinds.items()))} (0 = kernel)")
    for (b_, a_, k_) in ((64, 170, 5), (1024, 1024, 5), (1024, 1024, 16)):
        lines.append(f"vqa_eval_rows alone, {b_} x {a_}, k {k_}, accumulators + table + log: "
                     f"{time_eval_rows(pkg, b_, a_, k_):.2f} us per call (device events, 200 calls)")
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
