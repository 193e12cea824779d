"""Two measurements for FasterRcnnVQAModel (device events, warm-up, then the median; needs a GPU):

  python tools/frcnn_step.py [OUT.json] [--batch 64] [--image 256] [--seq 16] [--steps 30] [--rounds 5]

  step  the captured training step (dropout 0.1, pipeline off, GEMM tiles by vqa_gemm_select's
        heuristics -- neither model is tuned here and the faster-rcnn GEMM shapes have no entry in
        tuning/gemm_gfx950.json) of vision "faster-rcnn" and, in the same process, order and
        settings, "resnet50": `rounds` windows of `steps` graph replays each, the two models
        alternated, ms per step
  cam   vqa_channel_cam against the torch expression it replaces on the same device tensor
        (NHWC bf16 -> permute + float + mean over channels + per-image min / max normalisation),
        at the ResNet-50 map of 224^2 (B x 49 x 2048) and the FPN pool map of 256^2 (B x 16 x 256):
        windows of 50 calls, alternated, us per call, issued eagerly (host launch cost included)
        and as 50 calls replayed from a captured graph

The committed result is profiles/frcnn_step.json."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


def window(fn, n):
    """ms per call of n calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "windows": len(v)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    if not torch.cuda.is_available():
        raise SystemExit("frcnn_step: needs a GPU (nothing is timed without one)")
    B, H, Lq = arg("--batch", 64), arg("--image", 256), arg("--seq", 16)
    steps, rounds = arg("--steps", 30), arg("--rounds", 5)
    pkg = load_package()
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "image_size": H, "seq_len": Lq,
           "settings": "captured step, dropout 0.1, pipeline off, untuned (vqa_gemm_select heuristics)"}
    engines = {}
    for vision in ("faster-rcnn", "resnet50"):
        sd = pkg.synthetic.make_state_dict(vision, seed=0)
        eng = pkg.engine.VQAEngine(sd, vision=vision, batch=B, seq_len=Lq, image_size=H, warmup=10, total=100000,
                                   dropout=0.1)
        nb = pkg.synthetic.make_batch(B, Lq, H, seed=1)
        eng.load_batch({k: (torch.as_tensor(v).cuda() if v is not None else None) for k, v in nb.items()})
        eng.capture()
        for _ in range(5):
            eng.train_step()
        torch.cuda.synchronize()
        engines[vision] = eng
        del sd
    t = {v: [] for v in engines}
    for _ in range(rounds):                             # alternated
        for v, eng in engines.items():
            t[v].append(window(eng.train_step, steps))
    res["step_ms"] = {v: dict(stats(x), vision_tokens=engines[v].fh ** 2, vision_calls=len(engines[v].res_calls))
                      for v, x in t.items()}
    assert all(np.isfinite(float(e.LOSS.item())) for e in engines.values())
    engines.clear()

    L_ = pkg.lib
    res["cam_us"] = {}
    for P, C in ((49, 2048), (16, 256)):
        g = torch.Generator().manual_seed(P)
        x = torch.randn(B, P, C, generator=g).abs().to(torch.bfloat16).cuda()
        heat, mean = torch.empty(B, P, device="cuda"), torch.empty(B, P, device="cuda")
        cnt = torch.zeros(B * L_.CAM_COUNTER_STRIDE, dtype=torch.int32, device="cuda")
        keep = {}

        def kernel():
            L_.call("vqa_channel_cam", x.data_ptr(), B, P, C, mean.data_ptr(), heat.data_ptr(), cnt.data_ptr())

        def expr():
            cam = x.permute(0, 2, 1).float().mean(1)
            mn, mx = cam.amin(1, keepdim=True), cam.amax(1, keepdim=True)
            keep["h"] = (cam - mn) / (mx - mn)
        for fn in (kernel, expr) * 3:
            fn()
        torch.cuda.synchronize()
        tk, te = [], []
        for _ in range(rounds):
            tk.append(window(kernel, 50) * 1e3)
            te.append(window(expr, 50) * 1e3)
        # the same 50 calls replayed from a captured graph (no host launch cost: what the kernel
        # costs inside the evaluation graph)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graphs = []
        for fn in (lambda: L_.call("vqa_channel_cam", x.data_ptr(), B, P, C, mean.data_ptr(), heat.data_ptr(),
                                   cnt.data_ptr(), stream=side), expr):
            g_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_, stream=side):
                for _ in range(50):
                    fn()
            g_.replay()
            graphs.append(g_)
        torch.cuda.synchronize()
        gk, ge = [], []
        for _ in range(rounds):
            gk.append(window(graphs[0].replay, 1) * 1e3 / 50)
            ge.append(window(graphs[1].replay, 1) * 1e3 / 50)
        res["cam_us"][f"{B}x{P}x{C}"] = {
            "vqa_channel_cam": stats(tk), "torch_expression": stats(te), "input_mb": B * P * C * 2 / 1e6,
            "vqa_channel_cam_graph": stats(gk), "torch_expression_graph": stats(ge),
            "max_abs_difference": float((heat - keep["h"]).abs().max())}
    txt = json.dumps(res, indent=1, sort_keys=True)
    print(txt)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
