"""Micro-benchmark of the ViT attention rollout at the benched shape (B 64, 224^2: 197 tokens,
12 layers x 12 heads x 64), on random bf16 q | k | v rows laid out as the engine's (ld 2304):

  python tools/rollout_micro.py [OUT.txt] [--batch 64] [--reps 20]

  a  the existing path: 12 x vqa_attn_probs into [12, B, 12, 197, 197] fp32 (1.43 GB at B 64), then
     the script's rollout by torch on the device (head mean, + I, row-normalise, 11 batched
     matrix products, row 0)
  b  12 x vqa_attn_headmean into [12, B, 197, 200] fp32 (121 MB) + 1 x vqa_rollout_cls

Device events around each whole pass, a / b alternated in one process after 3 warm-up passes each,
median and spread of `--reps` passes; a's two halves are also timed on their own.  The committed
result is profiles/vit_rollout_micro.txt."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

LAYERS, H, DH, N, LD = 12, 12, 64, 197, 200


def arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


def timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    B, reps = arg("--batch", 64), arg("--reps", 20)
    if not torch.cuda.is_available():
        raise SystemExit("rollout_micro: needs a GPU (nothing is timed without one)")
    pkg = load_package()
    L_, ops = pkg.lib, pkg.ops
    D = H * DH
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(LAYERS, B * N, 3 * D, generator=g).to(torch.bfloat16).cuda()
    att = torch.empty(LAYERS, B, H, N, N, device="cuda")
    aug = torch.zeros(LAYERS, B, N, LD, device="cuda")
    mask, unit = torch.empty(B, N - 1, device="cuda"), torch.empty(B, N - 1, device="cuda")
    probs, means = [], []
    for i in range(LAYERS):
        for lst, name in ((probs, "vqa_attn_probs"), (means, "vqa_attn_headmean")):
            d = L_.AttnDesc()
            d.q, d.ldq, d.k, d.ldk = ops.addr(qkv[i]), 3 * D, ops.addr(qkv[i], D), 3 * D
            d.batch, d.heads, d.lq, d.lk, d.dh, d.scale = B, H, N, N, DH, DH ** -0.5
            if name == "vqa_attn_probs":
                d.p = ops.addr(att[i])
                lst.append(ops.Call(name, ctypes.byref(d), desc=d, keep=(qkv, att)))
            else:
                lst.append(ops.Call(name, ctypes.byref(d), ops.addr(aug[i]), LD, desc=d, keep=(qkv, aug)))
    chain = ops.Call("vqa_rollout_cls", ops.addr(aug), LAYERS, B, N, LD, B * N * LD, ops.addr(mask), ops.addr(unit),
                     keep=(aug, mask, unit))
    eye = torch.eye(N, device="cuda")
    res = {}

    def a_probs():
        s = L_.stream_handle()
        for c in probs:
            c(s)

    def a_torch():
        j = None
        for i in range(LAYERS):
            m = att[i].mean(1) + eye
            m = m / m.sum(-1, keepdim=True)
            j = m if j is None else m @ j
        r = j[:, 0, 1:]
        res["a"] = r / r.amax(1, keepdim=True)

    def a():
        a_probs()
        a_torch()

    def b():
        s = L_.stream_handle()
        for c in means:
            c(s)
        chain(s)

    for fn in (a, b) * 3:
        fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):                               # alternated
        ta += timed(a, 1)
        tb += timed(b, 1)
    tp, tt = timed(a_probs, reps), timed(a_torch, reps)
    agree = float(((unit - res["a"]).abs().amax(1)).max())
    st = lambda v: f"median {float(np.median(v)):.3f} ms  min {min(v):.3f}  max {max(v):.3f}"   # noqa: E731
    lines = [f"ViT attention rollout, B {B}, {N} tokens, {LAYERS} layers x {H} heads x {DH}, {reps} passes each after 3 "
             f"warm-up passes, a / b alternated, device events around a whole pass ({torch.cuda.get_device_name(0)})",
             f"  a  12 x vqa_attn_probs + torch rollout   {st(ta)}",
             f"       12 x vqa_attn_probs alone           {st(tp)}",
             f"       torch rollout alone                 {st(tt)}",
             f"  b  12 x vqa_attn_headmean + vqa_rollout_cls  {st(tb)}",
             f"a / b = {float(np.median(ta)) / float(np.median(tb)):.1f}x; buffers: a {att.numel() * 4 / 1e9:.2f} GB, "
             f"b {aug.numel() * 4 / 1e6:.0f} MB (arithmetic, not a measurement)",
             f"max |a - b| of the maximum-normalised masks: {agree:.3e}"]
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
