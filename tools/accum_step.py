"""What gradient accumulation costs and saves at the benched shape (R50 + t5-base + 3 x SGA, B 64,
224^2, L 32, dropout 0.1, pipelined, graph): one process, three engines -- the plain step and
k = 2, 8 micro-batches per optimizer step (engine.use_accumulation) -- timed in alternating
windows of >= 20 optimizer steps, three windows each, with device events.  Also the device-event
time of vqa_grad_accumulate over the whole gradient arena (the add and the micro == 0 copy) and
of the full-range AdamW launch in the same run, each with the GB/s of its algorithmic bytes:
accumulate 12 B / element (two loads, one store), its copy form 8, AdamW 38 (p, g, m, v, vmax
in; p, m, v, vmax and the bf16 shadow out).

  python tools/accum_step.py [--steps 20] [--windows 3] [--k 2 8] [--out profiles/grad_accum_step.json]

Needs a GPU: without one it fails, it does not fall back."""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

B, L, H = 64, 32, 224
HBM_PEAK_GBS = 8000.0                   # MI355X HBM3E, 8 TB/s


def bench_args():
    return types.SimpleNamespace(batch=B, seq_len=L, image_size=H, blocks=3, no_pipeline=False, dp_groups=False,
                                 config5=False, tune_save=None, no_graph=True, shard_optimizer=False, dp_res_split=None,
                                 res_cumask=None,
                                 tune_table=os.path.join(ROOT, "t5-resnet-vqa_amd", "tuning", "gemm_gfx950.json"))


def device_batches(pkg, dev, rows, count, seed):
    return [{k: torch.as_tensor(v).to(dev) for k, v in pkg.synthetic.make_batch(rows, L, H, seed=seed + i).items()
             if v is not None} for i in range(count)]


def window(step, steps, dev):
    """ms per optimizer step over `steps` steps between two device events."""
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        step(i)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def time_call(fn, dev, reps=10, warm=2):
    """Median device-event ms of fn() (one launch) over `reps` launches after `warm`."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20, help="optimizer steps per timed window (>= 20)")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--k", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/accum_step.py: no GPU; this tool measures on the device and has no fallback")
    if a.steps < 20:
        sys.exit("--steps: a timed window is at least 20 optimizer steps")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pkg = load_package()
    Lb = pkg.lib
    args = bench_args()

    # the plain step: bench.py's own engine, tuned and captured
    pool = device_batches(pkg, dev, B, 2, seed=1)
    args.no_graph = False
    plain, _, plain_step = bench.make_step(args, pkg, dev, pool, False, 0, "t5-base")
    runs = {"plain": (1, plain_step)}
    engines = {1: plain}

    for k in a.k:
        args.no_graph = True                              # make_step builds and tunes; accum_step captures
        eng, _, _ = bench.make_step(args, pkg, dev, pool, False, 0, "t5-base")
        eng.use_accumulation(k)
        gpool = device_batches(pkg, dev, k * B, 2, seed=100 * k)
        eng.prime(gpool[0]["image_tensors"][:B])

        def step(i, eng=eng, gpool=gpool):
            eng.accum_step(gpool[i % 2], next_images=gpool[(i + 1) % 2]["image_tensors"][:B])
        runs[f"k{k}"] = (k, step)
        engines[k] = eng

    for name, (k, step) in runs.items():                  # warm-up: capture, first launches
        window(step, 4, dev)
    times = {name: [] for name in runs}
    for _ in range(a.windows):                            # alternating windows in one process
        for name, (k, step) in runs.items():
            times[name].append(window(step, a.steps, dev))
    out = {"shape": {"batch": B, "seq_len": L, "image_size": H, "blocks": 3, "dropout": 0.1, "pipeline": True,
                     "graph": True, "steps_per_window": a.steps, "windows": a.windows},
           "device": torch.cuda.get_device_name(dev), "step": {}}
    for name, (k, _) in runs.items():
        ts = times[name]
        ms = sorted(ts)[len(ts) // 2]
        out["step"][name] = {"micro_batches": k, "ms_per_optimizer_step": ms, "ms_windows": ts,
                             "window_spread_rel": (max(ts) - min(ts)) / ms, "pairs_per_s": k * B / ms * 1e3,
                             "ms_per_micro_batch": ms / k}
    base = out["step"]["plain"]["pairs_per_s"]
    for name in runs:
        out["step"][name]["pairs_per_s_vs_plain"] = out["step"][name]["pairs_per_s"] / base

    # kernels alone, same run: the accumulate over the whole arena and the full-range AdamW launch
    eng = engines[a.k[0]]
    eng.flush_optimizer()
    n = eng.lay.total
    s = Lb.stream_handle()
    micro = torch.zeros(1, dtype=torch.int32, device=dev)
    acc_call = pkg.ops.Call("vqa_grad_accumulate", eng.GACC.data_ptr(), eng.G32.data_ptr(), n, micro.data_ptr(),
                            keep=(eng.GACC, eng.G32, micro))
    kern = {}
    for name, m, nbytes in (("vqa_grad_accumulate_add", 1, 12), ("vqa_grad_accumulate_copy", 0, 8)):
        micro.fill_(m)
        med, lo, hi = time_call(lambda: acc_call(s), dev)
        kern[name] = {"elements": n, "bytes_per_element": nbytes, "ms": med, "ms_min": lo, "ms_max": hi,
                      "GBps": n * nbytes / med / 1e6}
    eng.GACC.zero_()                                      # a zero gradient: finite moments whatever the reps
    # the launch is a no-op unless an update is pending; nothing here clears the flag again
    eng.opt_state[Lb.ST_PENDING:Lb.ST_PENDING + 1].fill_(1.0)
    med, lo, hi = time_call(lambda: eng.adam_full(s), dev)
    kern["vqa_adamw_amsgrad_full"] = {"elements": n, "bytes_per_element": 38, "ms": med, "ms_min": lo, "ms_max": hi,
                                      "GBps": n * 38 / med / 1e6}
    for v in kern.values():
        v["share_of_hbm_peak"] = v["GBps"] / HBM_PEAK_GBS
    kern["accumulate_over_adamw_GBps"] = kern["vqa_grad_accumulate_add"]["GBps"] / kern["vqa_adamw_amsgrad_full"]["GBps"]
    out["kernels"] = kern
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
