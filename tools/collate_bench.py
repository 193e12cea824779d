"""Throughput of the input pipeline (data.DaquarCollate) against the train step.

  python tools/collate_bench.py [OUT.json] [--batches N] [--workers 0,4,8,16]
  python tools/collate_bench.py [OUT.json] --vit [--step-json BENCH.json] [--batches N] [--workers 0,4,8,16]

Writes 64 DAQUAR-like JPEGs (640 x 480 NYU-Depth frames, quality 90, random smooth
content so they compress like photographs) to a temp dir, then times, per decode-pool
size: host JPEG decode alone (PIL, `decode_workers` threads) and, with a GPU, the whole
collate (decode + pack + one H2D copy + the resize / ToTensor launch + question padding)
in pairs/s over N batches of 64.  The step consumes ~9,460 pairs/s (config 2, one GPU).

--vit: the ViT collate (data.DaquarVitCollate) on the same JPEGs, per decode-pool size, and the
GPU time of vqa_resize_pil_bilinear_u8 alone on the 64 decoded frames (device events around one
call, the median of 20 replays after 3 warm-ups), beside vqa_resize_linear_u8 to 224 x 224 on the
same frames.  --step-json: the result line `bench.py --model vit` printed in the same session; its
ms_per_step and the ratio of the resample's time to it go into the output."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def make_jpegs(d, n=64, seed=0):
    from PIL import Image
    g = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        # low-frequency content (a photograph-like spectrum): upsampled noise + gradients
        base = g.integers(0, 256, (30, 40, 3)).astype(np.float32)
        im = Image.fromarray(base.astype(np.uint8)).resize((640, 480), Image.BILINEAR)
        a = np.asarray(im).astype(np.float32) + g.normal(0, 6, (480, 640, 3))
        p = os.path.join(d, f"img{i:03d}.jpg")
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(p, quality=90)
        paths.append(p)
    return paths


def event_ms(fn, replays=20, warmups=3):
    """GPU time of fn() in ms between two device events: the median of `replays` after `warmups`."""
    for _ in range(warmups):
        fn()
    ts = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def resize_gpu_times(pkg, frames, size=224):
    """Event-timed GPU time of the two resize exports alone on the decoded `frames`."""
    L, D = pkg.lib, pkg.data
    lib, B = L.load(), len(frames)
    vb = D.VitImageBatcher(size, size)
    arrs = vb.check(frames)
    block, lut_off, tab_off = vb.metadata(arrs)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).cuda()
    meta = torch.from_numpy(block).cuda()
    max_h, max_w = max(a.shape[0] for a in arrs), max(a.shape[1] for a in arrs)
    stride = (max_h * size * 3 + 15) // 16 * 16
    work = torch.empty(B * stride, dtype=torch.uint8, device="cuda")
    out = torch.empty(B, 3, size, size, device="cuda")
    s = L.stream_handle()

    def pil():
        L.check(lib.vqa_resize_pil_bilinear_u8(src.data_ptr(), meta.data_ptr(), B, max_h, max_w, size, size,
                                               meta.data_ptr() + tab_off, meta.data_ptr() + lut_off, work.data_ptr(),
                                               stride, out.data_ptr(), s), "vqa_resize_pil_bilinear_u8")
    off, descs = 0, []
    for a in arrs:
        descs.append(L.ImageDesc(off, a.shape[0], a.shape[1]))
        off += a.nbytes
    darr = (L.ImageDesc * B)(*descs)
    ddesc = torch.from_numpy(np.frombuffer(darr, np.uint8).copy()).cuda()

    def linear():
        L.check(lib.vqa_resize_linear_u8(src.data_ptr(), ddesc.data_ptr(), B, size, size, out.data_ptr(), s),
                "vqa_resize_linear_u8")
    res = {}
    for name, fn in (("vqa_resize_pil_bilinear_u8", pil), ("vqa_resize_linear_u8", linear)):
        med, lo, hi = event_ms(fn)
        res[name] = {"gpu_ms_median": round(med, 4), "gpu_ms_min": round(lo, 4), "gpu_ms_max": round(hi, 4)}
    res["frames"] = B
    res["bytes_read"] = int(src.numel())
    res["bytes_intermediate"] = int(sum(a.shape[0] for a in arrs) * size * 3)
    res["bytes_written"] = int(out.numel() * 4)
    res["pil_over_linear"] = round(res["vqa_resize_pil_bilinear_u8"]["gpu_ms_median"]
                                   / res["vqa_resize_linear_u8"]["gpu_ms_median"], 3)
    return res


def main():
    args = sys.argv[1:]
    vit = "--vit" in args
    step_json = args[args.index("--step-json") + 1] if "--step-json" in args else None
    out = args[0] if args and not args[0].startswith("--") else None
    nb = int(args[args.index("--batches") + 1]) if "--batches" in args else 8
    workers = [int(w) for w in (args[args.index("--workers") + 1] if "--workers" in args else "0,4,8,16").split(",")]
    pkg = load_package()
    gpu = torch.cuda.is_available()
    res = {"batch": 64, "batches": nb, "image": "640x480 JPEG q90", "host_threads_visible": os.cpu_count(),
           "gpu": gpu, "collate": "DaquarVitCollate" if vit else "DaquarCollate", "runs": []}
    if vit and not gpu:
        raise SystemExit("--vit measures the GPU resample: no GPU found")
    with tempfile.TemporaryDirectory() as d:
        paths = make_jpegs(d)
        res["jpeg_bytes_mean"] = int(np.mean([os.path.getsize(p) for p in paths]))
        dps = [{"image_path": p, "question_ids": [5, 6, 7, 1], "decoder_question_ids": [5, 6, 7, 8, 1],
                "annotation_id": i % 170} for i, p in enumerate(paths)]
        if vit:
            r = resize_gpu_times(pkg, [pkg.data.decode_image(p) for p in paths])
            if step_json:
                line = [ln for ln in open(step_json).read().splitlines() if '"ms_per_step"' in ln][-1]
                r["vit_step_ms"] = json.loads(line)["ms_per_step"]
                r["pil_over_vit_step"] = round(r["vqa_resize_pil_bilinear_u8"]["gpu_ms_median"] / r["vit_step_ms"], 5)
            res["resize_gpu"] = r
            print(r, flush=True)
        for w in workers:
            if vit:
                col = pkg.data.DaquarVitCollate(32, decode_workers=w)
            else:
                col = pkg.data.DaquarCollate((224, 224), 32, device="cuda" if gpu else "cpu", decode_workers=w) \
                    if gpu else None
            dec = pkg.data.DaquarCollate.__new__(pkg.data.DaquarCollate)     # decode-only twin (no GPU)
            dec._pool = None
            if w:
                from concurrent.futures import ThreadPoolExecutor
                dec._pool = ThreadPoolExecutor(max_workers=w)
            dec._decode(dps)                                                 # warm the page cache / pool
            t0 = time.perf_counter()
            for _ in range(nb):
                dec._decode(dps)
            t_dec = (time.perf_counter() - t0) / nb
            r = {"decode_workers": w, "decode_pairs_per_s": round(64 / t_dec, 1)}
            if gpu:
                col(dps)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(nb):
                    col(dps)
                torch.cuda.synchronize()
                t_all = (time.perf_counter() - t0) / nb
                r["collate_pairs_per_s"] = round(64 / t_all, 1)
            res["runs"].append(r)
            print(r, flush=True)
    if out:
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
