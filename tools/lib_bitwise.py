"""Bitwise fingerprint of the benched step under the tree and library it runs from (an A/B of two
builds or two trees that must give the same bits: run once per side, compare the printed lines).
Builds the bench engine (B = 64, 224², pipelined, tuned, graphed, dropout 0.1), runs 3 steps and
prints the losses and a SHA-256 of the fp32 parameters, AdamW moments, bf16 shadow and log-probs.
  python tools/lib_bitwise.py [--fuse-norm | --dp-groups | --config5 | --model vit]
--fuse-norm: the engine with fuse_norm; --dp-groups: with dp.dp_t5_dw_groups' weight-gradient
groups; --config5: bench.py --config5's engine (t5-large, six blocks, e4m3 forward weight GEMMs)
at 224²; --model vit: VitVQAEngine at B = 4, seq_len 16, dec_len 8, 224², dropout 0.1, untuned,
graphed, over vit_model.make_batch batches."""
import argparse
import hashlib
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fuse-norm", action="store_true")
ap.add_argument("--dp-groups", action="store_true")
ap.add_argument("--config5", action="store_true")
ap.add_argument("--model", choices=("resnet", "vit"), default="resnet")
opt = ap.parse_args()
if opt.fuse_norm:
    os.environ["VQA_FUSE_NORM"] = "1"              # read by VQAEngine(fuse_norm=None), as bench.py builds it

pkg = load_package()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
on_dev = lambda nb: {k: torch.as_tensor(v).to(dev) for k, v in nb.items() if v is not None}   # noqa: E731
if opt.model == "vit":
    vm = pkg.vit_model
    eng = pkg.vit_engine.VitVQAEngine(vm.make_state_dict(seed=0), batch=4, seq_len=16, dec_len=8, image_size=224,
                                      device=dev, dropout=0.1)
    pool = [on_dev(vm.make_batch(4, 16, 8, 224, seed=1 + i)) for i in range(3)]
    eng.capture()

    def step(i):
        eng.load_batch(pool[i])
        eng.train_step()
else:
    args = types.SimpleNamespace(batch=64, seq_len=32, image_size=224, blocks=6 if opt.config5 else 3,
                                 no_pipeline=False, dp_groups=opt.dp_groups, config5=opt.config5,
                                 tune_table=os.path.join(ROOT, "t5-resnet-vqa_amd", "tuning", "gemm_gfx950.json"),
                                 tune_save=None, no_graph=False, shard_optimizer=False, dp_res_split=None,
                                 res_cumask=None)
    pool = [on_dev(pkg.synthetic.make_batch(64, 32, 224, seed=1 + i)) for i in range(4)]
    eng, _, step = bench.make_step(args, pkg, dev, pool, False, 0, "t5-large" if opt.config5 else "t5-base")
losses = []
for i in range(3):
    step(i)
    torch.cuda.synchronize()
    losses.append(float(eng.LOSS.item()))
eng.flush_optimizer()
torch.cuda.synchronize()
h = hashlib.sha256()
for t in (eng.P32, eng.M, eng.V, eng.VMAX, eng.P16, eng.LOGP):
    h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
print(json.dumps({"variant": " ".join(sys.argv[1:]), "losses": losses, "sha256": h.hexdigest()}))
