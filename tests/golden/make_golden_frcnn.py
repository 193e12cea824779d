"""Generate tests/golden/model_frcnn_256_l16.npz from the REFERENCE `FasterRcnnVQAModel`
(build container only).

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_frcnn.py

make_golden.py's recipe (its module set-up is imported as it is: the reference on sys.path,
transformers before the torchvision stub, T5 built from a local config), plus
`torchvision.models.detection` -> tests/golden/tv_frcnn_stub.py.  The case has
full_model_case's fields (B = 4, L = 16, H = 256, 3 eval-mode steps); `feat_*` is taken from
generate_answers(...)['pool'], `pyr_slice_{0,1,2,3}` are the first 8 channels of each FPN level,
and `sd_keys` / `sd_shapes` record the reference module's own state_dict() layout.  Outputs,
norms, hashes and names only -- no weights.
"""
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import transformers  # noqa: E402

import make_golden as MG  # noqa: E402  (sets up the reference imports and the torchvision stub)
import tv_frcnn_stub  # noqa: E402

det = types.ModuleType("torchvision.models.detection")
det.fasterrcnn_resnet50_fpn = tv_frcnn_stub.fasterrcnn_resnet50_fpn
sys.modules["torchvision"].models.detection = det
sys.modules["torchvision.models.detection"] = det

from model.faster_rcnn_vqa_model import FasterRcnnVQAModel  # noqa: E402

syn = MG.syn
VISION = "faster-rcnn"


def build_model():
    m = FasterRcnnVQAModel(VISION, "t5-base", answer_spaces=170)
    sd = syn.make_state_dict(VISION, seed=0)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    m.eval()
    return m


def frcnn_case(B=4, L=16, H=256, nsteps=3, warmup=2, total=20, seed=1):
    torch.manual_seed(0)
    model = build_model()
    ref_sd = model.state_dict()
    out = {"sd_keys": np.array(list(ref_sd)),
           "sd_shapes": np.array(["x".join(map(str, v.shape)) for v in ref_sd.values()]),
           "vision_param_count": len(list(model.vision_model.parameters()))}
    opt = MG.optimizer_groups(model)
    sched = transformers.get_linear_schedule_with_warmup(opt, num_warmup_steps=warmup, num_training_steps=total)
    nb = syn.make_batch(B, L, H, seed=seed)
    batch = MG.tb(nb)
    out.update({"image_sha": MG.sha(nb["image_tensors"]), "ids": nb["question_input_ids"],
                "mask": nb["question_attention_masks"], "targets": nb["annotation_ids"],
                "B": B, "L": L, "H": H, "warmup": warmup, "total": total})
    losses, norms, gnorms = [], [], []
    for s in range(nsteps):
        opt.zero_grad()
        lp, loss = model(**batch)
        loss.backward()
        if s == 0:
            out["log_probs"] = lp.detach().numpy()
            _, _, fmap = model.generate_answers(**{k: v for k, v in batch.items() if k != "annotation_ids"})
            assert list(fmap) == ["0", "1", "2", "3", "pool"], list(fmap)
            f = fmap["pool"].detach().numpy()
            out["feat_sum"] = np.array([f.sum(), np.abs(f).sum(), (f * f).sum()], dtype=np.float64)
            out["feat_slice"] = f[:, :8, :, :].copy()
            for k in "0123":
                out[f"pyr_slice_{k}"] = fmap[k].detach().numpy()[:, :8].copy()
        gnorms.append(MG.group_norms(model))
        gn = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        sched.step()
        losses.append(float(loss))
        norms.append(float(gn))
    out["losses"], out["grad_norms"], out["group_grad_norms"] = np.array(losses), np.array(norms), np.array(gnorms)
    sd = model.state_dict()
    out["post_t5_q0"] = sd["lang_model.block.0.layer.0.SelfAttention.q.weight"][:4, :16].numpy().copy()
    out["post_cls_w"] = sd["classification_layer.weight"][:4, :16].numpy().copy()
    out["post_sga_fc1"] = sd["sga_modules.2.ffn.mlp.fc1.weight"][:4, :16].numpy().copy()
    out["post_scaler_w"] = sd["upscale_layer.weight"][:4, :4].numpy().copy()
    init = syn.make_state_dict(VISION, seed=0)
    delta = {g: 0.0 for g in MG.GROUPS}
    for k, v in sd.items():
        if k.startswith("vision_model"):
            continue
        top = k.split(".", 1)[0]
        g = "scaler" if top in ("upscale_layer", "downscale_layer") else top
        delta[g] += float(np.abs(v.numpy().astype(np.float64) - init[k]).sum())
    out["group_abs_delta"] = np.array([delta[g] for g in MG.GROUPS])
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "model_frcnn_256_l16.npz"), **frcnn_case())
    print("faster-rcnn done", flush=True)
