"""Test infrastructure only: the CPU fp32 restatement of `FasterRcnnVQAModel`
(model/faster_rcnn_vqa_model.py) on top of oracle.vqa_oracle, which already restates everything
behind the vision map (T5 encoder, SGA blocks, pooler, head, clip, AdamW, schedule).

The vision branch is torchvision 0.16's `BackboneWithFPN` of fasterrcnn_resnet50_fpn: an
IntermediateLayerGetter over a ResNet-50 whose norms are FrozenBatchNorm2d (eps 1e-5; the same
arithmetic as the eval BatchNorm the oracle folds), returning layer1..layer4, and a
FeaturePyramidNetwork with a LastLevelMaxPool.  No detector part is kept by the model.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import vqa_oracle as orc

BODY, FPN = "vision_model.body.", "vision_model.fpn."


def body_features(sd, x):
    """C2..C5: the outputs of layer1..layer4 (oracle.vqa_oracle.resnet_features returns the last
    one only, so its ResNet-50 loop is restated here with the four taps)."""
    sdp = {k[len(BODY):]: v for k, v in sd.items() if k.startswith(BODY)}
    x = F.conv2d(x.float(), sdp["conv1.weight"], stride=2, padding=3)
    x = F.max_pool2d(F.relu(orc._bn_eval(x, sdp, "bn1")), 3, 2, 1)
    out = []
    for li, nb in enumerate((3, 4, 6, 3)):
        for bi in range(nb):
            p = f"layer{li + 1}.{bi}."
            stride = (1 if li == 0 else 2) if bi == 0 else 1
            idt = x
            o = F.relu(orc._bn_eval(F.conv2d(x, sdp[p + "conv1.weight"]), sdp, p + "bn1"))
            o = F.relu(orc._bn_eval(F.conv2d(o, sdp[p + "conv2.weight"], stride=stride, padding=1), sdp, p + "bn2"))
            o = orc._bn_eval(F.conv2d(o, sdp[p + "conv3.weight"]), sdp, p + "bn3")
            if (p + "downsample.0.weight") in sdp:
                idt = orc._bn_eval(F.conv2d(x, sdp[p + "downsample.0.weight"], stride=stride), sdp, p + "downsample.1")
            x = F.relu(o + idt)
        out.append(x)
    return out


def _conv(sd, name, x, **kw):
    return F.conv2d(x, sd[FPN + name + ".0.weight"], sd[FPN + name + ".0.bias"], **kw)


def fpn_maps(sd, images):
    """FeaturePyramidNetwork.forward + LastLevelMaxPool: {'0','1','2','3','pool'}."""
    with torch.no_grad():
        c = body_features(sd, images)
        last = _conv(sd, "inner_blocks.3", c[3])
        out = {"3": _conv(sd, "layer_blocks.3", last, padding=1)}
        for i in (2, 1, 0):
            lat = _conv(sd, f"inner_blocks.{i}", c[i])
            last = lat + F.interpolate(last, size=lat.shape[-2:], mode="nearest")
            out[str(i)] = _conv(sd, f"layer_blocks.{i}", last, padding=1)
        out["pool"] = F.max_pool2d(out["3"], 1, 2, 0)
    return out


def pool_stride2(sd, images):
    """The 'pool' level as the engine plans it: layer_blocks.3 taken at stride 2 over the lateral map."""
    with torch.no_grad():
        c5 = orc.resnet_features(sd, images, "resnet50", prefix=BODY)
        return _conv(sd, "layer_blocks.3", _conv(sd, "inner_blocks.3", c5), stride=2, padding=1)


def heatmap(fmap):
    """CNN_vqa_heatmap.py:131-137 per image: channel mean, min-max normalised (0 / 0 for a constant map)."""
    cam = fmap.mean(dim=1)
    mn = cam.flatten(1).min(dim=1).values[:, None, None]
    mx = cam.flatten(1).max(dim=1).values[:, None, None]
    return (cam - mn) / (mx - mn)


def model_forward(sd, batch, num_blocks=3, return_features=False, drop=orc._nodrop, pool=None):
    """FasterRcnnVQAModel.forward (:88-138); generate_answers (:140-197) with return_features."""
    maps = None
    if pool is None:
        maps = fpn_maps(sd, batch["image_tensors"])
        pool = maps["pool"]
    vis = F.conv_transpose2d(pool, sd["upscale_layer.weight"], sd["upscale_layer.bias"], stride=1, padding=1)
    txt = orc.t5_encoder(sd, batch["question_input_ids"], batch["question_attention_masks"], drop=drop)
    y = vis.view(vis.shape[0], vis.shape[1], -1).permute(0, 2, 1)
    fused = None
    for n in range(num_blocks):
        fused = orc.sga_block(sd, f"sga_modules.{n}", txt, y, drop, n)
        y = fused
    a = torch.softmax(fused @ sd["attention_pooler.attention.0.weight"].T + sd["attention_pooler.attention.0.bias"],
                      dim=1)
    pooled = torch.bmm(a.transpose(1, 2), fused).squeeze(1)
    lp = F.log_softmax(pooled @ sd["classification_layer.weight"].T + sd["classification_layer.bias"], dim=-1)
    loss = None
    if batch.get("annotation_ids") is not None:
        loss = F.nll_loss(lp, batch["annotation_ids"])
    return (lp, loss, maps) if return_features else (lp, loss)


class FrcnnOracleTrainer(orc.OracleTrainer):
    """OracleTrainer over the model above (trainable_keys / group_of: everything but
    vision_model.*; upscale_layer is the scaler group).  The frozen pool map of a batch is
    computed once per batch object and reused by later steps on it."""

    def __init__(self, sd, **kw):
        super().__init__(sd, "faster-rcnn", **kw)
        self._pool = {}

    def forward_backward(self, batch):
        for k in self.keys:
            self.sd[k].grad = None
        drop = orc._nodrop
        if self.dropout > 0.0:
            self.rng_counter += 1
            drop = orc.HashDropout(self.dropout, self.seed, self.rng_counter)
        key = id(batch["image_tensors"])
        if key not in self._pool:
            self._pool = {key: fpn_maps(self.sd, batch["image_tensors"])["pool"]}
        lp, loss = model_forward(self.sd, batch, self.num_blocks, drop=drop, pool=self._pool[key])
        loss.backward()
        return lp.detach(), loss.detach()
