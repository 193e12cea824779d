"""Stand-in for `torchvision.models.detection.fasterrcnn_resnet50_fpn`, used ONLY by
make_golden_frcnn.py.

torchvision is not installed in the build container, so the reference
`model/faster_rcnn_vqa_model.py:5` import cannot resolve.  The reference keeps only the
detector's `.backbone` (`:51-53`) and reads the levels it returns (`:102-108, 153-161`), so this
module restates that one attribute: torchvision 0.16's `BackboneWithFPN` -- `body`, a ResNet-50
(v1.5) without avgpool / fc whose norms are `FrozenBatchNorm2d` (four buffers, eps 1e-5, no
num_batches_tracked), returning layer1..layer4, and `fpn`, a FeaturePyramidNetwork (1x1 inner
and 3x3 layer blocks to 256 channels, each a Conv2dNormActivation holding one biased conv at index
0, nearest top-down upsampling, LastLevelMaxPool) -- with torchvision's child names and
state_dict keys.  It is a stand-in written from a description of that module, as tv_stub.py is
for ResNet: the ResNet / FPN arithmetic is pinned by this restatement, not by torchvision's code.
`pretrained=True` is accepted and ignored (no network); weights are loaded afterwards.
"""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F


class FrozenBatchNorm2d(nn.Module):
    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def forward(self, x):
        w, b = self.weight.reshape(1, -1, 1, 1), self.bias.reshape(1, -1, 1, 1)
        rv, rm = self.running_var.reshape(1, -1, 1, 1), self.running_mean.reshape(1, -1, 1, 1)
        scale = w * (rv + self.eps).rsqrt()
        return x * scale + (b - rm * scale)


class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = FrozenBatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = FrozenBatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = FrozenBatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        idt = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            idt = self.downsample(x)
        return self.relu(out + idt)


class Body(nn.ModuleDict):
    """IntermediateLayerGetter over resnet50 up to layer4: {'0': C2, '1': C3, '2': C4, '3': C5}."""

    def __init__(self):
        inplanes = 64
        mods = OrderedDict(conv1=nn.Conv2d(3, 64, 7, 2, 3, bias=False), bn1=FrozenBatchNorm2d(64),
                           relu=nn.ReLU(inplace=True), maxpool=nn.MaxPool2d(3, 2, 1))
        for i, (planes, blocks) in enumerate(zip((64, 128, 256, 512), (3, 4, 6, 3))):
            stride = 1 if i == 0 else 2
            down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), FrozenBatchNorm2d(planes * 4))
            layers = [Bottleneck(inplanes, planes, stride, down)]
            inplanes = planes * 4
            layers += [Bottleneck(inplanes, planes) for _ in range(1, blocks)]
            mods[f"layer{i + 1}"] = nn.Sequential(*layers)
        super().__init__(mods)

    def forward(self, x):
        out = OrderedDict()
        for name, m in self.items():
            x = m(x)
            if name.startswith("layer"):
                out[str(int(name[5:]) - 1)] = x
        return out


class FeaturePyramidNetwork(nn.Module):
    def __init__(self, in_channels=(256, 512, 1024, 2048), out_channels=256):
        super().__init__()
        # Conv2dNormActivation(norm_layer=None, activation_layer=None) is a Sequential of one conv
        self.inner_blocks = nn.ModuleList(nn.Sequential(nn.Conv2d(c, out_channels, 1)) for c in in_channels)
        self.layer_blocks = nn.ModuleList(nn.Sequential(nn.Conv2d(out_channels, out_channels, 3, padding=1))
                                          for _ in in_channels)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        names, feats = list(x.keys()), list(x.values())
        last = self.inner_blocks[-1](feats[-1])
        results = [self.layer_blocks[-1](last)]
        for i in range(len(feats) - 2, -1, -1):
            lateral = self.inner_blocks[i](feats[i])
            last = lateral + F.interpolate(last, size=lateral.shape[-2:], mode="nearest")
            results.insert(0, self.layer_blocks[i](last))
        names.append("pool")                                 # LastLevelMaxPool
        results.append(F.max_pool2d(results[-1], 1, 2, 0))
        return OrderedDict(zip(names, results))


class BackboneWithFPN(nn.Module):
    def __init__(self):
        super().__init__()
        self.body = Body()
        self.fpn = FeaturePyramidNetwork()
        self.out_channels = 256

    def forward(self, x):
        return self.fpn(self.body(x))


class _Detector(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = BackboneWithFPN()


def fasterrcnn_resnet50_fpn(pretrained=False, **kw):
    return _Detector()
