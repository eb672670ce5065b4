"""torchvision BasicBlock ResNet (resnet18 / resnet34) as a U-Net encoder on the HIP kernels.

The reference hands `encoder_name` to smp.Unet (reference vision_mtl/models/basic_model.py:10-29,
vision_mtl/utils/model_utils.py:10-31,118-132); smp's ResNetEncoder is torchvision's ResNet without `fc` / `avgpool`,
its stages [Identity, Seq(conv1, bn1, relu), Seq(maxpool, layer1), layer2, layer3, layer4] giving features with
3, 64, 64, 128, 256, 512 channels at strides 1..32.  The modules here carry torchvision's names, so state_dict keys and
shapes are torchvision's (under `backbone.encoder.`); they are parameter containers, the arithmetic is in ops:
  stem       conv1 7x7/s2 (implicit GEMM + statistics epilogue) -> bn1 + relu + maxpool 3x3/s2 as ONE node
             (ops.bn_act_pool3: the activated map is the stride-2 decoder skip, the pooled map feeds layer1)
  BasicBlock conv1 (3x3, stride 1 or 2) -> [bn1 + relu + conv2] (ops.bn_act_conv) ->
             relu(bn2(.) + identity)  or  relu(bn2(.) + downsample_bn(downsample_conv(x)))  (ops.bn_add_act)
Bottleneck ResNets (resnet50 and larger) are not restated.
"""
from __future__ import annotations

import typing as t

from torch import nn

from .. import layers as L
from .. import ops
from ..ops import ACT_RELU

# name -> blocks per stage (torchvision resnet18 / resnet34: BasicBlock)
BASIC_LAYERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
BOTTLENECK = ("resnet50", "resnet101", "resnet152", "resnext50_32x4d", "resnext101_32x4d", "resnext101_32x8d",
              "resnext101_32x16d", "resnext101_32x32d", "resnext101_32x48d")


class BasicBlock(nn.Module):
    """torchvision.models.resnet.BasicBlock (expansion 1)."""

    def __init__(self, inplanes: int, planes: int, stride: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
        self.stride = stride

    def run(self, x: L.Act) -> L.Act:
        x1, x2 = L.fork(x)  # conv1 and the shortcut
        raw1, st1, rpb1 = L.conv_raw(x1, self.conv1, self.bn1.training)
        C = self.conv1.out_channels
        raw2, st2, rpb2 = ops.bn_act_conv(raw1, st1, rpb1, self.bn1, C, ACT_RELU, self.conv2.weight,
                                          want_stats=self.bn2.training)
        z = L.Act(raw2, C)
        if self.downsample is None:
            return L.bn_add_act(z, st2, rpb2, self.bn2, ACT_RELU, res=x2)
        dc, dbn = self.downsample[0], self.downsample[1]
        rawd, std, rpbd = L.conv_raw(x2, dc, dbn.training)
        return L.bn_add_act(z, st2, rpb2, self.bn2, ACT_RELU, ds=(rawd, std, rpbd, dbn))


class ResNetEncoder(nn.Module):
    """smp encoders/resnet.py ResNetEncoder for BasicBlock ResNets: conv1, bn1, relu, maxpool, layer1..layer4."""

    def __init__(self, name: str = "resnet34", in_channels: int = 3, depth: int = 5):
        super().__init__()
        if name not in BASIC_LAYERS:
            raise NotImplementedError(f"encoder {name!r}: only the BasicBlock ResNets {sorted(BASIC_LAYERS)} are restated"
                                      + (" (Bottleneck ResNets are not)" if name in BOTTLENECK else ""))
        if not 1 <= depth <= 5:
            raise ValueError(f"encoder depth must be 1..5, got {depth}")
        self.name, self._depth = name, depth
        self.out_channels = (in_channels, 64, 64, 128, 256, 512)[: depth + 1]
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for i, (planes, n) in enumerate(zip((64, 128, 256, 512), BASIC_LAYERS[name])):
            stride = 1 if i == 0 else 2
            blocks = [BasicBlock(inplanes, planes, stride)] + [BasicBlock(planes, planes) for _ in range(n - 1)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
            inplanes = planes
        for m in self.modules():  # torchvision ResNet.__init__ (zero_init_residual=False)
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def run(self, x: L.Act) -> t.List[L.Act]:
        feats = [x]
        if self._depth == 1:
            feats.append(L.conv_bn_act(x, self.conv1, self.bn1, ACT_RELU))
            return feats
        skip, y = L.conv_bn_act_maxpool3(x, self.conv1, self.bn1, ACT_RELU)
        feats.append(skip)
        layers = [self.layer1, self.layer2, self.layer3, self.layer4][: self._depth - 1]
        for i, layer in enumerate(layers):
            for blk in layer:
                y = blk.run(y)
            if i == len(layers) - 1:  # the deepest feature: nothing downstream in the encoder
                feats.append(y)
            else:
                y, tap = L.fork(y)
                feats.append(tap)
        return feats
