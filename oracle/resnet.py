"""fp64-capable functional restatement of `basic` with a torchvision BasicBlock ResNet encoder (resnet18 / resnet34):
conv1 7x7/s2 -> bn1 -> relu -> maxpool 3x3/s2/p1 -> layer1..4 of BasicBlocks, over the state_dict, with
oracle.unet_mobilenetv3's _Net / unet_decoder and the heads of basic_forward.  Activations and the pool go through this
module's F at call time (tests patch F.relu, and may stand in for F to record the pool)."""
import torch.nn.functional as F

LAYERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


def _basic_block(n, x, name, stride, downsample):
    out = F.relu(n.bn(n.conv(x, f"{name}.conv1", stride, 1), f"{name}.bn1"))
    out = n.bn(n.conv(out, f"{name}.conv2", 1, 1), f"{name}.bn2")
    idt = n.bn(n.conv(x, f"{name}.downsample.0", stride, 0), f"{name}.downsample.1") if downsample else x
    return F.relu(out + idt)


def resnet_features(n, x, layers, depth=5):
    feats = [x]
    y = F.relu(n.bn(n.conv(x, "conv1", 2, 3), "bn1"))
    feats.append(y)
    if depth == 1:
        return feats
    y = F.max_pool2d(y, 3, 2, 1)
    cin = 64
    for i, (planes, nb) in enumerate(list(zip((64, 128, 256, 512), layers))[: depth - 1]):
        for j in range(nb):
            stride = 2 if (i > 0 and j == 0) else 1
            y = _basic_block(n, y, f"layer{i + 1}.{j}", stride, j == 0 and (stride != 1 or cin != planes))
            cin = planes
        feats.append(y)
    return feats


def resnet_basic_forward(sd, x, training, name, depth=5):
    from oracle.unet_mobilenetv3 import _Net, unet_decoder

    feats = resnet_features(_Net(sd, "backbone.encoder.", training), x, LAYERS[name], depth)
    dec = unet_decoder(_Net(sd, "backbone.decoder.", training), feats, n_blocks=depth)
    depth = F.conv2d(dec, sd["depth_head.0.weight"], sd["depth_head.0.bias"], padding=1)
    segm = F.conv2d(dec, sd["segm_head.0.weight"], sd["segm_head.0.bias"], padding=1)
    return dict(depth=depth, segm=segm)
