"""The tests' own restatement of detectron2's MSRA ResNet (STRIDE_IN_1X1 True, configs/R101_coco.yaml, R101_ytvis19.yaml): the
oracle's ResNet (oracle/mdqe_oracle.py::resnet) with a downsampling block's stride on the 1x1 conv1 instead of the 3x3 conv2.
Built from the oracle's own conv + FrozenBN step; pinned against transformers.ResNetModel in tests/test_resnet_msra_cpu.py and
handed to the oracle through its `backbone_fn` hook by tests/test_resnet_msra_gpu.py."""
import torch.nn.functional as F

import mdqe_oracle as O


def resnet_msra(sd, p, x, depth=50):
    """-> res3, res4, res5 (NCHW)."""
    x = O._conv_bn(sd, p + ".stem.conv1", x, 2, 3)
    x = F.max_pool2d(x, 3, 2, 1)
    outs = []
    for si, nb in enumerate(O.RESNET_BLOCKS[depth]):
        for b in range(nb):
            q = f"{p}.res{si + 2}.{b}"
            s = 2 if (b == 0 and si > 0) else 1
            sc = O._conv_bn(sd, q + ".shortcut", x, s, 0, relu=False) if (q + ".shortcut.weight") in sd else x
            y = O._conv_bn(sd, q + ".conv1", x, s, 0)
            y = O._conv_bn(sd, q + ".conv2", y, 1, 1)
            y = O._conv_bn(sd, q + ".conv3", y, 1, 0, relu=False)
            x = F.relu(y + sc)
        if si >= 1:
            outs.append(x)
    return outs
