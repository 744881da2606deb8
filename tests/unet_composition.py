"""Functional fp32 restatement of the reference's UNet (model.py:83-174) on torch.nn.functional, for tests.

Pinned to the reference's own outputs (tests/golden/model_unet_*.npz) by tests/test_unet.py, so GPU tests can use it at sizes the
fixtures do not cover.  Test infrastructure only: the product never imports it."""
import torch
import torch.nn.functional as F


def conv_block(x, sd, p):
    h = F.leaky_relu(F.conv2d(x, sd[p + "block.0.weight"], sd[p + "block.0.bias"], padding=1), 0.01)
    h = F.leaky_relu(F.conv2d(h, sd[p + "block.2.weight"], sd[p + "block.2.bias"], padding=1), 0.01)
    return h + F.conv2d(x, sd[p + "conv11.weight"], sd[p + "conv11.bias"])


def unet_forward(x, sd):
    enc = []
    h = x
    for k in range(1, 6):
        if k > 1:
            h = F.conv2d(enc[-1], sd[f"pool{k - 1}.weight"], sd[f"pool{k - 1}.bias"], stride=2, padding=1)
        enc.append(conv_block(h, sd, f"ConvBlock{k}."))
    h = enc[-1]
    for k in range(6, 10):
        up = F.conv_transpose2d(h, sd[f"upv{k}.weight"], sd[f"upv{k}.bias"], stride=2)
        h = conv_block(torch.cat([up, enc[9 - k]], 1), sd, f"ConvBlock{k}.")
    return x + F.conv2d(h, sd["conv10.weight"], sd["conv10.bias"], padding=1)
