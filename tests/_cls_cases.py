"""Shared by the classifier tests: nets.nn.YOLOCls models with deterministic synthetic weights, the
cases of tests/test_gpu_cls.py and fp64 restatements of the head.

Weights: the backbone's values are the detector's calibrated synthetic state dict
(synth.synth_state_dict of yolo_v11_<v>(80), seed 0) with net.p5.3.* (C2PSA) renamed to net.p5.2.*;
the head's come from numpy PCG64 keyed by name: conv weight N(0, 1/cin), BN gamma and running var
U(0.75, 1.25), BN beta and running mean N(0, 0.1), linear weight N(0, 36/1280) (gain 6: with gain 1
the softmax is nearly uniform and a test on probabilities shows nothing), linear bias N(0, 0.1).
test_cls_cpu.py checks the regime (p5 feature rms, logit std, top probabilities) in fp64.
"""
import functools
import zlib

import numpy as np
import torch

from yolo_hip import synth

LINEAR_GAIN = 6.0

# (variant, dtype, nc, batch, H, W): the smallest shapes at which the head can still go wrong
CASES = [
    ("n", torch.bfloat16, 1000, 4, 224, 224),   # 49 px: one full row tile plus a partial one
    ("n", torch.float16, 1000, 4, 224, 224),
    ("n", torch.float32, 1000, 4, 224, 224),
    ("n", torch.bfloat16, 3, 5, 32, 32),        # 1 px per image, nc below 8, images packed into one tile
    ("s", torch.float16, 10, 3, 96, 160),       # 15 px: odd map, width[5] = 512
    ("n", torch.bfloat16, 1000, 2, 320, 320),   # 100 px: several row tiles per image
    ("n", torch.bfloat16, 10, 33, 128, 64),     # 8 px: ReID-shaped crop, batch beyond one workgroup's images
    ("m", torch.bfloat16, 10, 1, 64, 64),       # 4 px: C3k backbone, batch 1
]


def case_id(c):
    v, dt, nc, b, h, w = c
    return f"{v}-{str(dt).split('.')[-1]}-nc{nc}-b{b}-{h}x{w}"


def _rng(name):
    return np.random.Generator(np.random.PCG64([0, zlib.crc32(name.encode())]))


def head_tensor(name, shape):
    rng, shape = _rng(name), tuple(int(s) for s in shape)
    if name.endswith("num_batches_tracked"):
        return np.zeros(shape, dtype=np.int64)
    if name.endswith("norm.weight") or name.endswith("norm.running_var"):
        return rng.uniform(0.75, 1.25, size=shape).astype(np.float32)
    if name.endswith("norm.bias") or name.endswith("norm.running_mean"):
        return rng.normal(0.0, 0.1, size=shape).astype(np.float32)
    if name == "head.conv.conv.weight":
        return (rng.standard_normal(size=shape) / np.sqrt(shape[1])).astype(np.float32)
    if name == "head.linear.weight":
        return (rng.standard_normal(size=shape) * (LINEAR_GAIN / np.sqrt(shape[1]))).astype(np.float32)
    if name == "head.linear.bias":
        return rng.normal(0.0, 0.1, size=shape).astype(np.float32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def state_dict(variant, nc):
    from nets import nn
    torch.manual_seed(0)
    det = getattr(nn, f"yolo_v11_{variant}")(80)
    src = synth.synth_state_dict(det.state_dict(), seed=0)
    model = getattr(nn, f"yolo_v11_cls_{variant}")(nc)
    out = {}
    for k, t in model.state_dict().items():
        if k.startswith("head."):
            out[k] = torch.from_numpy(head_tensor(k, t.shape))
        elif k.startswith("net.p5.2."):
            out[k] = src["net.p5.3." + k[len("net.p5.2."):]].clone()
        else:
            out[k] = src[k].clone()
        assert out[k].numel() == t.numel(), k
        out[k] = out[k].reshape(t.shape)
    return out


def make_model(variant, nc, dtype=torch.float32):
    """A fresh eval-mode yolo_v11_cls_<variant>(nc) with the synthetic weights (not fused)."""
    from nets import nn
    model = getattr(nn, f"yolo_v11_cls_{variant}")(nc)
    model.load_state_dict(state_dict(variant, nc))
    return model.eval().to(dtype)


def inputs(batch, h, w, seed=5):
    """(B, 3, H, W) uint8 scenes: the crops' format."""
    return (synth.synth_scenes(batch, h, w, seed=seed) * 255).round().clamp(0, 255).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def reference(variant, nc, batch, h, w):
    """(probs, logits, embed) of the module in fp64 on the CPU for inputs(batch, h, w) / 255."""
    m = make_model(variant, nc, torch.float64)
    with torch.no_grad():
        p, z, e = m.features(inputs(batch, h, w).double() / 255)
    return p, z, e


@functools.lru_cache(maxsize=None)
def cpu_in_dtype(variant, nc, batch, h, w, dtype):
    """The same module run on the CPU in `dtype` (the bar of the 16-bit end-to-end test)."""
    m = make_model(variant, nc, dtype)
    with torch.no_grad():
        p, z, e = m.features(inputs(batch, h, w).to(dtype) / 255)
    return p.double(), z.double(), e.double()


def folded_head_conv(variant, nc):
    """fp32-folded head.conv (weight (1280, cin), bias (1280,)) exactly as the library folds it
    (csrc/net_weights.cpp load_conv, fuse_conv's order: s = gamma / sqrt(var + eps), W' = s W,
    b' = beta - gamma * mean / sqrt(var + eps), every operation one IEEE fp32 operation), and
    head.linear's (W, b). numpy, not torch: torch's vectorised CPU division is not correctly
    rounded for every element, and one fp32 ulp of a scale moves a whole row of the fp32 handle's
    conv by more than its outputs' ulp."""
    sd = state_dict(variant, nc)
    f32 = lambda k: sd[k].numpy().astype(np.float32)
    w = f32("head.conv.conv.weight")[:, :, 0, 0]
    g, be = f32("head.conv.norm.weight"), f32("head.conv.norm.bias")
    mu, var = f32("head.conv.norm.running_mean"), f32("head.conv.norm.running_var")
    den = np.sqrt(var + np.float32(1e-3), dtype=np.float32)
    s = (g / den).astype(np.float32)
    wc = (s[:, None] * w).astype(np.float32)
    bc = (be - (g * mu).astype(np.float32) / den).astype(np.float32)
    return (torch.from_numpy(wc), torch.from_numpy(bc), sd["head.linear.weight"].float(), sd["head.linear.bias"].float())
