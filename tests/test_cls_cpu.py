"""The classifier's torch module (nets.nn.YOLOCls), its weight mapping, the Classifier front end on
the CPU device and the new C ABI symbols. No GPU."""
import os
import pickle
import re

import pytest
import torch

import _cls_cases as cc
from yolo_hip import _lib, weights
from yolo_hip.classify import Classified, Classifier


def test_state_dict_keys_and_shapes():
    from nets import nn
    m = nn.yolo_v11_cls_n(10)
    sd = m.state_dict()
    assert not any(k.startswith("net.p5.3") or k.startswith("fpn.") for k in sd)
    assert tuple(sd["net.p5.2.conv1.conv.weight"].shape) == (256, 256, 1, 1)         # C2PSA, not the SPPF
    assert "net.p5.2.res_m.0.conv1.qkv.conv.weight" in sd
    assert tuple(sd["head.conv.conv.weight"].shape) == (1280, 256, 1, 1)
    assert tuple(sd["head.conv.norm.running_var"].shape) == (1280,)
    assert tuple(sd["head.linear.weight"].shape) == (10, 1280) and tuple(sd["head.linear.bias"].shape) == (10,)
    assert [k for k in sd if k.startswith("head.")] == [
        "head.conv.conv.weight", "head.conv.norm.weight", "head.conv.norm.bias", "head.conv.norm.running_mean",
        "head.conv.norm.running_var", "head.conv.norm.num_batches_tracked", "head.linear.weight", "head.linear.bias"]
    # the backbone's keys are the detector's, minus the SPPF, with C2PSA one place earlier
    det = {k for k in nn.yolo_v11_n(80).state_dict() if k.startswith("net.")}
    want = {k.replace("net.p5.3.", "net.p5.2.") for k in det if not k.startswith("net.p5.2.")}
    assert {k for k in sd if k.startswith("net.")} == want
    assert m._yh_arch == ((3, 16, 32, 64, 128, 256), (1,) * 6, (False, True), 10)
    for v, w5 in (("t", 384), ("s", 512), ("m", 512), ("l", 512), ("x", 768)):
        assert getattr(nn, f"yolo_v11_cls_{v}")(7)._yh_arch[0][5] == w5


def test_forward_features_pickle():
    m = cc.make_model("n", 10)
    x = cc.inputs(3, 64, 96).float() / 255
    with torch.no_grad():
        p = m(x)
        pf, z, e = m.features(x)
    assert tuple(p.shape) == (3, 10) and tuple(z.shape) == (3, 10) and tuple(e.shape) == (3, 1280)
    assert torch.allclose(p.sum(1), torch.ones(3), atol=1e-6)
    assert torch.equal(p, pf) and torch.equal(p, z.softmax(1))
    mt = cc.make_model("n", 10).train()   # (a training forward moves the BN statistics: its own copy)
    with torch.no_grad():
        zt = mt(x)
    assert tuple(zt.shape) == (3, 10) and not torch.allclose(zt.sum(1), torch.ones(3))   # logits in training
    m2 = pickle.loads(pickle.dumps(m))
    assert m2._yh_arch == m._yh_arch
    state = dict(m.__dict__)
    del state["_yh_arch"]
    m3 = type(m).__new__(type(m))
    m3.__setstate__(state)
    assert m3._yh_arch == m._yh_arch
    with torch.no_grad():
        assert torch.equal(m2(x), p)
    fused = cc.make_model("n", 10).fuse()
    assert not hasattr(fused.head.conv, "norm")
    with torch.no_grad():
        assert (fused(x) - p).abs().max() < 1e-5


@pytest.mark.parametrize("variant,nc,b,h,w", [("n", 1000, 4, 224, 224), ("s", 10, 3, 96, 160), ("n", 1000, 2, 320, 320)])
def test_synthetic_weights_regime(variant, nc, b, h, w):
    """The synthetic classifier is in a sane regime in fp64: p5 rms, logit spread, top probabilities
    (measured: rms 1.28 / 2.12 / 0.81, logit std 2.64 / 3.63 / 1.37, top probabilities 0.017 - 0.996)."""
    m = cc.make_model(variant, nc, torch.float64)
    with torch.no_grad():
        f = m.net(cc.inputs(b, h, w).double() / 255)[2]
    p, z, _ = cc.reference(variant, nc, b, h, w)
    rms = f.pow(2).mean().sqrt().item()
    zs = z.std(1).mean().item()
    top = p.max(1).values
    print(f"p5 rms {rms:.3f}  logit std {zs:.2f}  top probs {top.tolist()}")
    # neither vanishing nor exploding features; logits spread enough that the softmax is far from
    # uniform (gain 1 gives a std near 0.4) and not saturated
    assert 0.7 <= rms <= 2.5
    assert 1.0 <= zs <= 8.0
    assert 5.0 / nc <= top.min().item() and top.max().item() <= 0.9999


def test_classifier_cpu_chunks_and_total():
    m = cc.make_model("n", 10)
    x = cc.inputs(5, 32, 64)
    one = Classifier(m, "cpu", max_batch=8).predict(x, embed=True)
    two = Classifier(m, "cpu", max_batch=2).predict(x, embed=True)
    assert isinstance(one, Classified) and one.top1.dtype == torch.int32 and int(one.total) == 5
    assert torch.allclose(one.probs, two.probs, atol=1e-6) and torch.equal(one.top1, two.top1)
    assert torch.allclose(one.embed, two.embed, atol=1e-4, rtol=1e-4)   # torch picks conv algorithms by batch
    with torch.no_grad():
        want = m(x.float() / 255)
    assert torch.allclose(one.probs, want, atol=1e-6)
    assert torch.equal(one.top1.long(), want.argmax(1)) and torch.allclose(one.conf, want.max(1).values, atol=1e-6)

    class FakeCrops:   # the three fields of yolo_hip.preprocess.Crops
        def __init__(self, data, total):
            self.data, self.rois, self.total = data, torch.zeros((data.shape[0], 6), dtype=torch.int32), total

    for n in (0, 3, 5, 9, -2):
        got = Classifier(m, "cpu", max_batch=2).predict(FakeCrops(x, torch.tensor([n], dtype=torch.int32)), embed=True)
        k = min(max(n, 0), 5)
        assert torch.allclose(got.probs[:k], want[:k], atol=1e-6)
        assert not got.probs[k:].any() and not got.embed[k:].any() and not got.conf[k:].any()
        assert (got.top1[k:] == -1).all() and (got.top1[:k] >= 0).all()
    assert Classifier(m, "cpu").predict(x).embed is None
    with pytest.raises(ValueError):
        Classifier(m, "cpu").predict(x[0])


def test_ultralytics_exact_mapping():
    m = cc.make_model("n", 10)
    names = weights.ultralytics_names(m)
    assert set(names) == set(m.state_dict())
    assert names["head.conv.conv.weight"] == "model.10.conv.conv.weight"
    assert names["head.conv.norm.running_mean"] == "model.10.conv.bn.running_mean"
    assert names["head.linear.bias"] == "model.10.linear.bias"
    assert names["net.p5.2.res_m.0.conv1.conv1.conv.weight"] == "model.9.m.0.attn.pe.conv.weight"
    assert names["net.p5.1.res_m.0.res_m.1.conv2.norm.weight"] == "model.8.m.0.m.1.cv2.bn.weight"
    assert names["net.p1.0.conv.weight"] == "model.0.conv.weight"
    assert len(set(names.values())) == len(names)
    assert all(re.match(r"model\.(\d|10)\.", u) for u in names.values())
    g = torch.Generator().manual_seed(3)
    src = {u: (torch.rand(t.shape, generator=g) if t.is_floating_point() else torch.full_like(t, 7))
           for (k, t), u in zip(m.state_dict().items(), names.values())}
    mapped = weights.map_ultralytics(src, m, mapping="exact")
    assert set(mapped) == set(m.state_dict())
    fresh = cc.make_model("n", 10)
    weights.load_ultralytics_weight(fresh, src, mapping="exact")
    for k, t in fresh.state_dict().items():
        assert torch.equal(t, src[names[k]]), k
    with pytest.raises(ValueError, match="reference"):
        weights.map_ultralytics(src, m, mapping="reference")


def test_abi_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "yolo_hip.h")).read()
    lib = _lib.lib()
    for name in ("yh_create_cls", "yh_classify"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib._PROTOS and hasattr(lib, name)
    assert "#define YH_CLS_EMBED 1280" in header
    assert len(_lib._PROTOS["yh_classify"][1]) == 11
    import yolo_hip
    from yolo_hip import classify
    assert yolo_hip.Classifier is classify.Classifier and yolo_hip.Classified is classify.Classified
