"""yh_fuse (csrc/fuse.hip) on the device: the bytes of yh_fuse_host on the whole case list of
tests/_fuse_cases.py, and Detector(tta=...) end to end - a mirrored pass over a mirrored image is the
plain pass over the image, mirrored. Marked gpu.
"""
import numpy as np
import pytest
import torch

import _fuse_cases as fc
from test_fuse_host import run
from yolo_hip import synth
from yolo_hip.detect import Detector

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", fc.ALL)
def test_device_equals_host(gpu, name):
    c = fc.case(name)
    out, cnt = run(c, gpu)
    host, hcnt = run(c, threads=1)
    assert cnt.cpu().tolist() == hcnt.tolist()
    assert out.cpu().numpy().tobytes() == host.numpy().tobytes()


def test_mirrored_pass_over_the_mirrored_image(gpu):
    """v11_n bf16, 128 x 128 images on a 128 x 128 canvas (the letterbox is the identity), batch 2: the
    mirrored pass flips the mirrored images back, so the network reads the same bytes in both runs.
    Counts, classes and scores are equal; x comes back as W - x with x1 and x2 swapped, within one
    fp32 ulp of W, wherever the transformed x-range lies inside [0, W]."""
    from nets import nn
    from yolo_hip.engine import Engine
    S = 128
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    eng = Engine(*model._yh_arch, gpu, torch.bfloat16)
    eng.load_module(model)
    images = [(synth.synth_scenes(1, S, S, seed=60 + i)[0].flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8)
              .contiguous() for i in range(2)]
    plain = Detector(eng, size=S, batch=2, tta=((1.0, False),)).predict(images)
    mirrored = Detector(eng, size=S, batch=2, tta=((1.0, True),)).predict([im.flip(1).contiguous() for im in images])
    a, b = plain.dets.cpu().numpy(), mirrored.dets.cpu().numpy()
    assert plain.counts.cpu().tolist() == mirrored.counts.cpu().tolist() and int(plain.counts.sum()) > 0
    assert np.array_equal(a[:, :, 4:], b[:, :, 4:])
    live = a[:, :, 4] > 0
    inside = live & (S - a[:, :, 2] >= 0) & (S - a[:, :, 0] <= S)
    assert inside.any()
    want = np.stack((S - a[:, :, 2], a[:, :, 1], S - a[:, :, 0], a[:, :, 3]), 2).astype(np.float64)
    assert np.abs(b[:, :, :4] - want)[inside].max() <= S * 2.0 ** -23
    with pytest.raises(ValueError, match="tile"):
        Detector(eng, size=S, batch=2, tile=64, tta=((1.0, True),))
