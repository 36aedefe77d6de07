"""yh_fuse_host (csrc/fuse_host.cpp) through yolo_hip.fuse_boxes on CPU tensors against the float64
reference of tests/_fuse_cases.py: the same clusters in the same order, boxes and scores within the
rounding an fp32 accumulation of n members allows; the argument errors; the geometry of a mirrored,
scaled test-time-augmentation pass.
"""
import ctypes

import numpy as np
import pytest
import torch

import _fuse_cases as fc
from yolo_hip import _lib, fuse_boxes
from yolo_hip.detect import pass_transform
from yolo_hip.preprocess import geometry

KEYS = ("dets", "counts", "group_xf", "group_weight", "group_offsets", "image_wh")


def run(c, dev="cpu", threads=0):
    N = c["image_wh"].shape[0]
    out = torch.full((N, c["max_out"], 6), -7.0, device=dev)        # reused buffers: every byte is written
    cnt = torch.full((N,), -7, dtype=torch.int32, device=dev)
    fuse_boxes(*[c[k].to(dev) for k in KEYS], c["max_groups"], iou=c["iou"], skip_score=c["skip_score"],
               max_out=c["max_out"], out=(out, cnt), threads=threads)
    return out, cnt


@pytest.mark.parametrize("name", fc.ALL)
def test_fuse_host_equals_the_reference(name):
    """Membership exactly; a coordinate within (n + 4) * 2**-23 * max(W, H) and the score within the
    same relative bound: n rounded products and n adds of the sums, one division and the slack of
    the divisor's own n roundings, half an ulp each of a value no larger than S * max(W, H)."""
    c = fc.case(name)
    out, cnt = (t.numpy() for t in run(c))
    assert np.isfinite(out).all()                                   # no NaN row or padding group was read
    for i, want in enumerate(c["want"]):
        want = np.asarray(want, np.float64).reshape(-1, 7)
        got = out[i, :cnt[i]].astype(np.float64)
        assert cnt[i] == len(want) and not out[i, cnt[i]:].any()
        assert np.array_equal(got[:, 5], want[:, 0]), "classes, in order"
        bound = (want[:, 1] + 4) * 2.0 ** -23
        assert (np.abs(got[:, :4] - want[:, 2:6]).max(1, initial=0) <= bound * c["image_wh"][i].max().item()).all()
        assert (np.abs(got[:, 4] - want[:, 6]) <= bound * want[:, 6]).all()
    if name == "mixed":     # by hand: the triple, the clipped box, the pair (its neighbour stays alone), the tie, two alone
        assert [w[1] for w in c["want"][0]] == [3, 1, 2, 3, 1, 1] and cnt.tolist() == [6, 0, 0, 1]
    if name == "max_out":
        assert cnt.tolist() == [12, 3]


def test_threads_and_fresh_buffers_give_the_same_bytes():
    c = fc.case("max_out")
    a, ac = run(c, threads=1)
    b, bc = fuse_boxes(*[c[k] for k in KEYS], c["max_groups"], max_out=c["max_out"], threads=4)
    assert a.numpy().tobytes() == b.numpy().tobytes() and ac.tolist() == bc.tolist()


def test_bad_arguments_are_einval():
    lib = _lib.lib()
    t = torch.ones((64,))
    z, o = torch.zeros((64,), dtype=torch.int32), torch.zeros((64,))
    p, q, out = (ctypes.c_void_p(v.data_ptr()) for v in (t, z, o))

    def call(dets=p, counts=q, groups=1, md=4, xf=p, wt=p, off=q, wh=p, images=1, max_groups=1, max_out=2, out=out, oc=out):
        return lib.yh_fuse_host(dets, counts, groups, md, xf, wt, off, wh, images, max_groups, 0.55, 0.0, max_out, out, oc, 1)

    assert call() == 0
    for kw, word in ((dict(groups=-1), b"groups"), (dict(md=-1), b"max_det"), (dict(images=-1), b"images"),
                     (dict(max_out=-1), b"max_out"), (dict(max_groups=0), b"max_groups"),
                     (dict(max_groups=fc.CAP // 4 + 1), b"YH_FUSE_MAX_CAND"), (dict(dets=None), b"null"),
                     (dict(counts=None), b"null"), (dict(xf=None), b"null"), (dict(wt=None), b"null"),
                     (dict(off=None), b"null"), (dict(wh=None), b"null"), (dict(out=None), b"null"), (dict(oc=None), b"null")):
        assert call(**kw) == -1 and word in lib.yh_last_error(), (kw, lib.yh_last_error())
    z[1] = 1                                                        # the image now owns group 0 ...
    assert call() == 0 and call(wt=q) == -1 and b"group_weight" in lib.yh_last_error()      # ... whose weight is 0
    c = fc.case("mixed")
    with pytest.raises(RuntimeError, match="YH_FUSE_MAX_CAND"):
        fuse_boxes(*[c[k] for k in KEYS], fc.CAP)
    with pytest.raises(TypeError, match="group_weight"):
        fuse_boxes(*[c[k].double() if k == "group_weight" else c[k] for k in KEYS], 3)


def test_mirrored_scaled_pass_maps_back_to_the_frame():
    """A 1080 x 1920 frame letterboxed onto a 0.83-scale canvas and flipped: the letterboxed corners,
    seen in the flipped canvas, go back to the frame's corners within 1e-3 px through yh_fuse_host."""
    H, W, canvas = 1080, 1920, (320, 544)
    nh, nw, top, left = geometry(H, W, canvas)
    f = pass_transform(H, W, canvas, mirror=True)
    assert f[0] < 0 and f[1] > 0
    seen = [canvas[1] - (left + nw), top, canvas[1] - left, top + nh, 0.5, 0]     # x1 < x2, as an NMS writes it
    out, cnt = fuse_boxes(torch.tensor([[seen]], dtype=torch.float32), torch.ones(1, dtype=torch.int32),
                          torch.tensor([f]), torch.ones(1), torch.tensor([0, 1], dtype=torch.int32),
                          torch.tensor([[W, H]], dtype=torch.float32), 1)
    assert cnt.tolist() == [1]
    assert np.abs(out[0, 0, :4].numpy().astype(np.float64) - [0, 0, W, H]).max() <= 1e-3
