"""Frames -> detections -> tracks -> crops -> classes, device-resident (yolo_hip.Classifier). Marked gpu.

Synthetic 1080p BGR frames go through Detector.predict(keep_frames=True), Tracker.update,
crop_rois(size=(128, 64)) and Classifier.predict on a side stream with no host synchronisation in
between; the chunked result equals one call on crops.data, rows at or beyond total are masked and
crops.gather(tracks.ids) lines the track ids up with the classes."""
import pytest
import torch

import _cls_cases as cc
from _util import make_model
from yolo_hip import preprocess as pre, synth
from yolo_hip.classify import Classifier
from yolo_hip.detect import Detector
from yolo_hip.engine import Engine
from yolo_hip.track import Tracker

pytestmark = pytest.mark.gpu


def _frame(h, w, seed):
    x = synth.synth_scenes(1, h, w, seed=seed)[0]
    return (x.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous()   # BGR HWC


def test_detect_track_crop_classify(gpu):
    det_model = make_model("n")
    eng = Engine(*det_model._yh_arch, gpu, torch.bfloat16)
    eng.load_module(det_model)
    max_det = 12
    det = Detector(eng, size=640, batch=2, conf=0.001, iou=0.65, max_det=max_det)
    trk = Tracker(2, gpu, track_high=0.001, track_low=0.0005, track_new=0.001)
    model = cc.make_model("n", 10)
    chunked = Classifier(model, gpu, torch.bfloat16, max_batch=16)
    whole = Classifier(model, gpu, torch.bfloat16, max_batch=2 * max_det)
    frames = [_frame(1080, 1920, 71), _frame(1080, 1920, 72)]

    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):
        d = det.predict(frames, keep_frames=True)
        trk.update(d)
        t = trk.update(d)                                            # the second frame confirms the tracks
        crops = pre.crop_rois(d.frames, t.dets, t.counts, (128, 64))
        got = chunked.predict(crops, embed=True)
        ids = crops.gather(t.ids)
        done = torch.cuda.Event()
        done.record(side)
    # everything above was enqueued on the side stream: its event is all the comparison waits for
    done.synchronize()

    cap = 2 * t.dets.shape[1]
    n = int(crops.total[0])
    assert crops.data.shape == (cap, 3, 128, 64) and 0 < n <= cap and n == int(t.counts.sum())
    assert got.probs.shape == (cap, 10) and got.embed.shape == (cap, 1280) and int(got.total[0]) == n
    one = whole.predict(crops.data, embed=True)
    assert torch.equal(got.probs[:n], one.probs[:n]) and torch.equal(got.embed[:n], one.embed[:n])
    assert torch.equal(got.top1[:n], one.top1[:n]) and torch.equal(got.conf[:n], one.conf[:n])
    assert not got.probs[n:].any() and not got.embed[n:].any() and not got.conf[n:].any()
    assert (got.top1[n:] == -1).all()
    assert torch.equal(got.top1[:n].long(), got.probs[:n].argmax(1)) and (got.conf[:n] > 0.09).all()
    assert torch.allclose(got.probs[:n].sum(1), torch.ones(n, device=gpu), atol=1e-5)
    # track ids follow their classes: slot i is row rois[i, 1] of frame rois[i, 0]
    rois = crops.rois[:n].cpu().tolist()
    want = [int(t.ids[r[0], r[1]]) for r in rois]
    assert ids[:n].cpu().tolist() == want and all(i >= 1 for i in want)
