"""yolo_hip.detect.Detector end to end on the device at the smallest shapes (v11_n bf16, synth
weights, size 320, batch 4): predict() against the same tiles run one batch at a time through
letterbox, Engine.forward, nms, a download and yh_merge_host - exactly - in tiled mode and with
tile=None (nms plus the numpy map-back), and the stream safety of results read late. Marked gpu.
"""
import numpy as np
import pytest
import torch

import _merge_cases as mc
from yolo_hip import synth
from yolo_hip.detect import Detector, merge, tile_transform, tiles

pytestmark = pytest.mark.gpu

SIZE, BATCH, CONF, IOU, MAX_DET = 320, 4, 0.001, 0.65, 300
SHAPES = ((416, 544), (320, 320), (200, 300))


def _images(seed):
    """uint8 HWC BGR images of SHAPES from synth_scenes."""
    out = []
    for i, (h, w) in enumerate(SHAPES):
        x = synth.synth_scenes(1, h, w, seed=seed + i)[0]                     # (3, h, w) RGB in [0, 1]
        out.append((x.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous())
    return out


@pytest.fixture(scope="module")
def engines(gpu):
    from nets import nn
    from yolo_hip.engine import Engine
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    engs = []
    for _ in range(2):
        e = Engine(*model._yh_arch, gpu, torch.bfloat16)
        e.load_module(model)
        engs.append(e)
    return engs


def _tile_dets(engine, gpu, images, tile, overlap=0.25):
    """The sequential restatement up to the merge: -> (crops per image, dets (T, tmd, 6), counts (T,)) on the
    CPU, one forward batch of BATCH tiles at a time (the last padded with blank canvases)."""
    from yolo_hip.engine import nms
    from yolo_hip.preprocess import letterbox
    crops = [tiles(h, w, tile, overlap) if tile else [(0, 0, w, h)] for h, w in SHAPES]
    tmd = min(MAX_DET, mc.CAP // max(len(c) for c in crops))
    views = [im.to(gpu)[y0:y0 + h, x0:x0 + w] for im, cs in zip(images, crops) for (x0, y0, w, h) in cs]
    dets, counts = [], []
    for b in range(0, len(views), BATCH):
        part = views[b:b + BATCH]
        x = torch.zeros((BATCH, 3, SIZE, SIZE), dtype=torch.uint8, device=gpu)
        letterbox(part, SIZE, device=gpu, out=x[:len(part)])
        d, c = nms(engine.forward(x), confidence_threshold=CONF, iou_threshold=IOU, max_det=tmd)
        dets.append(d.cpu()[:len(part)])
        counts.append(c.cpu()[:len(part)])
    return crops, torch.cat(dets, 0), torch.cat(counts, 0)


@pytest.fixture(scope="module")
def expected(gpu, engines):
    """seed -> (dets (3, MAX_DET, 6), counts (3,)) numpy, tiled 320 / 0.25; computed once, never modified."""
    want = {}
    for seed in (40, 50):
        crops, d, c = _tile_dets(engines[0], gpu, _images(seed), 320)
        assert [len(cs) for cs in crops] == [4, 1, 1]
        xf = torch.from_numpy(np.asarray([tile_transform(cr, SIZE) for cs in crops for cr in cs], np.float32))
        off = torch.tensor(np.cumsum([0] + [len(cs) for cs in crops]), dtype=torch.int32)
        wh = torch.tensor([[w, h] for h, w in SHAPES], dtype=torch.float32)
        out, cnt = merge(d.contiguous(), c.contiguous(), xf, off, wh, 4, iou=IOU, max_out=MAX_DET)   # yh_merge_host
        want[seed] = (out.numpy(), cnt.numpy(), c.numpy())
    return want


def _same(res, want):
    return (np.array_equal(res.counts.cpu().numpy(), want[1])
            and res.dets.cpu().numpy().tobytes() == want[0].tobytes())


def test_tiled_predict_equals_the_sequential_restatement(gpu, engines, expected):
    det = Detector(engines[0], size=SIZE, batch=BATCH, tile=320, overlap=0.25, conf=CONF, iou=IOU, max_det=MAX_DET)
    res = det.predict(_images(40))
    out, cnt, tile_counts = expected[40]
    assert res.dets.shape == (3, MAX_DET, 6) and res.counts.shape == (3,) and res.dets.is_cuda
    assert int(cnt.sum()) > 0 and (tile_counts > 0).all()          # the synthetic head fills its tiles
    assert (cnt[0] < tile_counts[:4].sum()) or cnt[0] == MAX_DET   # image 0 was merged from 4 tiles
    assert _same(res, expected[40])
    per = res.tolist()
    assert [p.shape[0] for p in per] == cnt.tolist()
    for p, (h, w) in zip(per, SHAPES):                              # source pixels, inside the image
        p = p.cpu().numpy()
        assert (p[:, :2] >= 0).all() and (p[:, 2] <= w).all() and (p[:, 3] <= h).all()
    # host images (numpy) give the same result
    assert _same(det.predict([im.numpy() for im in _images(40)]), expected[40])


def test_untiled_predict_is_nms_plus_the_map_back(gpu, engines):
    images = _images(40)
    crops, d, c = _tile_dets(engines[0], gpu, images, None)
    assert d.shape[0] == 3 and int(c.sum()) > 0
    det = Detector(engines[0], size=SIZE, batch=BATCH, conf=CONF, iou=IOU, max_det=MAX_DET)
    res = det.predict(images)
    got, cnt = res.dets.cpu().numpy(), res.counts.cpu().numpy()
    for i, (h, w) in enumerate(SHAPES):
        rows, keep = mc.map_rows(d[i, :int(c[i])].numpy(), tile_transform((0, 0, w, h), SIZE), w, h)
        rows = rows[keep][:MAX_DET]
        assert cnt[i] == len(rows) and np.array_equal(got[i, :len(rows)], rows) and not got[i, len(rows):].any()


@pytest.mark.parametrize("lanes", [1, 2])
def test_results_read_late_are_intact(gpu, engines, expected, lanes):
    det = Detector(engines[:lanes] if lanes > 1 else engines[0], size=SIZE, batch=BATCH, tile=320, overlap=0.25,
                   conf=CONF, iou=IOU, max_det=MAX_DET)
    a_in, b_in = _images(40), _images(50)
    first = det.predict(a_in)
    second = det.predict(b_in)          # reuses the pipeline's buffers and the allocator's blocks
    del a_in, b_in
    assert _same(second, expected[50])
    assert _same(first, expected[40])
    assert not np.array_equal(expected[40][0], expected[50][0])


def test_too_many_tiles_is_a_value_error(gpu, engines):
    det = Detector(engines[0], size=SIZE, batch=BATCH, tile=32, overlap=0.0)
    with pytest.raises(ValueError, match="MERGE_MAX_CAND"):
        side = 32 * (int(mc.CAP ** 0.5) + 1)
        det.plan([(side, side)])                                     # more tiles of one image than candidates
