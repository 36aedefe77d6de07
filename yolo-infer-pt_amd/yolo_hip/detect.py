"""Detections in source-image coordinates, with optional tiled inference.

`yolo_hip.preprocess.letterbox` takes decoded images of any size and `nms` returns boxes in the
coordinates of the square network canvas. This module closes the loop:

  tiles           cut an image into overlapping crops (pure Python)
  tile_transform  the six floats that take a crop's canvas coordinates back to the source image
  merge           yh_merge / yh_merge_host: map the tile detections back and, for images of two
                  or more tiles, drop duplicates across tile borders with a second greedy NMS -
                  one launch for all images of a call
  Detector        images in, source-pixel detections out: crops as views of the device-resident
                  image, letterbox, DetectPipeline (yh_forward_u8 + yh_nms), one merge

There is no counterpart in the reference (it never leaves the canvas: main.py moves the labels
into canvas space instead, and it has no tiled inference); the semantics are those stated in
include/yolo_hip.h, pinned by the numpy restatement in tests/_merge_cases.py.

Limits: duplicates are merged by IoU only - there is no intersection-over-smaller rule, and
boxes that touch an interior tile edge (objects cut by the tile) are not dropped.
"""
import ctypes

import numpy as np
import torch

from ._lib import MERGE_MAX_CAND


def _starts(length, tile, step):
    if length <= tile:
        return [0]
    s = list(range(0, length - tile + 1, step))
    if s[-1] != length - tile:
        s.append(length - tile)     # the regular grid stops short of the edge
    return s


def tiles(height, width, tile, overlap=0.2, full_image=False):
    """Crops (x0, y0, w, h) of a height x width image for tiled inference, row-major.

    An image no larger than tile x tile is one crop, the whole image. Otherwise every crop is
    min(tile, width) x min(tile, height) and lies inside the image; starts advance by
    step = tile - int(tile * overlap) from 0, with a last start at width - tile (height - tile)
    where the regular grid stops short of the edge. full_image=True appends the whole image as a
    last crop when there is more than one."""
    height, width, tile = int(height), int(width), int(tile)
    if height < 1 or width < 1 or tile < 1:
        raise ValueError("yolo_hip.tiles: height, width and tile must be positive")
    if not 0.0 <= overlap < 1.0:
        raise ValueError("yolo_hip.tiles: overlap must be in [0, 1)")
    if height <= tile and width <= tile:
        return [(0, 0, width, height)]
    step = tile - int(tile * overlap)
    w, h = min(tile, width), min(tile, height)
    crops = [(x0, y0, w, h) for y0 in _starts(height, tile, step) for x0 in _starts(width, tile, step)]
    if full_image and len(crops) > 1:
        crops.append((0, 0, width, height))
    return crops


def tile_transform(crop, size):
    """(sx, sy, px, py, ox, oy) as np.float32 for one crop (x0, y0, w, h) letterboxed to size x size
    (size an int) or to an H x W canvas (size = (H, W)):
    a canvas coordinate x maps to (x - px) * sx + ox in the source image (y alike). The scale is
    the fp32 quotient w / new_w of preprocess.geometry, exactly 1.0 when the crop is not resized."""
    from .preprocess import geometry
    x0, y0, w, h = (int(v) for v in crop)
    nh, nw, top, left = geometry(h, w, size)
    return (np.float32(w) / np.float32(nw), np.float32(h) / np.float32(nh), np.float32(left), np.float32(top),
            np.float32(x0), np.float32(y0))


def _check(name, t, shape, dtype, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"yolo_hip.merge: {name} must be a tensor")
    if t.dtype != dtype:
        raise TypeError(f"yolo_hip.merge: {name} must be {dtype}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"yolo_hip.merge: {name} is on {t.device}, expected {device}")
    if len(shape) != t.dim() or any(w is not None and w != g for w, g in zip(shape, t.shape)):
        want = tuple("*" if w is None else w for w in shape)
        raise ValueError(f"yolo_hip.merge: {name} has shape {tuple(t.shape)}, expected {want}")
    if not t.is_contiguous():
        raise ValueError(f"yolo_hip.merge: {name} must be contiguous")


def merge(dets, counts, tile_xf, tile_offsets, image_wh, max_tiles, iou=0.65, max_out=300, out=None, threads=0):
    """Tile detections -> source-image detections, all images of a call in one launch.

    dets (T, max_det, 6) f32 and counts (T,) i32 as `nms` returns them for the tile batch (rows at
    or beyond counts[t] are never read); tile_xf (T, 6) f32 rows of `tile_transform`; tile_offsets
    (N + 1,) i32 ascending - image i owns tiles tile_offsets[i]:tile_offsets[i + 1], tiles beyond
    the last offset (batch padding) are never visited; image_wh (N, 2) f32 (W, H); max_tiles: a
    bound on the tiles of one image, max_tiles * max_det <= MERGE_MAX_CAND. All on one device, all
    contiguous.
    -> (out (N, max_out, 6) f32, out_counts (N,) i32); out=(out, out_counts) reuses buffers. Every
    byte is written, rows beyond the count are 0.

    An image of one tile gets the plain inverse letterbox (clipped to the image, empty boxes
    dropped, input order); an image of several tiles additionally a greedy NMS at `iou` between
    equal classes (include/yolo_hip.h). cuda tensors run the HIP kernel (yh_merge) asynchronously
    on the current stream, CPU tensors the host twin (yh_merge_host, `threads` <= 0: every
    hardware thread)."""
    from ._lib import check, lib
    if not isinstance(dets, torch.Tensor) or dets.dim() != 3:
        raise ValueError("yolo_hip.merge: dets must be a (T, max_det, 6) tensor")
    dev = dets.device
    T, md = dets.shape[0], dets.shape[1]
    _check("dets", dets, (T, md, 6), torch.float32, dev)
    _check("counts", counts, (T,), torch.int32, dev)
    _check("tile_xf", tile_xf, (T, 6), torch.float32, dev)
    _check("tile_offsets", tile_offsets, (None,), torch.int32, dev)
    if tile_offsets.shape[0] < 1:
        raise ValueError("yolo_hip.merge: tile_offsets must hold images + 1 entries")
    N = tile_offsets.shape[0] - 1
    _check("image_wh", image_wh, (N, 2), torch.float32, dev)
    max_out = int(max_out)
    if out is None:
        o = torch.empty((N, max(max_out, 0), 6), dtype=torch.float32, device=dev)
        oc = torch.empty((N,), dtype=torch.int32, device=dev)
    else:
        o, oc = out
        _check("out", o, (N, max_out, 6), torch.float32, dev)
        _check("out_counts", oc, (N,), torch.int32, dev)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    args = (ptr(dets), ptr(counts), T, md, ptr(tile_xf), ptr(tile_offsets), ptr(image_wh), N, int(max_tiles),
            ctypes.c_double(iou), max_out, ptr(o), ptr(oc))
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(lib().yh_merge(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "merge")
    elif dev.type == "cpu":
        check(lib().yh_merge_host(*args, int(threads)), "merge_host")
    else:
        raise ValueError(f"yolo_hip.merge: unsupported device {dev}")
    return o, oc


class Detections:
    """Result of Detector.predict: dets (n, max_det, 6) f32 = x1, y1, x2, y2, score, class in source
    pixels and counts (n,) i32, both on the device; rows beyond an image's count are 0. frames:
    the device-resident sources of predict(..., keep_frames=True) (BGR tensors and NV12 objects,
    what preprocess.crop_rois takes), else None."""

    def __init__(self, dets, counts, frames=None):
        self.dets = dets
        self.counts = counts
        self.frames = frames

    def __len__(self):
        return self.dets.shape[0]

    def tolist(self):
        """Per-image (k, 6) tensors (reads counts on the host: synchronises the current stream)."""
        return [self.dets[i, :k] for i, k in enumerate(self.counts.tolist())]


class Detector:
    """Images of any size in, detections in source pixels out.

    engines: one Engine or a list of Engines with the same weights (DetectPipeline lanes).
    size: the square network canvas; batch: tiles per forward. tile=None: every image is
    letterboxed whole (one tile), so the result is `nms` followed by the inverse letterbox.
    tile=T: images larger than T x T are cut with tiles(h, w, T, overlap, full_image), every crop
    is letterboxed to the canvas, and the tiles of an image are merged at merge_iou (default: iou).
    conf / iou / tile_max_det are the per-tile NMS's thresholds and max_det; tile_max_det defaults
    to min(max_det, MERGE_MAX_CAND // most tiles of one image in the call). max_det rows per image
    come back.

    canvas=(H, W) (both multiples of 32, e.g. preprocess.rect_canvas(1080, 1920) = (384, 640))
    replaces the square canvas by a rectangle: the pipeline is built at that shape and every tile
    is letterboxed to it (preprocess.letterbox_frames). canvas=None is (size, size). predict()
    also takes preprocess.NV12 frames (image height and width are the planes'); they cannot be
    tiled (crops at odd offsets are out of scope): with `tile` set they raise ValueError.

    predict() never reads a device value on the host: sizes, tile lists and transforms come from
    the images' shapes. Stream safety, as yolo_hip.evaluate.Evaluator documents its own: the
    tile batches are forwarded on the pipeline's streams; predict() makes the caller's stream
    wait on every batch's `done` event before the merge runs there (no device synchronisation),
    so the returned tensors, allocated on the caller's stream, are safe to read on it as soon
    as predict() returns. Temporaries that another stream touches are record_stream'ed. One
    Detector serves one caller stream at a time.
    """

    def __init__(self, engines, size=640, batch=32, tile=None, overlap=0.2, full_image=False, conf=0.001, iou=0.65,
                 merge_iou=None, max_det=300, tile_max_det=None, canvas=None):
        from .pipeline import DetectPipeline
        self.size, self.batch = int(size), int(batch)
        self.tile = None if tile is None else int(tile)
        self.overlap, self.full_image = float(overlap), bool(full_image)
        self.conf, self.iou = float(conf), float(iou)
        self.merge_iou = self.iou if merge_iou is None else float(merge_iou)
        self.max_det = int(max_det)
        self.tile_max_det = None if tile_max_det is None else int(tile_max_det)
        if self.batch < 1 or self.max_det < 1:
            raise ValueError("yolo_hip.Detector: batch and max_det must be positive")
        if canvas is None:
            self.canvas = None
            ch = cw = self.size
        else:
            ch, cw = (int(v) for v in canvas)
            if ch < 32 or cw < 32 or ch % 32 or cw % 32:
                raise ValueError("yolo_hip.Detector: canvas sides must be positive multiples of 32")
            self.canvas = (ch, cw)
        self.pipe = DetectPipeline(engines, self.batch, ch, cw)
        self.device = self.pipe.eng.device

    def plan(self, shapes):
        """[(height, width), ...] -> (crops per image, tile_max_det, max_tiles): what predict() does
        with images of these shapes (host only)."""
        crops = [tiles(h, w, self.tile, self.overlap, self.full_image) if self.tile is not None else [(0, 0, w, h)]
                 for h, w in shapes]
        max_tiles = max((len(c) for c in crops), default=1)
        tmd = self.tile_max_det
        if tmd is None:
            tmd = min(self.max_det, MERGE_MAX_CAND // max_tiles)
        if tmd < 1 or tmd * max_tiles > MERGE_MAX_CAND:
            raise ValueError(f"yolo_hip.Detector: {max_tiles} tiles per image x tile_max_det {tmd} does not fit "
                             f"MERGE_MAX_CAND = {MERGE_MAX_CAND}; use larger tiles or less overlap")
        return crops, tmd, max_tiles

    def predict(self, images, keep_frames=False):
        """images -> Detections. keep_frames=True also returns the device-resident sources as
        `.frames`, so preprocess.crop_rois(det.frames, det.dets, det.counts, ...) needs no second
        upload."""
        from .preprocess import NV12, letterbox, letterbox_frames
        dev = self.device
        srcs, shapes = [], []
        for im in images:
            if isinstance(im, NV12):
                if self.tile is not None:
                    raise ValueError("yolo_hip.Detector: NV12 frames cannot be tiled (tile must be None)")
                srcs.append(im.to(dev, non_blocking=True))
                shapes.append((im.height, im.width))
                continue
            t = torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError("yolo_hip.Detector: images must be (h, w, 3) uint8 BGR or preprocess.NV12")
            if t.stride(2) != 1 or t.stride(1) != 3:
                t = t.contiguous()
            srcs.append(t.to(dev, non_blocking=True))
            shapes.append((t.shape[0], t.shape[1]))
        n = len(srcs)
        crops, tmd, max_tiles = self.plan(shapes)
        if n == 0:
            return Detections(torch.zeros((0, self.max_det, 6), dtype=torch.float32, device=dev),
                              torch.zeros((0,), dtype=torch.int32, device=dev), [] if keep_frames else None)
        canvas = ch, cw = self.canvas or (self.size, self.size)
        # host-side geometry of every tile, uploaded as one pinned block (below):
        # [xf (padded tile axis) x 6 | wh n x 2 | offsets n + 1 (i32)]
        views, xf, offsets = [], [], [0]
        for t, cs in zip(srcs, crops):
            for c in cs:
                x0, y0, w, h = c
                views.append(t if isinstance(t, NV12) else t[y0:y0 + h, x0:x0 + w])   # an NV12 frame is one whole tile
                xf.append(tile_transform(c, canvas))
            offsets.append(len(views))
        T = len(views)
        B = self.batch
        nb = (T + B - 1) // B
        TP = nb * B                              # the tile axis, padded to whole batches
        stage = torch.zeros(6 * TP + 2 * n + n + 1, dtype=torch.float32, pin_memory=True)
        stage[:6 * T].view(T, 6).copy_(torch.from_numpy(np.asarray(xf, dtype=np.float32).reshape(T, 6)))
        stage[6 * TP:6 * TP + 2 * n].view(n, 2).copy_(torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32))
        stage[6 * TP + 2 * n:].view(torch.int32).copy_(torch.tensor(offsets, dtype=torch.int32))
        on = stage.to(dev, non_blocking=True)
        tile_xf = on[:6 * TP].view(TP, 6)
        image_wh = on[6 * TP:6 * TP + 2 * n].view(n, 2)
        tile_offsets = on[6 * TP + 2 * n:].view(torch.int32)

        pipe = self.pipe
        pipe.nms_kwargs = dict(confidence_threshold=self.conf, iou_threshold=self.iou, max_det=tmd)
        # the pad tiles are blank canvases that no image references
        tdets = torch.empty((TP, tmd, 6), dtype=torch.float32, device=dev)
        tcounts = torch.empty((TP,), dtype=torch.int32, device=dev)
        if pipe.nms_stream is not None:          # written there, allocated (and merged) here
            tdets.record_stream(pipe.nms_stream)
            tcounts.record_stream(pipe.nms_stream)
        with torch.cuda.device(dev):
            done = []
            for b in range(nb):
                part = views[b * B:(b + 1) * B]
                x = torch.empty((B, 3, ch, cw), dtype=torch.uint8, device=dev)
                if self.canvas is None and not any(isinstance(v, NV12) for v in part):
                    letterbox(part, self.size, device=dev, out=x[:len(part)])
                else:
                    letterbox_frames(part, canvas, device=dev, out=x[:len(part)])
                if len(part) < B:
                    x[len(part):].zero_()
                done.append(pipe.submit(x, out=(tdets[b * B:(b + 1) * B], tcounts[b * B:(b + 1) * B]))[3])
            for e in done:
                pipe.wait(e)
            out = merge(tdets, tcounts, tile_xf, tile_offsets, image_wh, max_tiles, iou=self.merge_iou,
                        max_out=self.max_det)
        return Detections(*out, srcs if keep_frames else None)
