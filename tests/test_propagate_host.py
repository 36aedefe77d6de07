"""Track propagation on the host (yh_propagate_remember_host, yh_propagate_host; CPU only): the twin
against the numpy restatement of tests/_propagate_cases.py bit for bit - outputs and the state after
every step -, the planted shifts as known answers, the tracker fed by a `Propagator` over a stream
whose detector runs on every third frame, the ABI and the argument errors.
tests/test_gpu_propagate.py holds the kernels to this twin.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _motion_cases as mc
import _propagate_cases as pc
from yolo_hip import _lib
from yolo_hip import propagate as yp
from yolo_hip import track as yt


@pytest.mark.parametrize("name", list(pc.CASES))
def test_host_twin_matches_restatement(name):
    want = pc.reference(name)
    pc.same(pc.run(name, threads=1), want, name)
    if name.startswith("batch"):
        pc.same(pc.run(name, threads=3), want, name + " threads 3")
    if name in ("batch70", "batch-over"):
        first = want[1][0][3]
        assert 0 < first.max() < 70, "the gate must drop some entries and keep others"


@pytest.mark.parametrize("name", [n for n in pc.CASES if n.startswith("shift") or n.startswith("radius") or n == "flat"])
def test_planted_shift_is_recovered(name):
    c = pc.case(name)
    (dets, ids, sad, counts), state = pc.run(name)[1]
    e = state[0, pc.HDR:].view(pc.ENTRY)[0]
    if name == "shift-beyond":       # beyond the radius: whatever comes out carries its real SAD or is gated
        assert counts[0] == 0 or sad[0, 0] > 0
        return
    assert counts[0] == 1 and sad[0, 0] == 0 and ids[0, 0] == 1
    assert (e["ox"] - e["ox0"], e["oy"] - e["oy0"]) == c["planted"]
    moved = dets[0, 0, :4] - c["steps"][0][2][0][0, 0, :4]
    assert np.abs(moved - np.array(c["planted"] * 2, np.float32)).max() <= max(e["cw"], e["ch"]) / 2
    if name == "flat":
        assert moved.tolist() == [0, 0, 0, 0]


# (frame h, w), (box w, h), the start and the velocity (px a frame) of every object
FAST = ((240, 320), (40, 48), [[30, 60], [150, 130], [240, 60]], [[6, 13], [0, -14], [-7, 12]])
LARGE = ((720, 960), (288, 320), [[100, 220], [560, 180]], [[9, -7], [-8, 10]])


def _scene(size, box, start, vel, frames=13):
    """Textured rectangles on a textured background; they reverse after frame 4, inside a gap of a
    detector that runs on every third frame -> per frame (BGR frame, boxes (n, 4))."""
    bg = mc.world(61, *size)
    tex = [mc.world(62 + k, box[1], box[0]) for k in range(len(start))]
    pos, vel, out = np.array(start, np.float32), np.array(vel, np.float32), []
    for i in range(frames):
        f = bg.copy()
        for k, (x, y) in enumerate(pos.astype(int)):
            f[y:y + box[1], x:x + box[0]] = tex[k]
        out.append((f, np.concatenate([pos, pos + np.array(box, np.float32)], 1)))
        pos = pos + (vel if i < 4 else -vel)
    return out


def _track_scene(scene, propagate, period=3):
    """-> (ids per frame, the ids the tracker has handed out, and per skipped frame the worst
    |propagated box - truth| along x and y in cells of the entry)."""
    n = len(scene[0][1])
    trk = yt.Tracker(1, "cpu", max_tracks=16)
    prop = yp.Propagator(1, "cpu", max_tracks=16, radius=8)
    ids, err = [], []
    for i, (f, boxes) in enumerate(scene):
        truth = torch.from_numpy(boxes)
        if i % period == 0:
            dets = torch.zeros((1, 8, 6))
            dets[0, :n, :4], dets[0, :n, 4] = truth, 0.9
            tracks = trk.update(dets, torch.tensor([n], dtype=torch.int32))
            prop.remember([f], tracks)
            order = tracks.det_index[0, :int(tracks.counts[0])].long()   # the truth row of every remembered track
        elif propagate:
            p = prop.propagate([f])
            assert int(p.counts[0]) == len(order)
            e = prop.state[0, pc.HDR:].numpy().view(pc.ENTRY)[:len(order)]
            d = (p.dets[0, :len(order), :4] - truth[order]).abs().numpy()
            err.append((float((d[:, 0::2].max(1) / e["cw"]).max()), float((d[:, 1::2].max(1) / e["ch"]).max())))
            tracks = trk.update(p.dets, p.counts)
        else:
            tracks = trk.update(torch.zeros((1, 8, 6)), torch.zeros((1,), dtype=torch.int32))
        ids.append(sorted(tracks.ids[0, :int(tracks.counts[0])].tolist()))
    return ids, int(trk.state[0, 1]), err


def test_propagated_boxes_stay_within_a_cell_of_the_truth():
    """Boxes of 288 x 320 (cells of 9 x 10 pixels) that move up to one cell a frame: every object keeps its
    id, and on every skipped frame every propagated box is within one cell of the truth along each
    axis. The propagated box is the remembered one - the tracker's filtered box - moved by the search,
    so its error is the filter's lag at the last detector frame plus the search's. After a reversal
    the filter lags by about 0.6 of the speed, which is why this scene is slow in cells. Coasting keeps
    the ids here as well: the control that loses them is the next test's, on a fast scene."""
    ids, handed, err = _track_scene(_scene(*LARGE), True)
    assert all(f == [1, 2] for f in ids) and handed == 2
    assert len(err) == 8 and max(max(e) for e in err) <= 1.0, err


def test_propagation_keeps_ids_where_coasting_loses_them():
    """Boxes of 40 x 48 (cells of 1 x 2 pixels) that move up to 7 cells a frame: with the propagated rows
    every object keeps its id in every frame; with no rows on the skipped frames the tracker coasts
    past the reversal, finds nothing where it predicted, and the objects are born again under new ids
    (which stay tentative, hence unreported). A coasted box misses a reversal by four frames of motion,
    and the IoU association gives up at about 0.4 of a box side, 13 cells: coasting loses an id only
    above 3 cells a frame, where the filter's lag (above) is about two cells. No scene shows both,
    hence two scenes; the boxes of this one are not held to the truth."""
    scene = _scene(*FAST)
    ids, handed, _ = _track_scene(scene, True)
    assert all(f == [1, 2, 3] for f in ids) and handed == 3
    control, handed, _ = _track_scene(scene, False)
    assert handed > 3 and any(f != [1, 2, 3] for f in control[3::3])


def test_abi_symbols_and_argument_errors():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "yolo_hip.h")).read()
    L = _lib.lib()
    for name in ("yh_propagate", "yh_propagate_host", "yh_propagate_remember", "yh_propagate_remember_host",
                 "yh_propagate_state_bytes", "yh_propagate_workspace_bytes"):
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib._PROTOS and hasattr(L, name)
    assert L.yh_abi_version() == _lib.ABI_VERSION == 7
    assert L.yh_propagate_state_bytes(3, 70) == 3 * (16 + 1088 * 70) and L.yh_propagate_state_bytes(1, 257) == 0
    assert L.yh_propagate_workspace_bytes(40, 70) == 32 * 70 * 32 and L.yh_propagate_workspace_bytes(1, 0) == 0
    import yolo_hip
    assert yolo_hip.Propagator is yp.Propagator and yolo_hip.Propagated is yp.Propagated
    img = np.zeros((36, 64, 3), np.uint8)
    state = yp.propagate_state(1, 4)
    state.fill_(0x5A)
    out = [np.full((1, 4, 6), -7, np.float32)] + [np.full(s, -7, np.int32) for s in ((1, 4), (1, 4), (1,))]
    ptr = [ctypes.c_void_p(a.ctypes.data) for a in out]

    def call(radius=2, mt=4, h=36, fmt=0, plane0=True, batch=1, counts=True):
        d = _lib.YhFrame(img.ctypes.data if plane0 else None, None, h, 64, 0, 0, fmt, 0)
        sp = ctypes.c_void_p(state.data_ptr())
        a = L.yh_propagate_host(ctypes.byref(d), batch, None, sp, 1, mt, radius, 24, 4, *ptr[:3], ptr[3] if counts else None, 1)
        if radius != 2:                  # remember takes no radius
            return a, -1
        return a, L.yh_propagate_remember_host(ctypes.byref(d), batch, None, ptr[0], ptr[1], ptr[3] if counts else None, 4,
                                               sp, 1, mt, 1)

    for kw in (dict(radius=0), dict(radius=17), dict(mt=0), dict(mt=257), dict(h=0), dict(fmt=7), dict(plane0=False),
               dict(batch=-1), dict(counts=False), dict(fmt=1, h=35)):
        a, b = call(**kw)
        assert a == -1 and b == -1 and L.yh_last_error(), kw
        assert all((o == -7).all() for o in out) and (state == 0x5A).all(), kw
    with pytest.raises(ValueError):
        yp.propagate([img], torch.zeros((1, 100), dtype=torch.uint8))
    with pytest.raises(ValueError):
        yp.Propagator(1, "cpu", radius=17)
