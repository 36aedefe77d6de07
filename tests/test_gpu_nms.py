"""On-device NMS (yh_nms) vs the reference goldens and the oracle. Marked gpu.

Bar: bit-exact kept rows (x1, y1, x2, y2, score, class) and counts for float32
head outputs; for 16-bit outputs, bit-exact against the oracle run with the same
dtype rounding of threshold and wh2xy corners.

The second half runs the named case list of tests/_nms_cases.py (one case per selection path
of csrc/nms.hip) through engine.nms(out=, workspace=) on caller-owned, poisoned buffers.
"""
import numpy as np
import pytest
import torch

import _nms_cases as cases
from _util import golden_name
from conftest import load_golden
from oracle import nms as onms
from yolo_hip import synth

pytestmark = pytest.mark.gpu


def _gpu_nms(y, dev, **kw):
    from yolo_hip.engine import nms
    dets, counts = nms(y.to(dev), **kw)
    counts = counts.cpu().tolist()
    dets = dets.cpu().numpy()
    return [dets[i, :c] for i, c in enumerate(counts)]


def _unpack(counts, flat):
    out, o = [], 0
    for c in counts:
        out.append(flat[o:o + c])
        o += c
    return out


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, f"image {i}: kept {a.shape[0]} vs {b.shape[0]}"
        np.testing.assert_array_equal(a, b, err_msg=f"image {i}")


def test_matches_reference_golden_synthetic(gpu):
    g = load_golden("nms_synth.npz")
    y = torch.stack([synth.synth_head_output(8400, 80, seed=int(s), mode=str(m))
                     for m, s in zip(g["modes"], g["seeds"])])
    _assert_same(_gpu_nms(y, gpu), _unpack(g["counts"], g["dets"]))


def test_matches_reference_golden_on_model_output(gpu):
    g = load_golden("nms_forward_n640.npz")
    y = torch.from_numpy(load_golden(golden_name("n", 640, 1))["y"])
    _assert_same(_gpu_nms(y, gpu), _unpack(g["counts"], g["dets"]))


@pytest.mark.parametrize("seed", range(6))
def test_random_cases_vs_oracle(gpu, seed):
    rng = np.random.default_rng(seed)
    B = int(rng.integers(1, 4))
    A = int(rng.integers(50, 3000))
    nc = int(rng.choice([1, 3, 80]))
    y = np.empty((B, 4 + nc, A), np.float32)
    y[:, 0:2] = rng.uniform(0, 320, size=(B, 2, A))
    y[:, 2:4] = rng.uniform(2, 120, size=(B, 2, A))
    s = 1 / (1 + np.exp(-rng.normal(-4, 3, size=(B, nc, A))))
    if seed % 2:  # heavy ties: quantised scores
        s = np.round(s * 64) / 64
    y[:, 4:] = s.astype(np.float32)
    kw = dict(confidence_threshold=float(rng.choice([0.001, 0.05, 0.3])), iou_threshold=float(rng.choice([0.3, 0.5, 0.65, 0.9])),
              max_det=int(rng.choice([1, 17, 300])), max_nms=int(rng.choice([50, 5000, 30000])))
    want = onms.non_max_suppression(y, kw["confidence_threshold"], kw["iou_threshold"], kw["max_det"], kw["max_nms"])
    got = _gpu_nms(torch.from_numpy(y), gpu, **kw)
    _assert_same(got, want)


@pytest.mark.parametrize("case", ["small_max_wh", "huge_boxes"])
def test_cross_class_overlap_vs_oracle(gpu, case):
    """Boxes of different classes overlap after the class offset (max_wh below the coordinate
    range, or boxes wider than max_wh / 2): the same-class shortcut of the IoU mask must not
    apply, and cross-class suppression must match the oracle."""
    y, max_wh = cases.cross_class_overlap(case)
    for iou in (0.3, 0.65):
        want = onms.non_max_suppression(y, 0.001, iou, 300, 30000, max_wh=max_wh)
        _assert_same(_gpu_nms(torch.from_numpy(y), gpu, iou_threshold=iou, max_wh=max_wh), want)


def test_empty_and_ragged_batch(gpu):
    y = torch.zeros(3, 84, 500)
    y[:, 2:4] = 20.0
    y[1, 4 + 2, 7] = 0.9
    y[1, 0:2, 7] = 100.0
    got = _gpu_nms(y, gpu)
    assert [g.shape[0] for g in got] == [0, 1, 0]
    np.testing.assert_array_equal(got[1], np.array([[90, 90, 110, 110, 0.9, 2]], np.float32))


def test_many_candidates_multiple_select_batches(gpu):
    """Every pair is a candidate (>4096 per image). By _nms_cases.census these inputs take a first batch
    of up to 2048 entries and, for the second image, up to 43 fast later batches; neither reaches the
    radix select (the case list below does)."""
    y = torch.stack([synth.synth_head_output(8400, 80, seed=9, mode="stress"),
                     synth.synth_head_output(8400, 80, seed=10, mode="dense")])
    for kw in (dict(), dict(max_det=1024, max_nms=20000), dict(iou_threshold=0.05, max_det=1024)):
        want = onms.non_max_suppression(y.numpy(), **kw)
        _assert_same(_gpu_nms(y, gpu, **kw), want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_vs_oracle(gpu, dtype):
    y = torch.stack([synth.synth_head_output(8400, 80, seed=4, mode="typical"),
                     synth.synth_head_output(8400, 80, seed=5, mode="dense")]).to(dtype)
    want = onms.non_max_suppression(y.float().numpy(), half=dtype)
    _assert_same(_gpu_nms(y, gpu), want)


def test_dropin_non_max_suppression(gpu):
    from utils.util import non_max_suppression
    g = load_golden("nms_forward_n640.npz")
    y = torch.from_numpy(load_golden(golden_name("n", 640, 1))["y"]).to(gpu)
    out = non_max_suppression(y)
    assert isinstance(out, list) and len(out) == 1 and out[0].device == y.device
    _assert_same([out[0].cpu().numpy()], _unpack(g["counts"], g["dets"]))


@pytest.mark.parametrize("iou", [-0.1, -0.0, -1e-30])
def test_negative_iou_threshold_vs_oracle(gpu, iou):
    """with iou_threshold < 0 a disjoint pair (IoU 0 > thr) suppresses too, across
    classes, so the same-class shortcut must not apply (torchvision's greedy contract)."""
    y = cases.negative_iou()
    want = onms.non_max_suppression(y, 0.001, iou, 300, 30000)
    _assert_same(_gpu_nms(torch.from_numpy(y), gpu, iou_threshold=iou), want)


@pytest.mark.parametrize("scores", ["spread", "tied", "spread_then_tied"])
def test_few_kept_long_continuation_vs_oracle(gpu, scores):
    """Boxes of each class piled on one spot: an image keeps about one box per class of 67 k
    candidates, so NMS runs later batches until max_nms candidates are processed (the C5
    pattern). 'spread': scores over many bins (the fast path's compact list); 'tied': one score
    for every pair (a single bin past 4096 keys: the radix-select path and its list).

    'spread_then_tied': a fast later batch followed by the switch to the radix path. Of 8400
    pairs per image 1500 have scores spread over 101 bins (at most 32 per bin) and 6900 share one
    score: a first batch of about 970 keys, one fast later batch of the about 530 spread keys
    left, then the tied bin (past 4096 keys) in two radix batches. Anchors 7, 107, .., 1007 are
    small boxes apart from the pile and from each other, so tied entries are kept (in tie order)
    and both the later batches' results and the max_nms cut inside the tied bin show in the
    output: the oracle keeps [96, 96], [40, 40] and [59, 62] rows per image for the three
    settings, of which 74 / 78, 18 / 22 and 37 / 44 carry the tied score."""
    y, kws = cases.few_kept(scores)
    for kw in kws:
        want = onms.non_max_suppression(y, 0.001, 0.65, kw.get("max_det", 300), kw.get("max_nms", 30000))
        _assert_same(_gpu_nms(torch.from_numpy(y), gpu, **kw), want)


# ---------------------------------------------------------------- the case list (tests/_nms_cases.py)
POISON = 0xA5
MARGIN = 256    # bytes of poison either side of the workspace view (keeps its 256-byte alignment)


class _Buffers:
    """dets, counts and a workspace of exactly nms_workspace_bytes as views into larger poisoned
    buffers; check() asserts that every byte outside the three views still holds the poison."""

    def __init__(self, dev, B, nc, A, max_det, ws_buf=None):
        from yolo_hip.engine import nms_workspace_bytes
        self.need = nms_workspace_bytes(B, nc, A)
        self.dets_buf = torch.full(((B + 2) * max_det * 6 * 4,), POISON, dtype=torch.uint8, device=dev)
        self.counts_buf = torch.full(((B + 2) * 4,), POISON, dtype=torch.uint8, device=dev)
        self.ws_buf = ws_buf if ws_buf is not None else torch.empty(self.need + 2 * MARGIN, dtype=torch.uint8, device=dev)
        assert self.ws_buf.numel() >= self.need + 2 * MARGIN
        self.ws_buf[:MARGIN] = POISON
        self.ws_buf[MARGIN + self.need:] = POISON
        self.dets = self.dets_buf.view(torch.float32).view(B + 2, max_det, 6)[1:B + 1]
        self.counts = self.counts_buf.view(torch.int32)[1:B + 1]
        self.ws = self.ws_buf[MARGIN:MARGIN + self.need]
        self.rows = max_det * 6 * 4

    def check(self, what):
        for name, outside in (("dets", (self.dets_buf[:self.rows], self.dets_buf[-self.rows:])),
                              ("counts", (self.counts_buf[:4], self.counts_buf[-4:])),
                              ("workspace", (self.ws_buf[:MARGIN], self.ws_buf[MARGIN + self.need:]))):
            for side, t in zip(("before", "after"), outside):
                assert bool((t == POISON).all()), f"{what}: bytes {side} the {name} view were written"


def _need(name):
    from yolo_hip.engine import nms_workspace_bytes
    B, no, A = cases.case(name)[0].shape
    return nms_workspace_bytes(B, no - 4, A)


def _buffers(name, dev, ws_buf=None):
    """ws_buf: the buffer to carve the case's workspace (and its margins) from, else a fresh one"""
    y, kw, _ = cases.case(name)
    B, no, A = y.shape
    return _Buffers(dev, B, no - 4, A, kw.get("max_det", 300), None if ws_buf is None else ws_buf[:_need(name) + 2 * MARGIN])


def _run_case(name, bufs, what=""):
    """the case through engine.nms(out=, workspace=) inside poisoned buffers -> kept rows per image"""
    from yolo_hip.engine import nms
    dev = bufs.ws.device
    dets, counts = nms(cases.tensor(name).to(dev), out=(bufs.dets, bufs.counts), workspace=bufs.ws, **cases.case(name)[1])
    assert dets.data_ptr() == bufs.dets.data_ptr() and counts.data_ptr() == bufs.counts.data_ptr()
    c = counts.cpu().tolist()
    d = dets.cpu().numpy()
    bufs.check(f"{name} {what}")
    return [d[i, :k] for i, k in enumerate(c)]


@pytest.mark.parametrize("name", cases.ALL)
def test_case_in_poisoned_buffers_on_a_stale_workspace(gpu, name):
    """Every case, bit-exact against the oracle, three times in one exactly-sized workspace: filled
    with ones, filled with zeros, and as the largest case of the list (overflow at the first
    selection, three radix batches; one image, so it fits) left it. nms_zero clears only the counts,
    the histograms and the gather counter; everything else must be written before it is read."""
    want = cases.want(name)
    bufs = _buffers(name, gpu)
    bufs.ws.fill_(0xFF)
    cases.assert_same(_run_case(name, bufs, "after ones"), want, f"{name} after ones:")
    bufs.ws.zero_()
    cases.assert_same(_run_case(name, bufs, "after zeros"), want, f"{name} after zeros:")
    big = _buffers(cases.LARGEST, gpu, bufs.ws_buf)   # same start; its far margin falls inside bufs.ws
    cases.assert_same(_run_case(cases.LARGEST, big), cases.want(cases.LARGEST), "the largest case:")
    cases.assert_same(_run_case(name, bufs, "after the largest case"), want, f"{name} after the largest case:")


def test_sequence_of_shapes_through_one_workspace(gpu):
    """One workspace sized for the largest shape, cases of different (B, nc, A) back to back in it,
    large to small and back, nothing cleared in between: what a rebuilt pipeline's result ring does."""
    order = ["ragged_130", "radix_first", "bin4097_md1024", "A1001_nc13", "bin65_md300", "A5_nc1", "bin1_md300",
             "A7_nc11", "bin1217_bf16", "few_kept_spread_then_tied", "conf_zero", "radix_after_fast", "ragged_130_bf16"]
    ws_buf = torch.empty(max(_need(n) for n in order) + 2 * MARGIN, dtype=torch.uint8, device=gpu)
    for step, name in enumerate(order):
        got = _run_case(name, _buffers(name, gpu, ws_buf), f"step {step}")
        cases.assert_same(got, cases.want(name), f"step {step} {name}:")


def test_rejects_strided_or_small_buffers(gpu):
    """engine.nms refuses, before any launch, a counts or workspace that yh_nms would write as dense memory
    although it is not, and a workspace below nms_workspace_bytes."""
    from yolo_hip.engine import nms, nms_workspace_bytes
    y = cases.tensor("A7_nc11").to(gpu)
    B, no, A = y.shape
    need = nms_workspace_bytes(B, no - 4, A)
    dets = torch.full((B, 300, 6), -7.0, device=gpu)
    counts = torch.full((2 * B,), -7, dtype=torch.int32, device=gpu)
    ws = torch.full((2 * need,), POISON, dtype=torch.uint8, device=gpu)
    bad = [dict(out=(dets, counts[::2]), workspace=ws[:need]),
           dict(out=(dets, counts[:B]), workspace=ws[::2]),
           dict(out=(dets, counts[:B]), workspace=ws[:need - 1]),
           dict(out=(dets.transpose(0, 1).contiguous().transpose(0, 1), counts[:B]), workspace=ws[:need])]
    for kw in bad:
        with pytest.raises(ValueError):
            nms(y, **kw)
    torch.cuda.synchronize()
    assert bool((dets == -7.0).all()) and bool((counts == -7).all()) and bool((ws == POISON).all())
    got_d, got_c = nms(y, out=(dets, counts[:B]), workspace=ws[:need])
    got = [got_d[i, :k].cpu().numpy() for i, k in enumerate(got_c.cpu().tolist())]
    cases.assert_same(got, cases.want("A7_nc11"))
    assert bool((ws[need:] == POISON).all()) and bool((counts[B:] == -7).all())
