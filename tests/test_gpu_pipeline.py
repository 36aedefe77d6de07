"""Two-stream DetectPipeline (forward k+1 beside NMS k), and with two forward lanes
(forwards of consecutive batches overlap on two engines), vs the sequential schedule,
at the bench's full size (v11_n, 640x640, batch 32, bf16). Marked gpu.

Bar: bit-identical detections and counts for every batch - the pipeline only
reorders independent work across streams. Plus the on-device NMS of a full
bench batch against the CPU oracle on the same head output (bit-exact).

The result ring (result_ring=True, the mode bench.py times) runs at a small shape
(batch 3, 96x160) with three lanes: every batch read inside its validity window,
for both NMS placements and both idle_skip settings, and submit(out=) into
caller-owned rows.
"""
import numpy as np
import pytest
import torch

from oracle import nms as onms
from yolo_hip import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(gpu):
    from nets import nn
    from yolo_hip.engine import Engine
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    eng = Engine(*model._yh_arch, gpu, torch.bfloat16)
    eng.load_module(model)
    return eng


def test_pipeline_equals_sequential(gpu, engine):
    from yolo_hip.engine import nms
    from yolo_hip.pipeline import DetectPipeline
    B, S = 32, 640
    xs = [synth.synth_scenes(B, S, S, seed=200 + i).to(gpu, torch.bfloat16) for i in range(3)]
    want = []
    for x in xs:
        y = engine.forward(x)
        d, c = nms(y)
        want.append((d.cpu(), c.cpu()))
    pipe = DetectPipeline(engine, B, S, S)
    got = [pipe.submit(x) for x in xs + xs[:1]]   # 4 batches: buffer reuse is exercised
    torch.cuda.synchronize()
    for i, (d, c, _, _) in enumerate(got):
        wd, wc = want[i % 3]
        assert torch.equal(c.cpu(), wc), f"batch {i}: counts differ"
        for j, k in enumerate(wc.tolist()):
            assert torch.equal(d[j, :k].cpu(), wd[j, :k]), f"batch {i} image {j}"


def test_two_lane_pipeline_equals_sequential(gpu, engine):
    from nets import nn
    from yolo_hip.engine import Engine, nms
    from yolo_hip.pipeline import DetectPipeline
    B, S = 32, 640
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    lane1 = Engine(*model._yh_arch, gpu, torch.bfloat16)
    lane1.load_module(model)
    xs = [synth.synth_scenes(B, S, S, seed=210 + i).to(gpu, torch.bfloat16) for i in range(3)]
    want = []
    for x in xs:
        d, c = nms(engine.forward(x))
        want.append((d.cpu(), c.cpu()))
    pipe = DetectPipeline([engine, lane1], B, S, S)
    got = [pipe.submit(x) for x in xs + xs]   # 6 batches over 2 lanes and 4 head buffers
    pipe.drain()
    torch.cuda.synchronize()
    for i, (d, c, _, _) in enumerate(got):
        wd, wc = want[i % 3]
        assert torch.equal(c.cpu(), wc), f"batch {i}: counts differ"
        for j, k in enumerate(wc.tolist()):
            assert torch.equal(d[j, :k].cpu(), wd[j, :k]), f"batch {i} image {j}"


def test_full_batch_nms_matches_oracle(gpu, engine):
    from yolo_hip.engine import nms
    x = synth.synth_scenes(32, 640, 640, seed=300).to(gpu, torch.bfloat16)
    y = engine.forward(x)
    d, c = nms(y)
    d, c = d.cpu().numpy(), c.cpu().tolist()
    want = onms.non_max_suppression(y.float().cpu().numpy(), half=torch.bfloat16)
    assert len(want) == 32
    for j, w in enumerate(want):
        assert c[j] == w.shape[0], f"image {j}: kept {c[j]} vs {w.shape[0]}"
        np.testing.assert_array_equal(d[j, :c[j]], w, err_msg=f"image {j}")


# ---------------------------------------------------------------- the result ring (the benchmark's mode)
RB, RH, RW = 3, 96, 160


@pytest.fixture(scope="module")
def lanes3(gpu, engine):
    """three engines with the same weights: the benchmark's three forward lanes"""
    from nets import nn
    from yolo_hip.engine import Engine
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    more = [Engine(*model._yh_arch, gpu, torch.bfloat16) for _ in range(2)]
    for e in more:
        e.load_module(model)
    return [engine] + more


@pytest.fixture(scope="module")
def ring_inputs(gpu, engine):
    """Distinct inputs, many detections (scenes, noise: 300 per image of 18 k - 34 k candidates)
    next to few (a dark scene, a flat image: some tens of a few hundred candidates), so that a ring
    slot's and the workspace's previous contents differ from what the next batch writes; with each
    the sequential schedule's (dets, counts)."""
    from yolo_hip.engine import nms
    g = torch.Generator().manual_seed(1)
    xs = [synth.synth_scenes(RB, RH, RW, seed=400), torch.full((RB, 3, RH, RW), 0.5),
          torch.rand(RB, 3, RH, RW, generator=g), synth.synth_scenes(RB, RH, RW, seed=401) * 0.05,
          synth.synth_scenes(RB, RH, RW, seed=402), torch.zeros(RB, 3, RH, RW),
          synth.synth_scenes(RB, RH, RW, seed=403) * 0.05]
    xs = [x.to(gpu, torch.bfloat16) for x in xs]
    want = []
    for x in xs:
        d, c = nms(engine.forward(x))
        want.append((d.cpu(), c.cpu()))
    kept = [int(c.sum()) for _, c in want]
    assert max(kept) >= 4 * max(min(kept), 1), f"the inputs should mix many and few detections: {kept}"
    return xs, want


def _same_batch(d, c, want, what):
    wd, wc = want
    c = c.cpu()
    assert torch.equal(c, wc), f"{what}: counts {c.tolist()} vs {wc.tolist()}"
    d = d.cpu()
    for j, k in enumerate(wc.tolist()):
        assert torch.equal(d[j, :k], wd[j, :k]), f"{what} image {j}"


@pytest.mark.parametrize("idle_skip", [True, False])
@pytest.mark.parametrize("nms_on_lane", [False, True])
def test_result_ring_equals_sequential(gpu, lanes3, ring_inputs, nms_on_lane, idle_skip):
    """Three lanes, result_ring=True: batch k lives in slot k % slots and is read after wait(done), at
    the last moment of its window - right before batch k + slots, which overwrites it, is submitted."""
    from yolo_hip.pipeline import DetectPipeline
    xs, want = ring_inputs
    pipe = DetectPipeline(lanes3, RB, RH, RW, nms_on_lane=nms_on_lane, result_ring=True, idle_skip=idle_skip)
    slots = len(pipe.dets)
    assert slots == 6
    n = 2 * slots + 1
    got = []

    def read(k):
        d, c, _, done = got[k]
        pipe.wait(done)
        _same_batch(d, c, want[k % len(xs)], f"batch {k}")

    for k in range(n):
        if k >= slots:
            read(k - slots)
        got.append(pipe.submit(xs[k % len(xs)]))
        assert got[k][0].data_ptr() == pipe.dets[k % slots].data_ptr()
    for k in range(n - slots, n):
        read(k)
    pipe.drain()
    torch.cuda.synchronize()


def test_result_ring_submit_into_caller_rows(gpu, lanes3, ring_inputs):
    """submit(x, out=(dets, counts)) into rows of one caller-owned tensor, the way Detector packs a
    call; the ring's workspace is still the one every batch's NMS reuses."""
    from yolo_hip.pipeline import DetectPipeline
    xs, want = ring_inputs
    pipe = DetectPipeline(lanes3, RB, RH, RW, result_ring=True)
    n = 2 * len(pipe.dets) + 1
    tdets = torch.full((n * RB, 300, 6), float("nan"), device=gpu)
    tcounts = torch.full((n * RB,), -1, dtype=torch.int32, device=gpu)
    done = [pipe.submit(xs[k % len(xs)], out=(tdets[k * RB:(k + 1) * RB], tcounts[k * RB:(k + 1) * RB]))[3]
            for k in range(n)]
    for e in done:
        pipe.wait(e)
    pipe.drain()
    torch.cuda.synchronize()
    for k in range(n):
        _same_batch(tdets[k * RB:(k + 1) * RB], tcounts[k * RB:(k + 1) * RB], want[k % len(xs)], f"batch {k}")
