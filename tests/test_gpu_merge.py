"""yh_merge (csrc/merge.hip) on the device against yh_merge_host and the numpy restatement: the same
bytes on the whole case list of tests/_merge_cases.py, the candidate cap and the NaN-poisoned
padding rows included. Marked gpu.
"""
import numpy as np
import pytest
import torch

import _merge_cases as mc
from yolo_hip.detect import merge

pytestmark = pytest.mark.gpu

_KEYS = ("dets", "counts", "tile_xf", "tile_offsets", "image_wh")


def _run(c, dev, out=None):
    t = [c[k].to(dev) for k in _KEYS]
    N = c["image_wh"].shape[0]
    if out is None:
        out = (torch.full((N, c["max_out"], 6), -7.0, device=dev), torch.full((N,), -7, dtype=torch.int32, device=dev))
    got = merge(*t, c["max_tiles"], iou=c["iou"], max_out=c["max_out"], out=out)
    assert got[0] is out[0] and got[1] is out[1]
    return out


def test_device_equals_host_on_every_case(gpu):
    """One test over the whole list: all launches are queued before the first download."""
    got = {name: _run(mc.case(name), gpu) for name in mc.ALL}
    torch.cuda.synchronize()
    for name in mc.ALL:
        c = mc.case(name)
        host = merge(*[c[k] for k in _KEYS], c["max_tiles"], iou=c["iou"], max_out=c["max_out"], threads=1)
        out, cnt = got[name][0].cpu().numpy(), got[name][1].cpu().numpy()
        assert np.isfinite(out).all(), name
        assert np.array_equal(cnt, host[1].numpy()), f"{name}: counts {cnt.tolist()} vs {host[1].tolist()}"
        assert out.tobytes() == host[0].numpy().tobytes(), name
        assert np.array_equal(out, c["want"][0]) and np.array_equal(cnt, c["want"][1]), name


def test_side_stream_and_fresh_buffers(gpu):
    c = mc.case("mixed")
    s = torch.cuda.Stream(device=gpu)
    t = [c[k].to(gpu) for k in _KEYS]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out, cnt = merge(*t, c["max_tiles"], iou=c["iou"], max_out=c["max_out"])
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), c["want"][0]) and np.array_equal(cnt.cpu().numpy(), c["want"][1])


def test_bad_arguments_raise_on_the_device_path(gpu):
    c = mc.case("chain")
    t = [c[k].to(gpu) for k in _KEYS]
    with pytest.raises(RuntimeError, match="YH_MERGE_MAX_CAND"):
        merge(*t, mc.CAP)
    with pytest.raises(RuntimeError, match="max_tiles"):
        merge(*t, 0)
    with pytest.raises(ValueError, match="expected cuda"):
        merge(t[0], c["counts"], *t[2:], 2)
