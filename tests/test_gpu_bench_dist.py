"""bench.py under torch.distributed.run at world size 1: the data-parallel path
(process group on backend "nccl" = RCCL, the gather of the packed detections to
rank 0 on device tensors) runs on the GPU, and rank 0's gathered rows equal its
own NMS results (bench.py records the check). The run is a plain one (no --full)
with --dump-outputs, so the result line's fields and the dumped detections of the
last timed step are checked too. Marked gpu.

The N > 1 gather logic itself is covered on CPU by tests/test_dist_gloo.py.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("extra", [[], ["--serial"]])
def test_bench_under_torchrun_world1_gathers_over_rccl(gpu, extra, tmp_path):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--no-cpu-baseline", "--no-roofline", "--dump-outputs", str(tmp_path / "dump"), *extra]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])
    assert rec["n_gpus"] == 1 and rec["value"] > 0
    assert rec["gather"] is not None and "1 rank(s)" in rec["gather"], rec["gather"]
    assert rec["gather"].endswith("match: True"), rec["gather"]
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert rec["roofline"] is None and rec["cpu_baseline"] is None   # a plain run: neither without --full
    # --dump-outputs: the gathered detections of the last timed step, float32, nothing past the counts
    dets, counts = np.load(tmp_path / "dump" / "dets.npy"), np.load(tmp_path / "dump" / "counts.npy")
    assert dets.dtype == np.float32 and counts.dtype == np.float32
    assert dets.shape == (32, 300, 6) and counts.shape == (32,)
    assert counts[:4].tolist() == rec["kept_last_step"]
    assert np.isfinite(dets).all() and ((counts >= 0) & (counts <= 300)).all() and counts.sum() > 0
    for d, c in zip(dets, counts.astype(int)):
        assert (d[:c, 4] > 0.001).all() and (np.diff(d[:c, 4]) <= 0).all()   # kept rows: score-descending
        assert not d[c:].any()
