"""compute_ap(plot=True) (reference utils/util.py:180-222, 286-292): the same six values
as plot=False, and the four curve images at 9 x 6 in, 250 dpi, in a save_dir it creates.
"""
import numpy as np
import pytest
import torch
from PIL import Image

from conftest import load_golden
from yolo_hip.metrics import compute_ap

FILES = ("PR_curve.png", "F1_curve.png", "P_curve.png", "R_curve.png")


@pytest.fixture(scope="module")
def cat():
    g = load_golden("metrics_synth.npz")
    tp, conf, cls, tgt = [], [], [], []
    for i in range(int(g["n_img"])):
        out = g[f"out_{i}"]
        tp.append(g[f"correct_{i}"].reshape(out.shape[0], 10))
        conf.append(out[:, 4])
        cls.append(out[:, 5])
        tgt.append(g[f"tgt_{i}"].reshape(-1, 5)[:, 0])
    return [np.concatenate(x, 0) for x in (tp, conf, cls, tgt)]


@pytest.fixture(scope="module")
def plain(cat):
    return compute_ap(*cat, device="cpu")


@pytest.mark.parametrize("n_names", [6, 80])
def test_plot_returns_the_same_and_writes_four_pngs(cat, plain, n_names, tmp_path):
    save_dir = tmp_path / "does" / "not" / "exist"
    names = [f"class{i}" for i in range(n_names)]
    got = compute_ap(*cat, plot=True, names=names, device="cpu", save_dir=str(save_dir))
    assert len(got) == 6
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    assert tuple(got[2:]) == tuple(plain[2:])
    for f in FILES:
        with Image.open(save_dir / f) as im:
            assert im.format == "PNG" and im.size == (2250, 1500)
            assert len(im.convert("L").getcolors(1 << 16)) > 2          # something is drawn


def test_plot_with_tensors_names_dict_and_no_names(cat, plain, tmp_path):
    t = [torch.from_numpy(x) for x in cat]
    got = compute_ap(*t, plot=True, names={i: str(i) for i in range(6)}, save_dir=str(tmp_path / "a"))
    assert tuple(got[2:]) == tuple(plain[2:])
    compute_ap(*t, plot=True, save_dir=str(tmp_path / "b"))
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == sorted(FILES)
