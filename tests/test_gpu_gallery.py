"""The identity search on the device (csrc/gallery.hip) against its host twins on the case list of
tests/_gallery_cases.py: the same bytes for scores, index, rows_out, gallery, labels, size and
next_label, outputs inside poisoned buffers whose margins stay untouched. Marked gpu.

The host twins themselves are pinned to the numpy restatement by tests/test_gallery_host.py.
"""
import numpy as np
import pytest
import torch

import _gallery_cases as gc
import yolo_hip

pytestmark = pytest.mark.gpu


def check_search(case, gpu, chunks=gc.CHUNKS):
    want = gc.run_search(case, threads=4)
    for chunk_rows in chunks:
        got = gc.run_search(case, gpu, chunk_rows)
        assert np.array_equal(got[0], want[0]), ("scores", chunk_rows)
        assert np.array_equal(got[1], want[1]), ("index", chunk_rows)
    return want


@pytest.mark.parametrize("dim,nq,n,k", gc.SEARCH_CASES)
def test_search_device_equals_host(gpu, dim, nq, n, k):
    check_search(gc.search_case(dim, nq, n, k), gpu)


@pytest.mark.parametrize("k", [1, 5, 32])
def test_ties_and_galleries_in_score_order(gpu, k):
    """Ties at the k-th place; a gallery where every row enters the running k best, and one where
    none does after the first k."""
    check_search(gc.tie_case(k), gpu)
    for descending in (False, True):
        _, index = check_search(gc.ordered_case(descending, k), gpu)
        assert (index[:, 0] == (0 if descending else 199)).all()


def test_clamped_counts_and_sizes_and_no_labels(gpu):
    case = dict(gc.search_case(64, 65, 65, 5), labels=None)
    case["gallery"][:3] = -128
    case["q"][1] = -128
    for size, count in ((-4, None), (1000, 1000), (64, -1), (None, 64), (65, None)):
        check_search(dict(case, size=size, count=count), gpu)


@pytest.mark.parametrize("dim,nq,n,k,chunk_rows", [
    (1280, 130, 4092, 8, 0),       # capacity 4099: more chunks than XCDs, three query tiles
    (64, 70, 2500, 5, 1024),       # eight waves per workgroup, a partial last chunk
    (2048, 65, 300, 32, 0),        # the longest rows with the longest lists: one wave per workgroup
    (128, 600, 700, 3, 192),       # ten query tiles
])
def test_search_at_the_shapes_the_launch_turns_on(gpu, dim, nq, n, k, chunk_rows):
    case = gc.search_case(dim, nq, n, k)
    assert len(case["gallery"]) == n + 7
    check_search(case, gpu, (chunk_rows,))


@pytest.mark.parametrize("args", gc.ENROL_CASES)
def test_enrol_device_equals_host(gpu, args):
    case = gc.enrol_case(*args)
    gc.same_enrol(gc.run_enrol(case, gpu), gc.run_enrol(case), args)


def test_a_gallery_moved_to_the_cpu_continues_with_the_same_bytes(gpu):
    rng = np.random.default_rng(21)
    batches = [torch.from_numpy(rng.integers(-128, 128, (40, 128), dtype=np.int8)) for _ in range(4)]
    host, dev = yolo_hip.Gallery(130, 128), yolo_hip.Gallery(130, 128, gpu)
    for step, b in enumerate(batches):
        if step == 2:
            assert dev.to("cpu").device.type == "cpu"
        take = torch.from_numpy((rng.integers(0, 2, 40)).astype(np.int32))
        res = []
        for gal in (host, dev):
            x = b.to(gal.device)
            found = gal.search(x, k=4)
            rows = gal.enrol(x, take=take.to(gal.device))
            gal.remove(3 * step)
            res.append([t.cpu() for t in found] + [rows.cpu()])
        for a, w in zip(*res):
            assert torch.equal(a, w), step
    for name in ("data", "labels", "size", "next_label"):
        assert torch.equal(getattr(dev, name).cpu(), getattr(host, name)), name
    assert host.size.item() > 60


def test_identify_gives_one_label_per_person_across_cameras(gpu):
    dev = gc.identify_scenario(gpu)
    host = gc.identify_scenario("cpu")
    for name in ("data", "labels", "size", "next_label"):
        assert torch.equal(getattr(dev, name).cpu(), getattr(host, name)), name


def test_classifier_embeddings_feed_identify_on_the_device(gpu):
    """crop_rois -> Classifier.predict(embed=True) -> Gallery.identify(embed, count=crops.total),
    nothing read back in between: rows beyond the total come back unknown and are not enrolled."""
    import _cls_cases as cc
    import _track_cases as tc
    from yolo_hip import preprocess as pre, synth
    from yolo_hip.classify import Classifier

    def frame(seed):
        x = synth.synth_scenes(1, 240, 320, seed=seed)[0]
        return (x.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous()   # BGR HWC

    cls = Classifier(cc.make_model("n", 10), gpu, torch.bfloat16, max_batch=16)
    gal = yolo_hip.Gallery(32, 1280, gpu)
    rows = [[tc.box(60, 80, 50, 90, 0.9), tc.box(200, 120, 60, 100, 0.8)], [tc.box(100, 100, 70, 70, 0.7)]]
    dets, counts = tc.pack(rows, 4)
    crops = pre.crop_rois([frame(71), frame(72)], dets.to(gpu), counts.to(gpu), (64, 32))
    got = cls.predict(crops, embed=True)
    labels, scores = gal.identify(got.embed, cos_min=2.0, count=crops.total)     # nothing is known at cosine 2
    assert got.embed.shape == (8, 1280) and int(crops.total[0]) == 3
    assert labels[3:].tolist() == [-1] * 5 and (scores[3:] == gc.INT32_MIN).all()
    assert gal.size.item() == 3 - int((labels[:3] < 0).sum()) and gal.next_label.item() == gal.size.item()
    again, _ = gal.identify(got.embed, count=crops.total, enrol=False)
    assert again[3:].tolist() == [-1] * 5 and gal.next_label.item() == gal.size.item() <= 3
