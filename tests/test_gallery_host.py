"""The host twins of the identity search (yh_gallery_search_host, yh_gallery_enrol_host) against the
numpy restatement of include/yolo_hip.h in tests/_gallery_cases.py: the same integers, whatever the
chunking; the argument errors; and the behaviour the tracker's per-stream ids lack - one label for
one person across cameras. CPU only.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _gallery_cases as gc
import yolo_hip
from yolo_hip import _lib
from yolo_hip import gallery as yg

NEW_SYMBOLS = ("yh_gallery_workspace_bytes", "yh_gallery_search", "yh_gallery_search_host", "yh_gallery_enrol",
               "yh_gallery_enrol_host")


def check_search(case, want=None):
    """The three chunkings and two thread counts give the restatement's integers. The host twin is one
    loop over the rows: of chunk_rows it sees the argument check and the workspace that the chunking
    asks for, so here the chunk loop pins that every chunking is accepted with its own workspace size
    and changes nothing. The chunks' lists and their merge exist on the device only and are tested
    there (tests/test_gpu_gallery.py). One thread count is enough for the chunkings other than 0."""
    want = gc.search(case["gallery"], case["labels"], case["size"], case["q"], case["count"], case["k"]) \
        if want is None else want
    for chunk_rows in gc.CHUNKS:
        for threads in (1, 3) if chunk_rows == 0 else (3,):
            got = gc.run_search(case, chunk_rows=chunk_rows, threads=threads)
            assert np.array_equal(got[0], want[0]), ("scores", chunk_rows, threads)
            assert np.array_equal(got[1], want[1]), ("index", chunk_rows, threads)
    return want


def test_the_case_list_covers_the_sizes_the_paths_turn_on():
    dims, nqs, ns, ks = (set(c[i] for c in gc.SEARCH_CASES) for i in range(4))
    assert dims == {64, 128, 1280} and nqs == {0, 1, 63, 64, 65, 130} and ks == {1, 5, 32}
    assert {0, 1, 63, 64, 65, 200, 127, 128, 129} <= ns
    for k in ks:
        assert any(c[3] == k and c[2] == k - 1 for c in gc.SEARCH_CASES), k
        assert any(c[3] == k and c[2] == k for c in gc.SEARCH_CASES), k


@pytest.mark.parametrize("dim,nq,n,k", gc.SEARCH_CASES)
def test_search_host_equals_the_restatement(dim, nq, n, k):
    case = gc.search_case(dim, nq, n, k)
    scores, index = check_search(case)
    m = gc.clamp(case["count"], nq)
    assert (index[m:] == -1).all() and (scores[m:] == gc.INT32_MIN).all()
    if nq > 2:
        assert (index[2] == -1).all()                                  # the zero query
    if nq and n:
        # the data has teeth: the rows beyond size would win query 0, and so would the hidden labels
        full = gc.search(case["gallery"], case["labels"], None, case["q"], case["count"], k)
        assert full[1][0, 0] == n and index[0, 0] != n
        if n > 2:
            bare = gc.search(case["gallery"], None, n, case["q"], case["count"], k)
            assert not np.array_equal(bare[1], index)
            assert (case["labels"][index[index >= 0]] >= 0).all()
    cand = int((case["labels"][:n] >= 0).sum())
    if nq and m:
        assert (index[0] >= 0).sum() == min(k, cand)                   # INT32_MIN / -1 beyond the candidates


@pytest.mark.parametrize("k", [1, 5, 32])
def test_ties_fall_to_the_lower_row(k):
    case = gc.tie_case(k)
    s = case["q"].astype(np.int32) @ case["gallery"].astype(np.int32).T
    ranked = -np.sort(-s, axis=1)
    assert (ranked[:, k - 1] == ranked[:, k]).all(), "the case lost its ties at the k-th place"
    scores, index = check_search(case)
    assert (np.diff(scores, axis=1) <= 0).all()
    tied = np.diff(scores, axis=1) == 0
    assert (np.diff(index, axis=1)[tied] > 0).all() and tied.any() or k == 1


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("descending", [False, True])
def test_galleries_in_score_order(descending, k):
    """Ascending: every row enters the running k best. Descending: none after the first k."""
    case = gc.ordered_case(descending, k)
    scores, index = check_search(case)
    want = np.arange(k) if descending else 199 - np.arange(k)
    assert (index == want[None, :]).all()


def test_counts_and_sizes_are_clamped_and_minus_128_is_legal():
    case = dict(gc.search_case(64, 65, 65, 5), labels=None)
    case["gallery"][:3] = -128
    case["q"][1] = -128
    for size, count in ((-4, None), (1000, 1000), (64, -1), (None, 64)):
        c = dict(case, size=size, count=count)
        scores, index = check_search(c)
    assert check_search(dict(case, count=None))[0][1, 0] == 128 * 128 * 64


@pytest.mark.parametrize("args", gc.ENROL_CASES)
def test_enrol_host_equals_the_restatement(args):
    case = gc.enrol_case(*args)
    got, want = gc.run_enrol(case), gc.want_enrol(case)
    gc.same_enrol(got, want, args)
    rows = want[4]
    assert (rows[1::7] == -1).all()                                    # the zero rows
    if case["take"] is not None:
        assert (rows[case["take"] == 0] == -1).all() and (rows[case["take"] == -5] >= 0).any()


def test_enrol_cases_have_teeth():
    fills = gc.want_enrol(gc.enrol_case(*gc.ENROL_CASES[1]))
    assert fills[2] == 40 and (fills[4][:10] >= 0).any() and (fills[4][-40:] == -1).all()   # full in the middle
    given = gc.enrol_case(*gc.ENROL_CASES[2])
    res = gc.want_enrol(given)
    on = res[4] >= 0
    assert np.array_equal(res[1][res[4][on]], given["labels_in"][on]) and res[3] == 4242    # next_label untouched
    own = gc.want_enrol(gc.enrol_case(*gc.ENROL_CASES[0]))
    assert own[3] == 4242 + (own[4] >= 0).sum() > 4242
    assert gc.want_enrol(gc.enrol_case(*gc.ENROL_CASES[6]))[2] == 8                         # a size beyond capacity


def test_two_calls_in_a_row_and_a_search_of_what_they_enrolled():
    rng = np.random.default_rng(9)
    gal = yolo_hip.Gallery(100, 64)
    a = torch.from_numpy(rng.integers(-128, 128, (70, 64), dtype=np.int8))
    b = torch.from_numpy(rng.integers(-128, 128, (70, 64), dtype=np.int8))
    a[4] = 0
    ra = gal.enrol(a)
    assert gal.size.item() == 69 and gal.next_label.item() == 69 and ra[4].item() == -1 and ra[69].item() == 68
    rb = gal.enrol(b, labels=torch.arange(500, 570, dtype=torch.int32))
    assert gal.size.item() == 100 and gal.next_label.item() == 69
    assert rb[:31].tolist() == list(range(69, 100)) and (rb[31:] == -1).all()
    assert gal.labels[:69].tolist() == list(range(69)) and gal.labels[69:].tolist() == list(range(500, 531))
    assert torch.equal(gal.data[69:], b[:31]) and torch.equal(gal.data[:4], a[:4]) and torch.equal(gal.data[4:69], a[5:])
    scores, index, labels = gal.search(b[:40], k=3)
    assert index[:31, 0].tolist() == list(range(69, 100)) and labels[:31, 0].tolist() == list(range(500, 531))
    want = gc.search(gal.data.numpy(), gal.labels.numpy(), 100, b[:40].numpy(), None, 3)
    assert np.array_equal(scores.numpy(), want[0]) and np.array_equal(index.numpy(), want[1])
    assert np.array_equal(labels.numpy(), gal.labels.numpy()[want[1]])


def test_identify_gives_one_label_per_person_across_cameras():
    gc.identify_scenario("cpu")


def test_workspace_is_per_chunk_and_query_never_per_row_and_query():
    lib = _lib.lib()
    al = lambda v: (v + 255) // 256 * 256
    assert lib.yh_gallery_workspace_bytes(200, 65, 5, 64) == al(4 * 65 * 5 * 8)
    assert lib.yh_gallery_workspace_bytes(200, 65, 5, 128) == al(2 * 65 * 5 * 8)
    assert yg.gallery_workspace(200, 65, 5, 128).numel() == al(2 * 65 * 5 * 8)
    assert lib.yh_gallery_workspace_bytes(0, 65, 5, 0) == 0 and lib.yh_gallery_workspace_bytes(200, 0, 5, 0) == 0
    for nq, k in ((64, 1), (512, 8), (512, 32)):
        small, big = (lib.yh_gallery_workspace_bytes(c, nq, k, 0) for c in (1 << 16, 1 << 20))
        assert 0 < small <= big <= 1024 * nq * k * 8, (nq, k)             # the chunk count is bounded
        assert big < (1 << 20) * nq                                    # far below a byte per (row, query)
    for bad in ((-1, 4, 1, 0), (4, -1, 1, 0), (4, 4, 0, 0), (4, 4, 33, 0), (4, 4, 1, 32), (4, 4, 1, -64)):
        assert lib.yh_gallery_workspace_bytes(*bad) == 0, bad


def test_bad_arguments_are_einval():
    lib = _lib.lib()
    t = torch.zeros((1 << 16,))
    b = ctypes.c_void_p(t.data_ptr())

    def search(gallery=b, capacity=8, dim=64, q=b, nq=4, k=2, chunk=0, scores=b, index=b, ws=b, ws_bytes=1 << 18):
        return lib.yh_gallery_search_host(gallery, None, None, capacity, dim, q, nq, None, k, chunk, scores, index, ws,
                                          ws_bytes, 1)

    assert search() == 0 and search(gallery=None, capacity=0, ws=None, ws_bytes=0) == 0
    assert search(q=None, nq=0, scores=None, index=None, ws=None, ws_bytes=0) == 0
    for kw, word in ((dict(dim=0), b"dim"), (dict(dim=96), b"dim"), (dict(dim=4096), b"dim"), (dict(k=0), b"k must"),
                     (dict(k=33), b"k must"), (dict(capacity=-1), b">= 0"), (dict(nq=-1), b">= 0"),
                     (dict(capacity=(1 << 31) - 1), b"capacity exceeds"),
                     (dict(chunk=32), b"chunk_rows"), (dict(chunk=-64), b"chunk_rows"), (dict(chunk=100), b"chunk_rows"),
                     (dict(ws_bytes=8), b"workspace too small"), (dict(ws=None), b"null workspace"),
                     (dict(gallery=None), b"null gallery"), (dict(q=None), b"null q"), (dict(scores=None), b"null scores"),
                     (dict(index=None), b"null scores")):
        assert search(**kw) == -1, kw
        assert word in lib.yh_last_error(), (kw, lib.yh_last_error())

    p = [ctypes.c_void_p(t.data_ptr() + 16384 * i) for i in range(6)]   # operands that do not overlap

    def enrol(gallery=p[0], labels=p[1], size=p[2], capacity=8, dim=64, q=p[3], nq=4, labels_in=None, nxt=p[4], rows=p[5]):
        return lib.yh_gallery_enrol_host(gallery, labels, size, capacity, dim, q, nq, None, None, labels_in, nxt, rows, 1)

    assert enrol() == 0 and enrol(labels_in=p[4], nxt=None) == 0 and enrol(q=None, nq=0, rows=None) == 0
    for kw, word in ((dict(dim=32), b"dim"), (dict(capacity=-1), b">= 0"), (dict(nq=-2), b">= 0"), (dict(size=None), b"null size"),
                     (dict(gallery=None), b"null gallery"), (dict(labels=None), b"null gallery"), (dict(q=None), b"null q"),
                     (dict(rows=None), b"null q"), (dict(nxt=None), b"null next_label")):
        assert enrol(**kw) == -1, kw
        assert word in lib.yh_last_error(), (kw, lib.yh_last_error())


def test_device_entry_points_reject_before_any_launch():
    """yh_gallery_search and yh_gallery_enrol check their arguments, the 16-byte alignment of the device
    operands included, before the first HIP call: every call here fails, so nothing reaches a device
    and the test needs none. (A call that passed the checks would launch.)"""
    lib = _lib.lib()
    t = torch.zeros((1 << 16,))
    base = t.data_ptr()
    assert base % 16 == 0
    p = [base + 32768 * i for i in range(6)]
    vp = ctypes.c_void_p

    def search(gallery=p[0], q=p[1], ws=p[2], dim=64, k=2, chunk=0, ws_bytes=1 << 15, scores=p[3]):
        return lib.yh_gallery_search(vp(gallery), None, None, 8, dim, vp(q), 4, None, k, chunk, vp(scores), vp(p[4]),
                                     vp(ws), ws_bytes, None)

    def enrol(gallery=p[0], q=p[1], dim=64, size=p[3], nxt=p[5]):
        return lib.yh_gallery_enrol(vp(gallery), vp(p[2]), vp(size) if size else None, 8, dim, vp(q), 4, None, None, None,
                                    vp(nxt) if nxt else None, vp(p[4]), None)

    for off in range(1, 16):
        for kw in (dict(gallery=p[0] + off), dict(q=p[1] + off), dict(ws=p[2] + off)):
            assert search(**kw) == -1, (off, kw)
            assert b"16-byte aligned" in lib.yh_last_error(), (off, kw)
        for kw in (dict(gallery=p[0] + off), dict(q=p[1] + off)):
            assert enrol(**kw) == -1, (off, kw)
            assert b"16-byte aligned" in lib.yh_last_error(), (off, kw)
    # the checks the device symbols share with the twins come first
    for kw, word in ((dict(dim=96), b"dim"), (dict(k=0), b"k must"), (dict(k=33), b"k must"), (dict(chunk=100), b"chunk_rows"),
                     (dict(ws_bytes=8), b"workspace too small"), (dict(ws=0), b"null workspace"),
                     (dict(scores=0), b"null scores"), (dict(dim=96, q=p[1] + 1), b"dim")):
        assert search(**kw) == -1, kw
        assert word in lib.yh_last_error(), (kw, lib.yh_last_error())
    for kw, word in ((dict(dim=32), b"dim"), (dict(size=0), b"null size"), (dict(nxt=0), b"null next_label"),
                     (dict(dim=32, gallery=p[0] + 4), b"dim")):
        assert enrol(**kw) == -1, kw
        assert word in lib.yh_last_error(), (kw, lib.yh_last_error())
    assert not t.any()                                                 # nothing was written


def test_the_python_layer_checks_its_arguments():
    g, q = torch.zeros((8, 64), dtype=torch.int8), torch.zeros((4, 64), dtype=torch.int8)
    with pytest.raises(ValueError, match="k must be"):
        yolo_hip.gallery_search(g, q, 0)
    with pytest.raises(ValueError, match="chunk_rows"):
        yolo_hip.gallery_search(g, q, 1, chunk_rows=96)
    with pytest.raises(ValueError, match="multiple of 64"):
        yolo_hip.gallery_search(g[:, :32].contiguous(), q[:, :32].contiguous())
    with pytest.raises(TypeError, match="yolo_hip.gallery: q must be torch.int8"):
        yolo_hip.gallery_search(g, q.float())
    with pytest.raises(ValueError, match="yolo_hip.gallery: the feature length"):
        yolo_hip.Gallery(10, 100)
    with pytest.raises(ValueError, match="shape"):
        yolo_hip.gallery_search(g, torch.zeros((4, 128), dtype=torch.int8))
    with pytest.raises(ValueError, match="contiguous"):
        yolo_hip.gallery_search(g, torch.zeros((4, 128), dtype=torch.int8)[:, ::2])
    with pytest.raises(ValueError, match="shape"):
        yolo_hip.gallery_search(g, q, 2, out=(torch.zeros((4, 1), dtype=torch.int32),) * 2)
    with pytest.raises(ValueError, match="next_label"):
        yolo_hip.gallery_enrol(g, torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), q)
    with pytest.raises(ValueError, match="multiple of 64"):
        yolo_hip.Gallery(10, 100)
    with pytest.raises(ValueError, match=">= 0"):
        yolo_hip.Gallery(10, 64).remove(-1)


def test_the_new_symbols_are_in_the_header_the_protos_and_the_library():
    lib = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "yolo_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib._PROTOS, name
        assert hasattr(lib, name), name
    assert "YH_GALLERY_MAX_K 32" in header and yg.MAX_K == 32
    assert lib.yh_abi_version() == 7
    for name in ("Gallery", "gallery_search", "gallery_enrol", "gallery_workspace"):
        assert callable(getattr(yolo_hip, name))
