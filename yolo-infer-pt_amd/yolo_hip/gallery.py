"""Identities across streams and time: a gallery of unit int8 features searched on the device.

`Tracker` gives ids that are local to one stream's track table. A `Gallery` is the global side: a
caller-owned database of `embed_quantize` rows with a label each, searched for the k best rows
per query in one pass over the gallery - the exact int32 products on the int8 MFMA, the running
k best of every query kept on chip, the (nq, n) score matrix never written - and appended to
without a read-back:

  gallery_search     yh_gallery_search / yh_gallery_search_host (functional)
  gallery_enrol      yh_gallery_enrol / yh_gallery_enrol_host
  gallery_workspace  the scratch buffer of a search
  Gallery            data, labels, size, next_label and a workspace; search, enrol, remove, identify

There is no counterpart in the reference; the semantics are those stated in include/yolo_hip.h,
pinned by the numpy restatement in tests/_gallery_cases.py. cuda tensors run the HIP kernels on
the current stream, CPU tensors the host twins: the same bytes.
"""
import ctypes
import math

import torch

from . import track as _track
from .track import _ptr, embed_quantize

MAX_K = 32   # YH_GALLERY_MAX_K
_WHO = "yolo_hip.gallery"


def _check(name, t, shape, dtype, device):
    _track._check(name, t, shape, dtype, device, who=_WHO)


def _check_dim(dim):
    return _track._check_dim(dim, who=_WHO)


def _check_k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"yolo_hip.gallery: k must be in [1, {MAX_K}], got {k}")
    return k


def _check_chunk(chunk_rows):
    chunk_rows = int(chunk_rows)
    if chunk_rows < 0 or chunk_rows % 64:
        raise ValueError(f"yolo_hip.gallery: chunk_rows must be 0 or a positive multiple of 64, got {chunk_rows}")
    return chunk_rows


def gallery_workspace(capacity, nq, k=1, chunk_rows=0, device="cpu"):
    """The scratch buffer of `gallery_search` for these sizes (uint8; k keys of 8 bytes per chunk and
    query; its contents mean nothing between calls)."""
    from ._lib import lib
    n = lib().yh_gallery_workspace_bytes(int(capacity), int(nq), _check_k(k), _check_chunk(chunk_rows))
    return torch.empty((n,), dtype=torch.uint8, device=device)


def _matrix(name, t, dtype=torch.int8):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"yolo_hip.gallery: {name} must be a (rows, dim) tensor")
    _check(name, t, tuple(t.shape), dtype, t.device)


def gallery_search(gallery, q, k=1, labels=None, size=None, count=None, chunk_rows=0, out=None, workspace=None,
                   threads=0):
    """The k best gallery rows of every query (yh_gallery_search) -> (scores, index), both (nq, k)
    int32. gallery (capacity, dim) int8, q (nq, dim) int8; size (1,) i32 or None: only the first
    clamp(size, 0, capacity) rows exist; labels (capacity,) i32 or None: a row with a negative label is
    no candidate; count (1,) i32 or None: queries at or beyond it have no candidates, nor has a query
    of zeros ("no feature"). A score is the exact int32 product of the two rows (16129 times the
    cosine of two `embed_quantize` rows); the order is score descending, then row ascending.
    Positions without a candidate hold the smallest int32 and index -1. chunk_rows: 0, or the rows of
    the chunks the gallery is searched in (a multiple of 64); the result does not depend on it.
    out: (scores, index) to write. workspace: a `gallery_workspace` to reuse (None: allocated per
    call)."""
    from ._lib import check, lib
    _matrix("gallery", gallery)
    _matrix("q", q)
    dev = gallery.device
    capacity, dim = gallery.shape
    nq = q.shape[0]
    _check_dim(dim)
    _check("q", q, (nq, dim), torch.int8, dev)
    k, chunk_rows = _check_k(k), _check_chunk(chunk_rows)
    if labels is not None:
        _check("labels", labels, (capacity,), torch.int32, dev)
    if size is not None:
        _check("size", size, (1,), torch.int32, dev)
    if count is not None:
        _check("count", count, (1,), torch.int32, dev)
    if out is None:
        scores = torch.empty((nq, k), dtype=torch.int32, device=dev)
        index = torch.empty((nq, k), dtype=torch.int32, device=dev)
    else:
        scores, index = out
        _check("out scores", scores, (nq, k), torch.int32, dev)
        _check("out index", index, (nq, k), torch.int32, dev)
    L = lib()
    need = L.yh_gallery_workspace_bytes(capacity, nq, k, chunk_rows)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    else:
        _check("workspace", workspace, (None,), torch.uint8, dev)
    args = (_ptr(gallery), _ptr(labels), _ptr(size), capacity, dim, _ptr(q), nq, _ptr(count), k, chunk_rows,
            _ptr(scores), _ptr(index), _ptr(workspace), workspace.numel())
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(L.yh_gallery_search(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "gallery_search")
    elif dev.type == "cpu":
        check(L.yh_gallery_search_host(*args, int(threads)), "gallery_search_host")
    else:
        raise ValueError(f"yolo_hip.gallery: unsupported device {dev}")
    return scores, index


def gallery_enrol(gallery, labels, size, q, take=None, labels_in=None, next_label=None, count=None, out=None,
                  threads=0):
    """Append query rows to a gallery in place (yh_gallery_enrol) -> rows (nq,) int32: the gallery row
    each query row took, or -1. The rows of q are walked in order; row i is enrolled iff i is below
    count (None: every row), take[i] != 0 (None: every row), the row is not all zero and the
    gallery is not full. It takes row size[0], which then grows by one, and the label labels_in[i],
    or next_label[0], which then grows by one. gallery, labels, size (1,) i32 and next_label (1,)
    i32 are updated in place; nothing is read back to the host."""
    from ._lib import check, lib
    _matrix("gallery", gallery)
    _matrix("q", q)
    dev = gallery.device
    capacity, dim = gallery.shape
    nq = q.shape[0]
    _check_dim(dim)
    _check("q", q, (nq, dim), torch.int8, dev)
    _check("labels", labels, (capacity,), torch.int32, dev)
    _check("size", size, (1,), torch.int32, dev)
    for name, t in (("take", take), ("labels_in", labels_in)):
        if t is not None:
            _check(name, t, (nq,), torch.int32, dev)
    if labels_in is None and next_label is None:
        raise ValueError("yolo_hip.gallery: without labels_in, next_label must be given")
    if next_label is not None:
        _check("next_label", next_label, (1,), torch.int32, dev)
    if count is not None:
        _check("count", count, (1,), torch.int32, dev)
    if out is None:
        out = torch.empty((nq,), dtype=torch.int32, device=dev)
    else:
        _check("out", out, (nq,), torch.int32, dev)
    L = lib()
    args = (_ptr(gallery), _ptr(labels), _ptr(size), capacity, dim, _ptr(q), nq, _ptr(count), _ptr(take),
            _ptr(labels_in), _ptr(next_label), _ptr(out))
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(L.yh_gallery_enrol(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "gallery_enrol")
    elif dev.type == "cpu":
        check(L.yh_gallery_enrol_host(*args, int(threads)), "gallery_enrol_host")
    else:
        raise ValueError(f"yolo_hip.gallery: unsupported device {dev}")
    return out


class Gallery:
    """A database of identities on one device: `data` (capacity, dim) int8 features, `labels`
    (capacity,) int32 (negative: the row is no candidate), `size` (1,) int32 rows in use and
    `next_label` (1,) int32, the label the next new identity gets. The four tensors are the whole
    state: torch.save them, assign them back, or move the gallery with to(); the bytes mean the
    same on host and device.

    search(q, k=1, count=None) -> (scores, index, labels), each (nq, k): `gallery_search` over the
    rows in use, and the labels of the rows found, -1 where there is none.
    enrol(q, take=None, labels=None, count=None) -> rows: `gallery_enrol`; labels None gives each
    enrolled row a new label. Several rows may share a label: enrol further views of an identity
    under its label instead of averaging them.
    remove(label) takes the rows of that label out of every later search (their label becomes
    -1 - label); the rows stay where they are.
    identify(features, cos_min=0.5, count=None, enrol=True) -> (labels, scores): see there.

    Launches run on the current stream and update the state in place: keep the calls of one
    Gallery on one stream. Nothing here reads a device value on the host."""

    def __init__(self, capacity, dim, device="cpu"):
        self.capacity, self.dim = int(capacity), _check_dim(dim)
        if self.capacity < 0:
            raise ValueError("yolo_hip.Gallery: capacity must be >= 0")
        self.device = torch.device(device)
        self.data = torch.zeros((self.capacity, self.dim), dtype=torch.int8, device=self.device)
        self.labels = torch.full((self.capacity,), -1, dtype=torch.int32, device=self.device)
        self.size = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.next_label = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._workspace = None

    def to(self, device):
        """Move the state to another device, in place; returns self."""
        self.device = torch.device(device)
        self.data, self.labels = self.data.to(self.device), self.labels.to(self.device)
        self.size, self.next_label = self.size.to(self.device), self.next_label.to(self.device)
        self._workspace = None
        return self

    def _ws(self, nq, k):
        from ._lib import lib
        need = lib().yh_gallery_workspace_bytes(self.capacity, nq, k, 0)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return self._workspace

    def _labels_of(self, rows):
        found = rows >= 0
        return torch.where(found, self.labels[rows.clamp(min=0).long()], torch.full_like(rows, -1)) \
            if self.capacity else torch.full_like(rows, -1)

    def search(self, q, k=1, count=None, threads=0):
        k = _check_k(k)
        scores, index = gallery_search(self.data, q, k, labels=self.labels, size=self.size, count=count,
                                       workspace=self._ws(q.shape[0], k), threads=threads)
        return scores, index, self._labels_of(index)

    def enrol(self, q, take=None, labels=None, count=None):
        return gallery_enrol(self.data, self.labels, self.size, q, take=take, labels_in=labels,
                             next_label=self.next_label, count=count)

    def remove(self, label):
        label = int(label)
        if label < 0:
            raise ValueError("yolo_hip.Gallery: a label is >= 0")
        self.labels.masked_fill_(self.labels == label, -1 - label)

    def identify(self, features, cos_min=0.5, count=None, enrol=True, threads=0):
        """Global labels for a batch of features -> (labels (nq,) int32, scores (nq,) int32).

        features (nq, dim): f32 embeddings (`Classified.embed`; quantised with `embed_quantize`) or
        int8 rows taken as they are. count (1,) i32 or None: the rows that exist (`Crops.total`).
        Each row is searched with k = 1. It is known iff its best score is at least
        ceil(cos_min * 16129), and then gets the label of the row found. An unknown row that holds a
        feature (below count, not all zero) is enrolled as a new identity and gets its new label
        (enrol=False, or a full gallery: -1). Rows without a feature get -1. scores: the best score,
        the smallest int32 where the gallery had no candidate.

        The rows a call enrols are not visible to that call's own search: two unknown rows of one
        call that show the same person get two labels. Queries of one call are not de-duplicated.
        Everything is device work on the current stream; nothing is read on the host."""
        if not isinstance(features, torch.Tensor) or features.dim() != 2:
            raise ValueError("yolo_hip.Gallery: features must be a (rows, dim) tensor")
        q = features if features.dtype == torch.int8 else embed_quantize(features, count=count, threads=threads)
        scores, index, found = self.search(q, 1, count=count, threads=threads)
        scores, found = scores[:, 0], found[:, 0]
        known = scores >= math.ceil(float(cos_min) * 16129.0)
        labels = torch.where(known, found, torch.full_like(found, -1))
        if enrol:
            rows = self.enrol(q, take=(~known).to(torch.int32), count=count)
            labels = torch.where(rows >= 0, self._labels_of(rows), labels)
        return labels, scores
