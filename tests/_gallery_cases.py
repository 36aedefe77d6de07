"""The specification of yh_gallery_search and yh_gallery_enrol (include/yolo_hip.h) restated in numpy,
the case list both test files walk, and the runners that put outputs inside poisoned buffers.
Every comparison made with these is equality of integers."""
import numpy as np
import torch

import yolo_hip

INT32_MIN = np.iinfo(np.int32).min
POISON = -9
CHUNKS = (0, 64, 128)


def clamp(v, hi):
    return hi if v is None else min(max(int(v), 0), hi)


def search(gallery, labels, size, q, count, k):
    """scores, index (nq, k) int32: the int32 q @ g.T, ordered by score descending then row."""
    capacity, nq = len(gallery), len(q)
    n, m = clamp(size, capacity), clamp(count, nq)
    s = q.astype(np.int32) @ gallery[:n].astype(np.int32).T
    cand = np.flatnonzero(np.ones(n, bool) if labels is None else labels[:n] >= 0)
    scores = np.full((nq, k), INT32_MIN, np.int32)
    index = np.full((nq, k), -1, np.int32)
    for i in range(nq):
        if i >= m or not q[i].any():
            continue
        order = cand[np.lexsort((cand, -s[i, cand].astype(np.int64)))][:k]
        scores[i, :len(order)] = s[i, order]
        index[i, :len(order)] = order
    return scores, index


def enrol(gallery, labels, size, q, count, take, labels_in, next_label):
    """-> gallery, labels, size, next_label, rows after the call."""
    gallery, labels = gallery.copy(), labels.copy()
    capacity, nq = len(gallery), len(q)
    n, m = clamp(size, capacity), clamp(count, nq)
    rows = np.full(nq, -1, np.int32)
    for i in range(nq):
        if i < m and (take is None or take[i] != 0) and q[i].any() and n < capacity:
            gallery[n] = q[i]
            if labels_in is None:
                labels[n] = next_label
                next_label += 1
            else:
                labels[n] = labels_in[i]
            rows[i] = n
            n += 1
    return gallery, labels, n, next_label, rows


# (dim, nq, n, k): every dim of {64, 128, 1280}, nq of {0, 1, 63, 64, 65, 130}, n of {0, 1, k - 1, k,
# 63, 64, 65, 200} and k of {1, 5, 32}; n crosses k, 64 and 128 from both sides
SEARCH_CASES = [
    (64, 0, 200, 5), (64, 1, 0, 1), (64, 63, 1, 5), (128, 64, 4, 5), (128, 65, 5, 5), (64, 130, 31, 32),
    (64, 65, 32, 32), (128, 63, 63, 32), (1280, 64, 64, 5), (64, 130, 65, 1), (1280, 130, 200, 32),
    (128, 1, 200, 1), (64, 64, 200, 5), (128, 64, 127, 5), (128, 64, 128, 5), (64, 63, 129, 32), (64, 65, 6, 5),
    (128, 130, 1, 1),
]


def search_case(dim, nq, n, k, seed=0):
    """Full-range int8 data. Rows of 127s lie beyond size and query 0 is all 127, so they would win
    if read; half the rows are copies of other rows, so ties decide; the rows that would rank first
    for every third query carry negative labels; query 2 is zero and count cuts three queries off."""
    rng = np.random.default_rng(1000 * dim + 10 * nq + n + k + seed)
    capacity = n + 7
    gallery = rng.integers(-128, 128, (capacity, dim), dtype=np.int8)
    half = n // 2
    gallery[n - half:n] = gallery[rng.permutation(n - half)[:half]] if half else gallery[n:n]
    gallery[n:] = 127
    q = rng.integers(-128, 128, (nq, dim), dtype=np.int8)
    if nq:
        q[0] = 127
    if nq > 2:
        q[2] = 0
    labels = rng.integers(0, 1000, capacity).astype(np.int32)
    if n > 2 and nq:
        s = q[::3].astype(np.int32) @ gallery[:n].astype(np.int32).T
        first = np.unique(s.argmax(1))[:max(1, n // 4)]
        labels[first] = -1 - labels[first]
    count = nq - 3 if nq > 5 else None
    return dict(gallery=gallery, labels=labels, size=n, q=q, count=count, k=k)


def ordered_case(descending, k, dim=64, nq=65, n=200):
    """Scores strictly ascending (or descending) in the row, for every query: in one order every row
    enters the running k best, in the other none after the first k."""
    v = 3 * np.arange(n) - 300
    if descending:
        v = v[::-1]
    gallery = np.repeat((v // dim)[:, None], dim, 1)
    gallery += np.arange(dim)[None, :] < (v % dim)[:, None]
    q = np.repeat(1 + np.arange(nq)[:, None] % 3, dim, 1)
    assert (gallery.sum(1) == v).all()
    return dict(gallery=gallery.astype(np.int8), labels=None, size=None, q=q.astype(np.int8), count=None, k=k)


def tie_case(k=5, dim=64, nq=63, n=200):
    """Seven distinct rows repeated: every score occurs 28 times or more, so the k-th place is a tie."""
    rng = np.random.default_rng(77)
    base = rng.integers(-128, 128, (7, dim), dtype=np.int8)
    q = rng.integers(-128, 128, (nq, dim), dtype=np.int8)
    return dict(gallery=base[np.arange(n) % 7], labels=None, size=None, q=q, count=None, k=k)


def _t(a, device, dtype=torch.int32):
    if a is None:
        return None
    if np.isscalar(a):
        a = np.array([a])
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)


def run_search(case, device="cpu", chunk_rows=0, threads=0):
    """gallery_search with the outputs inside poisoned buffers -> scores, index as numpy; asserts the
    margins and the inputs are untouched."""
    nq, k = len(case["q"]), case["k"]
    bufs = [torch.full((nq + 2, k), POISON, dtype=torch.int32, device=device) for _ in range(2)]
    g, q = _t(case["gallery"], device, torch.int8), _t(case["q"], device, torch.int8)
    labels = _t(case["labels"], device)
    out = (bufs[0][1:nq + 1], bufs[1][1:nq + 1])
    got = yolo_hip.gallery_search(g, q, k, labels=labels, size=_t(case["size"], device), count=_t(case["count"], device),
                                  chunk_rows=chunk_rows, out=out, threads=threads)
    assert got[0] is out[0] and got[1] is out[1]
    for b in bufs:
        b = b.cpu().numpy()
        assert (b[0] == POISON).all() and (b[-1] == POISON).all(), "margin"
    assert np.array_equal(g.cpu().numpy(), case["gallery"]) and np.array_equal(q.cpu().numpy(), case["q"])
    return bufs[0][1:nq + 1].cpu().numpy(), bufs[1][1:nq + 1].cpu().numpy()


# (dim, capacity, size, nq, with take, with labels_in, count): masks and zero rows; a gallery that
# fills up in the middle of a call; caller's labels; more rows than one block of the device walk;
# nothing to do; a gallery that is full already; a size beyond the capacity
ENROL_CASES = [
    (64, 300, 10, 130, True, False, None), (128, 40, 30, 65, False, False, None), (64, 300, 0, 63, True, True, 50),
    (64, 700, 5, 600, True, False, 590), (1280, 20, 3, 0, False, False, None), (64, 8, 8, 5, False, False, None),
    (64, 8, 13, 5, False, True, None), (1280, 50, 0, 64, True, False, 70), (64, 300, 250, 300, False, False, -2),
    (128, 400, 1, 257, True, True, None),
]


def enrol_case(dim, capacity, size, nq, with_take, with_labels, count):
    rng = np.random.default_rng(dim + capacity + 3 * nq)
    gallery = rng.integers(-128, 128, (capacity, dim), dtype=np.int8)
    labels = rng.integers(0, 1000, capacity).astype(np.int32)
    q = rng.integers(-128, 128, (nq, dim), dtype=np.int8)
    q[1::7] = 0
    take = (rng.integers(0, 3, nq).astype(np.int32) - 1) * 5 if with_take else None   # -5, 0, 5
    labels_in = rng.integers(0, 1 << 30, nq).astype(np.int32) if with_labels else None
    return dict(gallery=gallery, labels=labels, size=size, q=q, count=count, take=take, labels_in=labels_in,
                next_label=4242)


def run_enrol(case, device="cpu"):
    """gallery_enrol, rows_out inside a poisoned buffer -> gallery, labels, size, next_label, rows."""
    nq = len(case["q"])
    buf = torch.full((nq + 2,), POISON, dtype=torch.int32, device=device)
    g, labels = _t(case["gallery"], device, torch.int8), _t(case["labels"], device)
    size, nxt = _t(case["size"], device), _t(case["next_label"], device)
    yolo_hip.gallery_enrol(g, labels, size, _t(case["q"], device, torch.int8), take=_t(case["take"], device),
                           labels_in=_t(case["labels_in"], device), next_label=nxt, count=_t(case["count"], device),
                           out=buf[1:nq + 1])
    b = buf.cpu().numpy()
    assert b[0] == POISON and b[-1] == POISON, "margin"
    return g.cpu().numpy(), labels.cpu().numpy(), int(size.item()), int(nxt.item()), b[1:nq + 1]


def want_enrol(case):
    next_label = case["next_label"]
    g, labels, n, nxt, rows = enrol(case["gallery"], case["labels"], case["size"], case["q"], case["count"], case["take"],
                                    case["labels_in"], next_label)
    return g, labels, n, nxt if case["labels_in"] is None else next_label, rows


def same_enrol(got, want, what=""):
    for name, a, b in zip(("gallery", "labels", "size", "next_label", "rows"), got, want):
        assert np.array_equal(a, b), (what, name)


def identify_scenario(device):
    """Two cameras see noisy views of the same 20 people and 5 strangers each: the views get the
    same labels across cameras, the strangers fresh ones, and remove() makes a label unknown."""
    rng = np.random.default_rng(5)
    dim = 256
    people = rng.normal(0, 1, (20, dim))
    view = lambda x: torch.from_numpy((x + 0.3 * rng.normal(0, 1, x.shape)).astype(np.float32)).to(device)
    cam1 = torch.cat([view(people), view(rng.normal(0, 1, (5, dim)))])
    perm = rng.permutation(20)
    cam2 = torch.cat([view(rng.normal(0, 1, (5, dim))), view(people[perm])])
    gal = yolo_hip.Gallery(64, dim, device)
    l1, s1 = gal.identify(cam1)
    assert l1.dtype == torch.int32 and l1.tolist() == list(range(25)) and (s1 == INT32_MIN).all()
    assert gal.size.item() == 25 and gal.next_label.item() == 25
    l2, s2 = gal.identify(cam2)
    assert l2[5:].tolist() == perm.tolist(), "the same people under the same labels"
    assert l2[:5].tolist() == [25, 26, 27, 28, 29], "the strangers are new"
    assert (s2[5:] >= 0.8 * 16129).all() and (s2[:5] < 0.5 * 16129).all()
    assert gal.size.item() == 30 and gal.next_label.item() == 30
    l3, _ = gal.identify(cam1, enrol=False)                           # nothing new this time
    assert l3.tolist() == list(range(25)) and gal.size.item() == 30
    gal.remove(3)
    l4, _ = gal.identify(cam1[:6], enrol=False)
    assert l4.tolist() == [0, 1, 2, -1, 4, 5]
    assert gal.labels[3].item() == -4 and gal.size.item() == 30
    l5, _ = gal.identify(cam1[:6])                                     # unknown again: a new identity
    assert l5.tolist() == [0, 1, 2, 30, 4, 5] and gal.size.item() == 31
    # int8 features are taken as they are, zero rows and rows beyond count have no identity
    q = yolo_hip.embed_quantize(cam2)
    q[7] = 0
    l6, _ = gal.identify(q, count=torch.tensor([20], dtype=torch.int32, device=device))
    want = [30 if v == 3 else v for v in l2.tolist()]                  # person 3 lives under label 30 now
    want[7] = -1
    want[20:] = [-1] * 5
    assert l6.tolist() == want and gal.size.item() == 31
    return gal
