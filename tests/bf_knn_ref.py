"""NumPy restatement of k-nearest-neighbour Hamming matching and Lowe's ratio test: the
specification fvo_bf_knn_match / fvo_bf_ratio_match are tested against (tests/test_bf_knn.py).

For query descriptors Q (u8 [n0,32]) and train descriptors T (u8 [n1,32]):
  D[q,t]      popcount of the 256-bit xor.
  knn(k)      row q's neighbours are the min(k, n1) train indices with the smallest (D[q,t], t),
              in that order: cv2's batchDistance inserts with a strict <, so equal distances keep
              ascending train index.
  ratio(r)    with (t1, d1), (t2, d2) = knn(2) of row q: the row is kept iff it has two neighbours
              and float64(d1) < r * float64(d2) (one IEEE double multiply, one strict compare: what
              `m.distance < r * n.distance` computes).  mutual: additionally q is the first query
              index with the smallest D[., t1] (the cross-check of BFMatcher(crossCheck=True)).
              Rows (queryIdx, trainIdx, distance) in ascending queryIdx."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distances(Q, T):
    """int32 [n0,n1] Hamming distances."""
    Q = np.asarray(Q, np.uint8).reshape(-1, 32)
    T = np.asarray(T, np.uint8).reshape(-1, 32)
    return _POP[Q[:, None, :] ^ T[None, :, :]].sum(-1, dtype=np.int32)


def knn(Q, T, k):
    """int32 [n0,k,2] rows of (trainIdx, distance), (-1, -1) where the train set has fewer than k."""
    D = distances(Q, T)
    n0, n1 = D.shape
    out = np.full((n0, k, 2), -1, np.int32)
    m = min(k, n1)
    if n0 and m:
        idx = np.argsort(D, axis=1, kind="stable")[:, :m]
        out[:, :m, 0] = idx
        out[:, :m, 1] = np.take_along_axis(D, idx, axis=1)
    return out


def ratio(Q, T, r, mutual):
    """int32 [M,3] rows (queryIdx, trainIdx, distance) that pass the ratio test."""
    D = distances(Q, T)
    nn = knn(Q, T, 2)
    rows = []
    for q in range(D.shape[0]):
        (t1, d1), (t2, d2) = nn[q]
        if t2 < 0:
            continue  # fewer than two neighbours
        if not float(d1) < float(r) * float(d2):
            continue
        if mutual and int(np.argmin(D[:, t1])) != q:  # argmin: the first index of the minimum
            continue
        rows.append((q, t1, d1))
    return np.asarray(rows, np.int32).reshape(-1, 3)
