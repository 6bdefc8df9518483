"""k-nearest-neighbour Hamming matching and Lowe's ratio test: fvo_bf_knn_match /
fvo_bf_ratio_match, their bindings, the cv2 shim's DescriptorMatcher and the front ends'
match_ratio, against the NumPy restatement tests/bf_knn_ref.py.  Distances are integers and the
ratio decision is one IEEE multiply and compare, so every GPU comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

import bf_knn_ref as ref
from conftest import gpu_available
from sanitize_build import run_check


def _desc(rows):
    """Descriptors with the given numbers of set bits: row i has bits 0 .. rows[i]-1 set."""
    d = np.zeros((len(rows), 32), np.uint8)
    for i, n in enumerate(rows):
        bits = np.zeros(256, np.uint8)
        bits[:n] = 1
        d[i] = np.packbits(bits)
    return d


# ----------------------------------------------------------------------------- known answers
def test_restatement_distance_and_tie_order():
    Q = _desc([0, 3])
    T = _desc([2, 1, 2, 0, 5])              # from query 0: 2 1 2 0 5; from query 1: 1 2 1 3 2
    assert np.array_equal(ref.distances(Q, T), [[2, 1, 2, 0, 5], [1, 2, 1, 3, 2]])
    # equal distances keep ascending train index
    assert np.array_equal(ref.knn(Q, T, 3), [[[3, 0], [1, 1], [0, 2]], [[0, 1], [2, 1], [1, 2]]])
    assert np.array_equal(ref.knn(Q, T, 1), [[[3, 0]], [[0, 1]]])
    assert np.array_equal(ref.knn(Q, T, 5)[1], [[0, 1], [2, 1], [1, 2], [4, 2], [3, 3]])
    assert np.array_equal(ref.distances(np.full((1, 32), 255, np.uint8), np.zeros((1, 32), np.uint8)), [[256]])


def test_restatement_fewer_train_rows_than_k():
    Q = _desc([0, 3, 7])
    T = _desc([2, 1])
    want = [[[1, 1], [0, 2], [-1, -1]], [[0, 1], [1, 2], [-1, -1]], [[0, 5], [1, 6], [-1, -1]]]
    assert np.array_equal(ref.knn(Q, T, 3), want)
    assert ref.knn(Q, T[:0], 2).shape == (3, 2, 2) and (ref.knn(Q, T[:0], 2) == -1).all()
    assert ref.knn(Q[:0], T, 2).shape == (0, 2, 2)


def test_restatement_ratio_needs_two_neighbours():
    Q = _desc([0, 3])
    assert ref.ratio(Q, _desc([0]), 1.0, 0).shape == (0, 3)    # n1 == 1: every row is dropped
    assert ref.ratio(Q, _desc([0]), 100.0, 1).shape == (0, 3)
    assert ref.ratio(Q, _desc([])[:0], 0.75, 0).shape == (0, 3)
    assert ref.ratio(Q[:0], _desc([0, 1]), 0.75, 0).shape == (0, 3)


def test_restatement_ratio_compare_is_strict():
    Q = _desc([0])
    T = _desc([4, 2])                        # distances 4 and 2: d1 = 2 (train 1), d2 = 4
    assert ref.ratio(Q, T, 0.5, 0).shape == (0, 3)                 # 2 < 0.5 * 4 is false
    assert np.array_equal(ref.ratio(Q, T, 0.51, 0), [[0, 1, 2]])
    assert np.array_equal(ref.ratio(Q, _desc([4, 1]), 0.5, 0), [[0, 1, 1]])
    # d1 == d2 is never kept at a ratio <= 1, d1 = d2 = 0 at no ratio
    assert ref.ratio(Q, _desc([3, 3]), 1.0, 0).shape == (0, 3)
    assert ref.ratio(Q, _desc([0, 0]), 1e9, 0).shape == (0, 3)
    # the product is formed in double: 0.55 * 100 = 55.00000000000001 > 55
    assert np.array_equal(ref.ratio(Q, _desc([100, 55]), 0.55, 0), [[0, 1, 55]])
    assert ref.ratio(Q, _desc([100, 56]), 0.55, 0).shape == (0, 3)


def test_restatement_mutual_drops_a_one_sided_best_match():
    Q = _desc([10, 12])
    T = _desc([12, 40])                      # query 0 -> train 0 at 2, but train 0's nearest is query 1 at 0
    assert np.array_equal(ref.ratio(Q, T, 0.75, 0), [[0, 0, 2], [1, 0, 0]])
    assert np.array_equal(ref.ratio(Q, T, 0.75, 1), [[1, 0, 0]])
    # the reverse tie goes to the first query index
    Q2 = _desc([12, 12])
    assert np.array_equal(ref.ratio(Q2, T, 0.75, 0), [[0, 0, 0], [1, 0, 0]])
    assert np.array_equal(ref.ratio(Q2, T, 0.75, 1), [[0, 0, 0]])


# ----------------------------------------------------------------------------- descriptor sets
SIZES = [(300, 257), (65, 513), (64, 64), (256, 256), (1, 2), (5, 1), (0, 10), (10, 0)]
RATIOS = (0.75, 0.8, 1.0)
KS = (1, 2, 3, 8)
CAP = 1024


def _make_set(n0, n1, seed):
    """Train rows random, the last 4 duplicating the first 4 (exact ties); two thirds of the query
    rows copies of distinct train rows with 0..89 random bit flips, the rest random."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    if n1 >= 8:
        T[-4:] = T[:4]
    Q = rng.integers(0, 256, (n0, 32), dtype=np.uint8)
    ncopy = min(2 * n0 // 3, n1)
    src = rng.permutation(n1)[:ncopy]
    for q, t in enumerate(src):
        bits = np.unpackbits(T[t])
        bits[rng.choice(256, int(rng.integers(0, 90)), replace=False)] ^= 1
        Q[q] = np.packbits(bits)
    return Q, T


def _tie_heavy():
    """tests/test_gpu_parity.py::test_bf_match_bit_exact's adversarial set: 8 distinct descriptors."""
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, size=(8, 32), dtype=np.uint8)
    r0 = base[rng.integers(0, 8, 700)]
    r1 = base[rng.integers(0, 8, 650)]
    r1[::3, 0] ^= 1
    return r0, r1


@functools.lru_cache(maxsize=None)
def _sets():
    return [_make_set(n0, n1, seed) for seed, (n0, n1) in enumerate(SIZES)] + [_tie_heavy()]


@functools.lru_cache(maxsize=None)
def _want_knn(k):
    return [ref.knn(Q, T, k) for Q, T in _sets()]


@functools.lru_cache(maxsize=None)
def _want_ratio(r, mutual):
    return [ref.ratio(Q, T, r, mutual) for Q, T in _sets()]


def test_descriptor_sets_exercise_the_ratio_test():
    """The figures the GPU tests' "keeps some, drops some" rests on, from the restatement alone."""
    sets = _sets()
    count = lambda r, m, i: len(_want_ratio(r, m)[i])  # noqa: E731
    nn = _want_knn(2)
    ties = [int(((n[:, 0, 1] == n[:, 1, 1]) & (n[:, 1, 0] >= 0)).sum()) for n in nn]
    # 300x257 and 65x513 at ratio 0.75: rows are kept and rows are dropped, some of them on d1 == d2
    assert (count(0.75, 0, 0), ties[0]) == (170, 25) and (count(0.75, 0, 1), ties[1]) == (38, 4)
    assert (count(0.8, 0, 0), count(0.8, 0, 1)) == (185, 42)
    # ratio 1.0 separates mutual on and off
    assert (count(1.0, 0, 0), count(1.0, 1, 0)) == (275, 202)
    assert (count(1.0, 0, 1), count(1.0, 1, 1)) == (61, 58)
    for r in RATIOS:
        for m in (0, 1):
            assert count(r, m, 8) == 0 and ties[8] == 700      # tie-heavy: d1 == d2 in every row
            assert all(count(r, m, i) == 0 for i in (5, 6, 7))  # n1 < 2 or n0 == 0
    # mutual rows are a subset of the non-mutual ones, and injective in trainIdx
    for i in range(len(sets)):
        a, b = _want_ratio(1.0, 0)[i], _want_ratio(1.0, 1)[i]
        assert set(map(tuple, b)) <= set(map(tuple, a)) and len(set(b[:, 1])) == len(b)


# ----------------------------------------------------------------------------- library surface
def test_library_exports_the_new_entry_points():
    from forest_slam_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert L.fvo_abi_version() == 7 == _lib.ABI_VERSION
    for name in ("fvo_bf_knn_match", "fvo_bf_ratio_match"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    L.fvo_kernel_name.restype = ctypes.c_char_p
    names = [L.fvo_kernel_name(i).decode() for i in range(L.fvo_kernel_count())]
    assert "bf_knn" in names and "bf_ratio" in names and len(set(names)) == len(names) <= 64
    # the new ids sit before the speckle filter's (which stay the last four); nothing before them moved
    assert names.index("bf_argmin") == 13 and names.index("voxel_down_sample") == 29


def test_shim_refusals():
    from forest_slam_amd import cv2_compat as cv2
    assert cv2.DescriptorMatcher_BRUTEFORCE_HAMMING == 4
    for kind in ("BruteForce-Hamming", cv2.DescriptorMatcher_BRUTEFORCE_HAMMING):
        assert isinstance(cv2.DescriptorMatcher_create(kind), cv2.HammingDescriptorMatcher)
    for kind in ("BruteForce", "BruteForce-L1", "BruteForce-Hamming(2)", "FlannBased", 1, 2, 3, 5, 6):
        with pytest.raises(NotImplementedError):
            cv2.DescriptorMatcher_create(kind)
    with pytest.raises(NotImplementedError, match="DescriptorMatcher_create"):
        cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=False)
    d = np.zeros((4, 32), np.uint8)
    m = cv2.DescriptorMatcher_create("BruteForce-Hamming")
    for k in (0, -1):
        with pytest.raises(cv2.error):
            m.knnMatch(d, d, k)
    with pytest.raises(NotImplementedError):
        m.knnMatch(d, d, 9)
    with pytest.raises(NotImplementedError):
        m.knnMatch(d, d, 2, mask=np.ones((4, 4), np.uint8))
    with pytest.raises(NotImplementedError):
        m.match(d, d, mask=np.ones((4, 4), np.uint8))
    with pytest.raises(cv2.error):
        m.knnMatch(np.zeros((4, 16), np.uint8), d, 2)
    bf = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True)
    with pytest.raises(cv2.error):
        bf.knnMatch(d, d, 2)                 # cv2: crossCheck allows k == 1 only
    with pytest.raises(cv2.error):
        bf.knnMatch(d, d, 0)
    with pytest.raises(NotImplementedError):
        bf.knnMatch(d, d, 1, mask=np.ones((4, 4), np.uint8))


def test_front_end_arguments_are_checked_before_the_gpu():
    from forest_slam_amd import cv2_compat as cv2, vo
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            vo._match_ratio(bad)
        with pytest.raises(cv2.error):
            cv2.ORBMatching({"match_ratio": bad})
    assert vo._match_ratio(0) == 0.0 and cv2.ORBMatching({"match_ratio": 0.8}).match_ratio == 0.8
    assert cv2.ORBMatching().match_ratio == 0.0


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU error")
def test_shim_without_gpu_raises():
    from forest_slam_amd import cv2_compat as cv2
    d = np.zeros((4, 32), np.uint8)
    m = cv2.DescriptorMatcher_create("BruteForce-Hamming")
    with pytest.raises(RuntimeError):
        m.knnMatch(d, d, 2)
    with pytest.raises(RuntimeError):
        m.match(d, d)
    with pytest.raises(RuntimeError):
        cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True).knnMatch(d, d, 1)


def test_host_validation_under_sanitizers(tmp_path):
    """fvo_bf_knn_match and fvo_bf_ratio_match of csrc/capi.cpp (every refusal, the k bound, null
    pointers, cap overflow, the no-launch case) as a stand-alone ASan + UBSan program:
    tests/sanitize/bf_knn_check.cpp."""
    run_check("bf_knn_check", tmp_path)


# ----------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _ctx():
    from forest_slam_amd import _lib
    return _lib.Context(64, 64, max_batch=8, stages=_lib.STAGE_BF, kp_capacity=CAP)


def _pack(sets):
    """[(Q, T)] -> device tensors (q u8 [B,CAP,32], nq i32 [B], t, nt).  The padding rows hold
    0xFF bytes in q and zeros in t: nothing past a set's end may take part."""
    import torch
    B = len(sets)
    q = np.full((B, CAP, 32), 255, np.uint8)
    t = np.zeros((B, CAP, 32), np.uint8)
    nq, nt = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for i, (a, b) in enumerate(sets):
        q[i, :len(a)], t[i, :len(b)] = a, b
        nq[i], nt[i] = len(a), len(b)
    return tuple(torch.from_numpy(x).cuda() for x in (q, nq, t, nt))


# The context serves 8 sets per call: the eight sized sets go in one batched call, the tie-heavy
# ninth in a call of its own.
def _calls():
    s = _sets()
    return [(0, s[:8]), (8, s[8:])]


def _rows(m, nm, i):
    return m[i, :nm[i]]


def _gpu_ratio(sets, r, mutual):
    m, nm = _ctx().bf_ratio_match(*_pack(sets), r, mutual=bool(mutual))
    return m.cpu().numpy(), nm.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
@pytest.mark.parametrize("k", KS)
def test_gpu_knn_equals_restatement(k):
    import torch
    for first, sets in _calls():
        q, nq, t, nt = _pack(sets)
        out = torch.full((len(sets), CAP, k, 2), -7, dtype=torch.int32, device="cuda")
        got = _ctx().bf_knn_match(q, nq, t, nt, k, out=out)
        assert got is out
        got = got.cpu().numpy()
        for i, (a, b) in enumerate(sets):
            want = _want_knn(k)[first + i]
            assert np.array_equal(got[i, :len(a)], want), (k, first + i, a.shape, b.shape)
            assert (got[i, len(a):] == -7).all()         # rows >= n_query are not written


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
@pytest.mark.parametrize("mutual", (0, 1))
@pytest.mark.parametrize("r", RATIOS)
def test_gpu_ratio_equals_restatement(r, mutual):
    for first, sets in _calls():
        m, nm = _gpu_ratio(sets, r, mutual)
        for i in range(len(sets)):
            want = _want_ratio(r, mutual)[first + i]
            assert nm[i] == len(want), (r, mutual, first + i, int(nm[i]), len(want))
            assert np.array_equal(_rows(m, nm, i), want), (r, mutual, first + i)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_ratio_known_answers():
    """The strict compare and the double product of the hand-written cases, on the device."""
    Q = _desc([0])
    for r, sets, want in ((0.5, [(Q, _desc([4, 2])), (Q, _desc([4, 1])), (Q, _desc([3, 3])), (Q, _desc([7]))],
                           [[], [[0, 1, 1]], [], []]),
                          (0.55, [(Q, _desc([100, 55])), (Q, _desc([100, 56]))], [[[0, 1, 55]], []]),
                          (1e9, [(Q, _desc([0, 0])), (Q, _desc([0, 1]))], [[], [[0, 0, 0]]])):
        m, nm = _gpu_ratio(sets, r, 0)
        for i, w in enumerate(want):
            assert np.array_equal(_rows(m, nm, i), np.asarray(w, np.int32).reshape(-1, 3)), (r, i)
            assert np.array_equal(_rows(m, nm, i), ref.ratio(*sets[i], r, 0))
    # a one-sided best match: kept without the reverse check, dropped with it
    sets = [(_desc([10, 12]), _desc([12, 40])), (_desc([12, 12]), _desc([12, 40]))]
    for mutual, want in ((0, [[[0, 0, 2], [1, 0, 0]], [[0, 0, 0], [1, 0, 0]]]), (1, [[[1, 0, 0]], [[0, 0, 0]]])):
        m, nm = _gpu_ratio(sets, 0.75, mutual)
        for i, w in enumerate(want):
            assert np.array_equal(_rows(m, nm, i), w), (mutual, i)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_mutual_rows_are_a_subset_of_bf_match():
    for first, sets in _calls():
        packed = _pack(sets)
        cm, cnm = (x.cpu().numpy() for x in _ctx().bf_match(*packed))
        for r in RATIOS:
            m, nm = (x.cpu().numpy() for x in _ctx().bf_ratio_match(*packed, r, mutual=True))
            for i in range(len(sets)):
                cross = set(map(tuple, _rows(cm, cnm, i)))
                assert set(map(tuple, _rows(m, nm, i))) <= cross, (r, first + i)
        assert first != 0 or (cnm[0] > len(_want_ratio(1.0, 1)[0]) > 0)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_calls_leave_no_state(oracle_mod):
    """bf_ratio_match, then bf_match, then bf_ratio_match and bf_knn_match on other data, on one
    context: every result equals its reference, and bf_match the oracle's."""
    s = _sets()
    first, second = [s[0], s[1], s[8]], [s[3], s[2], s[0]]
    ctx = _ctx()
    m, nm = _gpu_ratio(first, 0.8, 1)
    for i, j in enumerate((0, 1, 8)):
        assert np.array_equal(_rows(m, nm, i), _want_ratio(0.8, 1)[j]), j
    for sets in (first, second):
        cm, cnm = (x.cpu().numpy() for x in ctx.bf_match(*_pack(sets)))
        for i, (a, b) in enumerate(sets):
            assert np.array_equal(_rows(cm, cnm, i), oracle_mod.bf_match(a, b)), i
    for mutual in (1, 0):
        m, nm = _gpu_ratio(second, 0.8, mutual)
        for i, j in enumerate((3, 2, 0)):
            assert np.array_equal(_rows(m, nm, i), _want_ratio(0.8, mutual)[j]), (mutual, j)
    got = ctx.bf_knn_match(*_pack(second), 2).cpu().numpy()
    for i, j in enumerate((3, 2, 0)):
        assert np.array_equal(got[i, :len(second[i][0])], _want_knn(2)[j]), j
    cm, cnm = (x.cpu().numpy() for x in ctx.bf_match(*_pack(first)))
    assert np.array_equal(_rows(cm, cnm, 2), oracle_mod.bf_match(*first[2]))


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_argument_errors_reach_python():
    q, nq, t, nt = _pack(_sets()[:2])
    ctx = _ctx()
    for k in (0, 9):
        with pytest.raises(RuntimeError, match="k must be"):
            ctx.bf_knn_match(q, nq, t, nt, k)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="ratio must be"):
            ctx.bf_ratio_match(q, nq, t, nt, r)
    with pytest.raises(TypeError):
        ctx.bf_knn_match(q, nq, t, nt, 2, out=q)
    # the context still works
    m, nm = _gpu_ratio(_sets()[:2], 0.75, 0)
    assert np.array_equal(_rows(m, nm, 1), _want_ratio(0.75, 0)[1])


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_cv2_shim():
    import torch
    from forest_slam_amd import cv2_compat as cv2
    m = cv2.DescriptorMatcher_create("BruteForce-Hamming")
    for i in (0, 1, 4):
        Q, T = _sets()[i]
        knn = m.knnMatch(Q, T, k=2)
        assert len(knn) == len(Q) and all(len(row) == 2 for row in knn)
        got = [[x.queryIdx, x.trainIdx, int(x.distance)] for x, y in knn if x.distance < 0.75 * y.distance]
        assert np.array_equal(np.asarray(got, np.int32).reshape(-1, 3), _want_ratio(0.75, 0)[i]), i
        dev = m.knnMatchDevice(torch.from_numpy(Q), torch.from_numpy(T), 2)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), _want_knn(2)[i])
        one = m.match(Q, T)
        assert [[x.trainIdx, int(x.distance)] for x in one] == _want_knn(1)[i][:, 0].tolist()
        assert [x.queryIdx for x in one] == list(range(len(Q)))
    # shorter lists where the train set is: n1 == 1 gives singletons, n1 == 0 empty lists
    Q, T = _sets()[5]
    assert [len(row) for row in m.knnMatch(Q, T, 3)] == [1] * 5 and len(m.match(Q, T)) == 5
    assert m.knnMatch(Q, T[:0], 2) == [[]] * 5 and m.match(Q, T[:0]) == [] and m.knnMatch(Q[:0], T, 2) == []
    # the cross-checked matcher: k == 1 only, its matches as singleton or empty lists
    bf = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True)
    Q, T = _sets()[0]
    flat = bf.match(Q, T)
    lists = bf.knnMatch(Q, T, 1)
    assert len(lists) == len(Q) and max(len(row) for row in lists) == 1 and min(len(row) for row in lists) == 0
    assert [(x.queryIdx, x.trainIdx, x.distance) for row in lists for x in row] == [
        (x.queryIdx, x.trainIdx, x.distance) for x in flat]


# ----------------------------------------------------------------------------- front end
W, H = 320, 200


def _frames(seed, n, start=0):
    import torch
    from forest_slam_amd import synth
    seq = synth.StereoSequence(seed=seed, n_frames=n, W=W, H=H, device="cuda", start=start)
    L, R = seq.frames(range(n))
    torch.cuda.synchronize()
    return seq, L, R


def _fe(seq, **kw):
    from forest_slam_amd import synth, vo
    return vo.StereoFrontEnd(W, H, seq.K, synth.DIST_L, synth.BASELINE, batch=2, nfeatures=300, num_disparities=64,
                             ba_window=3, **kw)


def _step_state(fe, T, st, nb=4):
    """Host copies of a step's outputs and of its match lists (the valid rows only)."""
    import torch
    torch.cuda.synchronize()
    nm = fe.nmatch[:nb].cpu().numpy().copy()
    m = fe.matches[:nb].cpu().numpy()
    return dict(T=T.cpu().numpy().copy(), st=st.cpu().numpy().copy(), nm=nm, rows=[m[i, :nm[i]].copy() for i in range(nb)])


def _same(a, b):
    return (a["T"].tobytes() == b["T"].tobytes() and a["st"].tobytes() == b["st"].tobytes() and
            a["nm"].tobytes() == b["nm"].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a["rows"], b["rows"])))


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_frontend_match_ratio():
    import torch
    seq, L, R = _frames(33, 5, start=80)
    fe = _fe(seq, match_ratio=0.8)
    fe.prime(L[0], R[0])
    T, st = fe.step(L[1:3], R[1:3])
    got = _step_state(fe, T, st)
    assert (got["st"] == 1).all(), got["st"]
    # the match buffers hold the restatement's rows for the step's own descriptor sets (previous
    # -> current, left frames then right frames)
    qd, qn = fe.q_desc[:4].cpu().numpy(), fe.q_cnt[:4].cpu().numpy()
    td, tn = fe.desc[:4].cpu().numpy(), fe.cnt[:4].cpu().numpy()
    cross_total = 0
    for i in range(4):
        assert qn[i] > 0 and tn[i] > 0
        want = ref.ratio(qd[i, :qn[i]], td[i, :tn[i]], 0.8, 1)
        assert got["nm"][i] == len(want) > 0 and np.array_equal(got["rows"][i], want), i
        cross_total += len(ref.ratio(qd[i, :qn[i]], td[i, :tn[i]], 1e9, 1))
    assert sum(got["nm"]) < cross_total                      # the ratio test dropped matches
    second = _step_state(fe, *fe.step(L[3:5], R[3:5]))
    # one step captured in a HIP graph replays to the eager step's bytes
    g_fe = _fe(seq, match_ratio=0.8)
    g_fe.prime(L[0], R[0])
    g_fe.step(L[1:3], R[1:3])
    Ls, Rs = L[1:3].clone(), R[1:3].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Tg, stg = g_fe.step(Ls, Rs)
    Ls.copy_(L[3:5])
    Rs.copy_(R[3:5])
    g.replay()
    assert _same(_step_state(g_fe, Tg, stg), second)


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")
def test_gpu_frontend_match_ratio_0_is_the_default_path():
    seq, L, R = _frames(33, 3, start=80)
    states, kernels = [], []
    for kw in ({}, {"match_ratio": 0}, {"match_ratio": 0.8}):
        fe = _fe(seq, **kw)
        fe.prime(L[0], R[0])
        fe.ctx.timing_enable(None)
        T, st = fe.step(L[1:3], R[1:3])
        kernels.append({k: v[1] for k, v in fe.ctx.timing_read().items() if k.startswith("bf_")})
        fe.ctx.timing_enable([])
        states.append(_step_state(fe, T, st))
    assert _same(states[0], states[1]) and not _same(states[0], states[2])
    assert kernels[0] == kernels[1] == {"bf_argmin": 1, "bf_finish": 1}
    assert kernels[2] == {"bf_knn": 1, "bf_ratio": 1}
