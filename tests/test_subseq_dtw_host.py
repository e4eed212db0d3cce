"""CPU: alignment.subseq_dtw_host, the numpy restatement of asr_dtw_subseq_batch_dev's definition, against an
independent derivation - full DTW against a virtual zero-cost row - and on planted excerpts."""
import numpy as np
import pytest


def _via_zero_row(D):
    """Subsequence DTW as full DTW: prepend a row of zeros to D and let the path start anywhere in it.  With the
    accumulated cost of the zero row held at 0 (walking along it is free) the cell (1, j) of the padded matrix costs
    D[0][j] whichever of its predecessors it takes, which is the free start; the last row's first minimum ends the
    path, the traceback (diagonal, up, left; first minimum) stops when it reaches the zero row, and that row is
    removed.  Written cell by cell, with its own border handling."""
    Q, S = D.shape
    P = np.vstack([np.zeros((1, S)), D])
    A = np.empty_like(P)
    A[0] = 0.0
    for i in range(1, Q + 1):
        for j in range(S):
            if i == 1:
                best = 0.0                                  # every predecessor lies in the zero row (or outside)
            else:
                best = A[i - 1][j]
                if j > 0:
                    best = min(best, A[i - 1][j - 1], A[i][j - 1])
            A[i][j] = P[i][j] + best
    end = min(range(S), key=lambda j: (A[Q][j], j))
    i, j, path = Q, end, [(Q, end)]
    while i > 1:                                            # pinned first step: row 1 is entered from the zero row
        cands = [(A[i - 1][j - 1] if j > 0 else np.inf, 0), (A[i - 1][j], 1), (A[i][j - 1] if j > 0 else np.inf, 2)]
        w = min(cands)[1]
        i, j = i - (w != 2), j - (w != 1)
        path.append((i, j))
    path = path[::-1]
    rows, cols = np.array([p[0] - 1 for p in path]), np.array([p[1] for p in path])
    return A[Q][end] / Q, cols[0], end, (rows, cols)


def _check(D):
    from audio_sheet_retrieval_amd import alignment as al
    cost, start, end, path = al.subseq_dtw_host(D)
    rcost, rstart, rend, rpath = _via_zero_row(np.asarray(D, np.float64))
    assert cost == rcost and start == rstart and end == rend
    assert np.array_equal(path[0], rpath[0]) and np.array_equal(path[1], rpath[1])
    Q, S = D.shape
    rows, cols = path
    # monotone, steps of (1,1), (1,0), (0,1), every query row covered, the ends where they are said to be
    steps = set(zip(np.diff(rows).tolist(), np.diff(cols).tolist()))
    assert steps <= {(1, 1), (1, 0), (0, 1)}
    assert rows[0] == 0 and rows[-1] == Q - 1 and cols[0] == start and cols[-1] == end
    assert sorted(set(rows.tolist())) == list(range(Q))
    assert int(np.sum(rows == 0)) == 1                      # the path stops when it reaches row 0
    loop = [int(cols[np.flatnonzero(rows == i)[0]]) for i in range(Q)]
    assert np.array_equal(al.subseq_positions(path, Q), loop)
    return cost, start, end


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (5, 5), (7, 30), (30, 7), (40, 90)])
def test_random_matrices(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for _ in range(4):
        _check(rng.random(shape))


@pytest.mark.parametrize("shape", [(1, 6), (6, 1), (8, 8), (12, 40), (40, 12)])
def test_tie_heavy_matrices(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    for _ in range(6):
        _check(rng.choice([0.0, 0.5, 1.0], size=shape))
    _check(np.zeros(shape))                                 # all equal: the first-minimum rules alone decide
    cost, start, end = _check(np.ones(shape))
    assert end == 0 or shape[0] == 1 and end == 0           # first minimum of the last row


def test_bad_input_is_refused():
    from audio_sheet_retrieval_amd import alignment as al
    for bad in (np.zeros((0, 3)), np.zeros((3, 0)), np.zeros(4)):
        with pytest.raises(ValueError):
            al.subseq_dtw_host(bad)


def _planted(seed):
    """S in 150..400 independent standard-normal rows; the query: rows linspace(s0, s0 + L - 1, Q) of the reference
    plus 0.3 x noise, normalised; L in 30..90, Q between 0.6 and 1.6 times L.  The linspace positions are rounded to the
    nearest row: truncating them would give the stretch's last row a single query row whatever the tempo, while every
    other row gets Q / L of them, and the end of such a query is not where the stretch ends."""
    rng = np.random.default_rng(seed)
    S = int(rng.integers(150, 401))
    ref = rng.standard_normal((S, 32))
    L = int(rng.integers(30, 91))
    Q = int(round(L * rng.uniform(0.6, 1.6)))
    s0 = int(rng.integers(0, S - L + 1))
    rows = np.round(np.linspace(s0, s0 + L - 1, Q)).astype(int)
    qry = ref[rows] + 0.3 * rng.standard_normal((Q, 32))
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return unit(qry), unit(ref), unit(rng.standard_normal((S, 32))), s0, L


@pytest.mark.parametrize("seed", range(20))
def test_planted_excerpts_are_found(seed):
    from audio_sheet_retrieval_amd import alignment as al
    qry, ref, other, s0, L = _planted(seed)
    cost, start, end, path = al.subseq_dtw_host(al.cosine_dists_host(qry, ref))
    print("seed %d: start off by %d, end off by %d, cost %.3f" % (seed, start - s0, end - (s0 + L - 1), cost))
    assert abs(start - s0) <= 2 and abs(end - (s0 + L - 1)) <= 2
    cost_other = al.subseq_dtw_host(al.cosine_dists_host(qry, other))[0]
    print("         cost against a fresh random reference %.3f" % cost_other)
    assert cost < cost_other


def test_cosine_dists_host_is_scipys():
    from scipy.spatial.distance import cdist
    from audio_sheet_retrieval_amd import alignment as al
    rng = np.random.default_rng(3)
    for dim in (1, 2, 5, 31, 32, 64):
        a, b = rng.standard_normal((9, dim)).astype(np.float32), rng.standard_normal((13, dim)).astype(np.float32)
        assert np.array_equal(al.cosine_dists_host(a, b), cdist(a.astype(np.float64), b.astype(np.float64), "cosine")), dim
