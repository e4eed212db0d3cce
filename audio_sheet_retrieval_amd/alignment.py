"""Audio-to-sheet alignment on top of the embedding space: distance matrix + DTW on the GPU.

Mirror of audio_sheet_retrieval/utils/alignment.py:112-186 (align_baseline, align_pydtw, compute_alignment,
estimate_alignment_error) with utils/dtw_by_dist.py:dtw_by_dist behind it.  The cosine distance matrix, the accumulated
cost (anti-diagonal wavefront) and the traceback run in the library (asr_dtw_dev, float64, bit-exact with the
reference's NumPy arithmetic); the O(n) path post-processing and the interpolation stay on the host as in the reference.
The *_batch / compute_alignments variants align many pieces in one library call (asr_dtw_batch_dev: all pairs in one
launch per stage, the first-entry projection of align_pydtw computed on the device) with identical results.
"""
from __future__ import print_function

import numpy as np
from scipy.interpolate import interp1d


def dtw_by_dist_codes(engine, img_codes, spec_codes):
    """dtw_by_dist(cdist(img_codes, spec_codes, "cosine")) (utils/dtw_by_dist.py:5-34) -> (min_dist, dists, path):
    the reference transposes a wide matrix and swaps the returned path when it did NOT transpose (:13-15, :30-31)."""
    n_r, n_c = len(img_codes), len(spec_codes)
    if n_c > n_r:                                        # transposed = True: rows = spec codes
        md, d, p, q = engine.dtw(spec_codes, img_codes)
        return md, d.T, (p, q)
    md, d, p, q = engine.dtw(img_codes, spec_codes)
    return md, d, (q, p)


def dtw_by_dist_codes_batch(engine, pairs, want_dists=True, first=False, path=True):
    """dtw_by_dist_codes for a list of (img_codes, spec_codes) pairs in one call -> [(min_dist, dists, path)], with the
    same per-pair transposition.  first=True appends, per pair, the sheet index of the first path entry of every audio
    excerpt (align_pydtw's projection: path[1][first_entries(path[0], n_spec)]).  path=False: distances only
    (min_dist and path None)."""
    jobs, flipped = [], []
    for img, spec in pairs:
        wide = len(spec) > len(img)                      # rows = spec codes (transposed)
        jobs.append((spec, img) if wide else (img, spec))
        flipped.append(wide)
    res = engine.dtw_batch(jobs, want_dists=want_dists, want_path=path,
                           first_of=(["a" if w else "b" for w in flipped] if first else None))
    out = []
    for wide, r in zip(flipped, res):
        md, d, p, q = r[:4]
        item = (md, (d.T if wide else d) if d is not None else None, None if p is None else (p, q) if wide else (q, p))
        out.append(item + (r[4],) if first else item)
    return out


def first_entries(path0, n):
    """index of the first entry of every value 0..n-1 in a non-decreasing path row that visits each of them - the
    `np.flatnonzero(path[0] == col)[0]` loop of align_pydtw (utils/alignment.py:131-138) in O(len + n)"""
    return np.searchsorted(np.asarray(path0), np.arange(n), side="left")


def align_baseline(dists):
    """straight line from the first to the last sheet position, one value per audio excerpt (:112-116)"""
    return np.linspace(0, dists.shape[0] - 1, dists.shape[1])


def align_pydtw(engine, img_codes, spec_codes):
    """DTW alignment (:119-140): the sheet position of the first path entry of every audio excerpt"""
    _, dists, path = dtw_by_dist_codes(engine, img_codes, spec_codes)
    first = [int(np.flatnonzero(path[0] == col)[0]) for col in range(dists.shape[1])]
    return np.asarray(path[1])[first], dists


def compute_alignment(engine, img_codes, spec_codes, sheet_idxs, spec_idxs, align_by):
    """Audio frame -> sheet x-coordinate mapping (:143-177).  Returns (mapping dict, dict of intermediate results
    under the reference's keys)."""
    if align_by == "baseline":
        dists = engine.dtw(img_codes, spec_codes)[1]           # only the distance matrix is used here
        positions = align_baseline(dists)
    elif align_by == "pydtw":
        positions, dists = align_pydtw(engine, img_codes, spec_codes)
    else:
        raise ValueError("align_by must be 'baseline' or 'pydtw'")
    return _interpolate(positions, dists, sheet_idxs, spec_idxs)


def compute_alignments(engine, pieces, align_by):
    """compute_alignment for a list of pieces (img_codes, spec_codes, sheet_idxs, spec_idxs) with one library call for
    all of them -> [(mapping, details)], identical to calling compute_alignment per piece.  'baseline' computes only the
    distance matrices."""
    if align_by not in ("baseline", "pydtw"):
        raise ValueError("align_by must be 'baseline' or 'pydtw'")
    pydtw = align_by == "pydtw"
    res = dtw_by_dist_codes_batch(engine, [(img, spec) for img, spec, _, _ in pieces], first=pydtw, path=pydtw)
    out = []
    for (_, _, sheet_idxs, spec_idxs), r in zip(pieces, res):
        dists = r[1]
        positions = r[3] if pydtw else align_baseline(dists)
        out.append(_interpolate(positions, dists, sheet_idxs, spec_idxs))
    return out


def _interpolate(positions, dists, sheet_idxs, spec_idxs):
    """:157-177 - rounded sheet positions -> coordinates -> interpolated frame -> x mapping"""
    positions = np.round(positions).astype(np.int64)
    coords = sheet_idxs[positions]
    # excerpts whose frame index did not advance carry no new information for the interpolation (:163)
    advancing = np.diff(np.concatenate((spec_idxs[:1] - 1, spec_idxs))) > 0
    frames = np.arange(spec_idxs[0], spec_idxs[-1] + 1)
    on_sheet = interp1d(spec_idxs[advancing], coords[advancing])(frames)
    details = {"dists": dists, "aligned_sheet_idxs": positions, "aligned_sheet_coords": coords,
               "i_inter": frames, "a2s_alignment": on_sheet, "spec_idxs": spec_idxs}
    return dict(zip(frames, on_sheet)), details


def estimate_alignment_error(true_coords, true_onsets, a2s_mapping):
    """pixel error per annotated onset; onsets outside the mapped frame range count as 0 (:180-190)"""
    errors = np.zeros(len(true_onsets))
    for n, onset in enumerate(true_onsets):
        if onset in a2s_mapping:
            errors[n] = true_coords[n] - a2s_mapping[int(onset)]
    return errors


# ---- subsequence DTW: where in a long reference does a short query lie? (include/asr_hip.h: asr_dtw_subseq_batch_dev)

def subseq_dtw_host(dists):
    """The definition of asr_dtw_subseq_batch_dev restated in numpy on a float64 distance matrix (query rows x
    reference columns): A[0][j] = D[0][j], A[i][j] = D[i][j] + fmin(diagonal, fmin(up, left)) with an infinite border;
    end = first minimum of the last row, cost = A[Q-1][end] / Q; traceback by _traceback's rule (argmin over diagonal,
    up, left, the first minimum winning) until row 0 -> (cost, start, end, path), path = (rows, columns) in forward
    order.  The anti-diagonals are evaluated as vectors; every cell is the same sequence of float64 operations in any
    order of evaluation."""
    D = np.ascontiguousarray(dists, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] < 1 or D.shape[1] < 1:
        raise ValueError("subseq_dtw_host expects a (Q, S) matrix with Q, S >= 1")
    Q, S = D.shape
    A = np.full((Q + 1, S + 1), np.inf)                   # A[i + 1][j + 1] = accumulated cost of cell (i, j)
    A[1, 1:] = D[0]
    for d in range(1, Q + S - 1):
        i = np.arange(max(1, d - S + 1), min(d, Q - 1) + 1)
        j = d - i
        A[i + 1, j + 1] = D[i, j] + np.fmin(A[i, j], np.fmin(A[i, j + 1], A[i + 1, j]))
    end = int(np.argmin(A[Q, 1:]))
    cost = A[Q, end + 1] / Q
    i, j = Q - 1, end
    rows, cols = [i], [j]
    while i > 0:
        w = int(np.argmin((A[i, j], A[i, j + 1], A[i + 1, j])))     # diagonal, up (i-1, j), left (i, j-1)
        i -= w != 2
        j -= w != 1
        rows.append(i)
        cols.append(j)
    return float(cost), j, end, (np.array(rows[::-1], np.int64), np.array(cols[::-1], np.int64))


def follow_dtw_host(dists, state=None):
    """The definition of asr_dtw_follow_batch_dev restated in numpy: the rows of the float64 distance matrix `dists`
    (B new query rows x S reference columns) continue state = (acc float64 [S], org int32 [S], rows consumed), or start
    a stream (state None or 0 rows consumed: the first row is the free start).  Every cell carries, beside its
    accumulated cost, the column at which its best path started - the origin of the predecessor _traceback's rule
    picks (diagonal, up, left; strict <) - so per row the first minimum gives (cost, start, pos) without a traceback:
    for every row this is subseq_dtw_host on all rows up to it, whatever the cut into calls.
    -> (cost float64 [B], start int32 [B], pos int32 [B], new state).  Anti-diagonals are evaluated as vectors."""
    D = np.ascontiguousarray(dists, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] < 1 or D.shape[1] < 1:
        raise ValueError("follow_dtw_host expects a (B, S) matrix with B, S >= 1")
    B, S = D.shape
    n0 = 0 if state is None else int(state[2])
    A = np.full((B + 1, S + 1), np.inf)                   # A[i + 1][j + 1]: cell (i, j); row 0 is the carried row
    O = np.zeros((B + 1, S + 1), np.int32)
    if n0 == 0:
        A[1, 1:], O[1, 1:], first = D[0], np.arange(S), 1
    else:
        acc, org = np.asarray(state[0], np.float64), np.asarray(state[1], np.int32)
        if acc.shape != (S,) or org.shape != (S,):
            raise ValueError("follow_dtw_host: the state does not have the reference's length")
        A[0, 1:], O[0, 1:], first = acc, org, 0
    for d in range(first, B + S - 1):
        i = np.arange(max(first, d - S + 1), min(d, B - 1) + 1)
        j = d - i
        dg, up, lf = A[i, j], A[i, j + 1], A[i + 1, j]
        take_up = up < dg
        bst = np.where(take_up, up, dg)
        o = np.where(take_up, O[i, j + 1], O[i, j])
        A[i + 1, j + 1] = D[i, j] + np.fmin(dg, np.fmin(up, lf))
        O[i + 1, j + 1] = np.where(lf < bst, O[i + 1, j], o)
    rows = np.arange(B)
    pos = np.argmin(A[1:, 1:], axis=1)
    cost = A[rows + 1, pos + 1] / (n0 + rows + 1)
    start = O[rows + 1, pos + 1]
    return cost, start.astype(np.int32), pos.astype(np.int32), (A[B, 1:].copy(), O[B, 1:].copy(), n0 + B)


def cosine_dists_host(a, b):
    """float64 cosine distances of float32 code rows in the library's operation order (csrc/dist64.h): two accumulators
    over even / odd elements, summed, an odd tail element last; norms = sqrt of the same sum over squares;
    1 - dot / (|a| |b|) with the quotient clipped to [-1, 1]"""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)

    def sum2(p):
        n = p.shape[-1]
        a0, a1 = np.zeros(p.shape[:-1]), np.zeros(p.shape[:-1])
        for k in range(0, n - 1, 2):
            a0 = a0 + p[..., k]
            a1 = a1 + p[..., k + 1]
        return a0 + a1 + p[..., n - 1] if n & 1 else a0 + a1

    na, nb = np.sqrt(sum2(a * a)), np.sqrt(sum2(b * b))
    dot = np.empty((a.shape[0], b.shape[0]))
    step = max(1, (1 << 22) // max(1, b.size))
    for s0 in range(0, a.shape[0], step):                  # products of float32 values are exact in float64
        dot[s0:s0 + step] = sum2(a[s0:s0 + step, None, :] * b[None, :, :])
    cos = dot / (na[:, None] * nb[None, :])
    cos = np.where(np.abs(cos) > 1.0, np.copysign(1.0, cos), cos)
    return 1.0 - cos


def subseq_positions(path, n_q):
    """pos of asr_dtw_subseq_batch_dev: per query row the smallest reference column the path visits in it (the column
    of the row's first entry in forward order)"""
    rows, cols = np.asarray(path[0]), np.asarray(path[1])
    return cols[first_entries(rows, n_q)].astype(np.int32)


def locate_codes_batch(engine, queries, refs, pairs):
    """Subsequence DTW of pairs = [(query index, reference index)] over lists of (n, d) code arrays in one library
    call -> [(cost, start, end, path_len, pos)] (Engine.dtw_subseq_batch)"""
    return engine.dtw_subseq_batch(queries, refs, pairs)
