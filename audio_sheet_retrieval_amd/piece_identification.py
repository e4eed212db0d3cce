"""Piece identification on top of top-k retrieval - the vote of the reference's server
(audio_sheet_retrieval/audio_sheet_server.py:213-300 detect_score / detect_performance) and its persistent
embedding data base (:496-522 load/save_*_db_file: pickle of [codes, ids, id_to_name, snippets]).

Everything between the long input and the vote result stays on the GPU: window slicing, tower forward, top-k against
the resident data base, vote histogram and selection (csrc/piece_vote_kernels.hip).  SURVEY.md 8f row 1.

The server's default mode, the running vote of AudioSheetServer.run (:83-211), is track_scores / track_score (whole
recordings, batched) and PieceTracker (blocks of new frames): music gate and sliding vote in csrc/track_kernels.hip,
track_score_host the numpy restatement they are tested against.  live_track_scores starts one stage earlier, at blocks of
audio samples (audio_frontend.AudioStream -> PieceTracker).

Where in the score: locate_scores places a finished excerpt (subsequence DTW against the vote's candidates), and
ScoreFollower / follow_scores follow a stream block by block, the same alignment carried from call to call.
"""
from __future__ import annotations

import pickle
from collections import OrderedDict, namedtuple

import numpy as np

#: 2-d float32 arrays that already lie on the device, back to back in one buffer: `buf` a DeviceBuffer, `offsets[i]`
#: the first float of array i, `shapes[i]` its (rows, columns).  Engine-side producers: sheet_utils.umc.load_umc_sheets
#: (return_device=True; unrolled strips) and SpectrogramProcessor.process_many_dev (spectrograms).  Every function
#: here that takes a list of strips or spectrograms takes one of these instead (a plain 3-tuple works too).
DeviceArrays = namedtuple("DeviceArrays", ["buf", "offsets", "shapes"])


def _is_device(inputs):
    return isinstance(inputs, tuple) and len(inputs) == 3 and hasattr(inputs[0], "ptr")


def _to_device(engine, inputs):
    """-> (DeviceArrays, owned): host arrays are concatenated as float32 and uploaded once (owned: free the buffer
    afterwards); a device handle is passed through."""
    if _is_device(inputs):
        buf, offsets, shapes = inputs
        shapes = [tuple(int(v) for v in shp) for shp in shapes]
        if len(offsets) != len(shapes):
            raise ValueError("device handle: %d offsets for %d shapes" % (len(offsets), len(shapes)))
        return DeviceArrays(buf, [int(o) for o in offsets], shapes), False
    arrs = []
    for i, x in enumerate(inputs):
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("input %d: expected a 2-d array, got shape %r" % (i, x.shape))
        arrs.append(x)
    sizes = [a.size for a in arrs]
    offsets = [int(o) for o in np.concatenate([[0], np.cumsum(sizes)[:-1]])] if arrs else []
    flat = np.concatenate([a.ravel() for a in arrs]) if arrs else np.zeros(0, np.float32)
    buf = engine.alloc(max(flat.nbytes, 4)).upload(flat)
    return DeviceArrays(buf, offsets, [a.shape for a in arrs]), True


def _identity_desc(off, rows, T, r0, starts):
    """identity gather of the windows at columns `starts`: out[y, x] = src[off + (r0 + y) * T + start + x]"""
    d = np.zeros((len(starts), 9), np.float64)
    d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4] = off, T, r0, 1.0, rows - 1
    d[:, 5], d[:, 6], d[:, 7] = starts, 1.0, T - 1
    return d


def db_window_plan(shapes, offsets, win_shape, centre_rows):
    """The windows of initialize_sheet_db_from_imges / initialize_audio_db_from_specs (audio_sheet_server.py:403-494)
    for arrays of `shapes` at float `offsets` of one buffer -> (per array its window columns, gather descriptors
    (n, 9), ids (n,) int32).  Columns: np.arange(0, W - w, w // 4) - W - w itself is excluded and an array with
    W <= w has no window; rows: the central win_h of a sheet (centre_rows, :468-469), 0.. of a spectrogram."""
    win_h, win_w = win_shape
    indices, desc, ids = [], [], []
    for i, ((rows, T), off) in enumerate(zip(shapes, offsets)):
        r0 = rows // 2 - win_h // 2 if centre_rows else 0
        if r0 < 0 or r0 + win_h > rows:
            raise ValueError("input %d has %d rows, a window needs %d" % (i, rows, win_h))
        idx = np.arange(0, T - win_w, win_w // 4)
        indices.append(idx)
        desc.append(_identity_desc(off, rows, T, r0, idx))
        ids.append(np.full(len(idx), i, np.int32))
    return (indices, np.concatenate(desc) if desc else np.zeros((0, 9), np.float64),
            np.concatenate(ids) if ids else np.zeros(0, np.int32))


def query_window_plan(shapes, offsets, win_shape, n_samples, centre_rows):
    """window_plan for arrays described by shape and offset only -> (per array its window starts, descriptors)"""
    win_h, win_w = win_shape
    starts, desc = [], []
    for i, ((rows, T), off) in enumerate(zip(shapes, offsets)):
        r0 = rows // 2 - win_h // 2 if centre_rows else 0
        if T < win_w:
            raise ValueError("input %d has %d columns, a window needs %d" % (i, T, win_w))
        if r0 < 0 or r0 + win_h > rows:
            raise ValueError("input %d has %d rows, a window needs %d" % (i, rows, win_h))
        st = np.linspace(start=0, stop=T - win_w, num=n_samples).astype(np.int32)
        starts.append(st)
        desc.append(_identity_desc(off, rows, T, r0, st))
    return starts, (np.concatenate(desc) if desc else np.zeros((0, 9), np.float64))


def embed_windows_dev(engine, view, src_ptr, src_floats, desc, win_shape, d_win, d_codes, chunk, after_chunk=None):
    """cut-and-embed of a window table: per chunk of `chunk` descriptors one gather_windows_dev into d_win and one
    embed_view{1,2}_dev into rows s.. of d_codes; after_chunk(s, m) runs after each chunk (the query path's top-k)."""
    from . import _lib
    win_h, win_w = win_shape
    if (getattr(engine.cfg, "h%d" % view), getattr(engine.cfg, "w%d" % view)) != (win_h, win_w):
        engine.set_input_size(view, win_h, win_w)
    n_win = len(desc)
    for s in range(0, n_win, chunk):
        m = min(chunk, n_win - s)
        engine.gather_windows_dev(src_ptr, src_floats, desc[s:s + m], win_h, win_w, d_win.ptr)
        if view == 2:
            engine.embed_view2_dev(d_win.ptr, m, d_codes.offset(s * 32 * 4))
        else:
            engine.embed_view1_dev(d_win.ptr, _lib.IN_F32_RAW, m, d_codes.offset(s * 32 * 4))
        if after_chunk is not None:
            after_chunk(s, m)


class EmbeddingDB(object):
    """codes (N,32) float32, ids (N,) piece index per code, id_to_name {index: name}, optional snippets -
    the four objects the reference pickles (:498-510), plus the device-resident copies used for retrieval."""

    def __init__(self, engine, codes, ids, id_to_name, snippets=None):
        self.engine = engine
        self.codes = np.ascontiguousarray(codes, dtype=np.float32)
        self.ids = np.ascontiguousarray(ids, dtype=np.int32)
        if self.codes.ndim != 2 or self.codes.shape[1] != 32 or self.ids.shape != (self.codes.shape[0],):
            raise ValueError("codes must be (N,32) and ids (N,), got %r and %r" % (self.codes.shape, self.ids.shape))
        self.id_to_name = dict(id_to_name)
        self.snippets = snippets
        self.n_pieces = int(self.ids.max()) + 1 if self.ids.size else 1
        self._d_codes = engine.alloc(max(self.codes.nbytes, 4)).upload(self.codes)
        self._d_ids = engine.alloc(max(self.ids.nbytes, 4)).upload(self.ids)
        # the server loads its data base once and queries it per frame (:496-522, :530-563): the rows' float64 norms,
        # reciprocal norms and the unit-length copy the filter reads are computed here, once (asr_db_create) - a call
        # used to spend an extra pass over the whole pool on them
        self._handle = engine.db_create(self._d_codes.ptr, self.codes.shape[0], dim=32)
        self._scratch = {}                  # device buffers of the query path, grown on demand, kept between calls

    def scratch(self, name, nbytes):
        """a device buffer of at least nbytes that lives as long as the data base (detect_* run per frame)"""
        buf = self._scratch.get(name)
        if buf is None or buf.nbytes < nbytes:
            if buf is not None:
                buf.free()
            buf = self._scratch[name] = self.engine.alloc(max(int(nbytes), 4))
        return buf

    def topk_dev(self, q_ptr, n_q, k, idx_ptr, dist_ptr):
        self._handle.topk_dev(q_ptr, n_q, k, idx_ptr, dist_ptr)

    def retrieve(self, queries, k):
        """_retrieve_*_ids_for_* (:530-563) for host codes: (idx (Q,k) int32, dist (Q,k) float64)"""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        n = q.shape[0]
        dq = self.scratch("q", q.nbytes).upload(q)
        di, dd = self.scratch("idx", n * k * 4), self.scratch("dist", n * k * 8)
        self.topk_dev(dq.ptr, n, k, di.ptr, dd.ptr)
        return di.download((n, k), np.int32), dd.download((n, k), np.float64)

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self._handle.close()
            self._handle = None
            if getattr(self.engine, "ctx", None):      # (a closed engine took every device buffer with it)
                for b in list(self._scratch.values()) + [self._d_codes, self._d_ids]:
                    b.free()
            self._scratch = {}

    # persistent device buffers: `with EmbeddingDB(...) as db:` or close(); dropping the object releases them too
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            if getattr(self.engine, "ctx", None):      # after the engine closed, its buffers are gone with the context
                self.close()
        except Exception:
            pass

    @classmethod
    def load(cls, engine, path):
        with open(path, "rb") as fp:
            try:
                codes, ids, id_to_name, snippets = pickle.load(fp)
            except UnicodeDecodeError:          # written by the Python-2 reference
                fp.seek(0)
                codes, ids, id_to_name, snippets = pickle.load(fp, encoding="latin1")
        return cls(engine, codes, ids, id_to_name, snippets)

    @classmethod
    def from_pool(cls, engine, pool, view, names=None, max_windows=4096):
        """initialize_sheet_db (view 1, :309-354) / initialize_audio_db (view 2, :356-394) for every piece of `pool` at
        once.  `pool`: an AudioScoreRetrievalPool over all pieces with shuffle=False - its entities are listed piece
        after piece in the order of the reference's per-piece pools, and pool.get_device draws the augmentation numbers
        in the same order (NO_AUGMENT's sheet_scaling [1, 1] still draws one per sample).  The windows are cut on the
        device `max_windows` at a time and embedded with one call per chunk; ids = the entity's piece index,
        id_to_name = {piece index: names[index]} (default: the index), snippets = the empty array the reference keeps
        with keep_snippets=False."""
        if view not in (1, 2):
            raise ValueError("view must be 1 (sheet data base) or 2 (audio data base), got %r" % (view,))
        from . import _lib
        n = int(pool.shape[0])
        win_h, win_w = pool.sheet_dim if view == 1 else pool.spec_dim
        if (getattr(engine.cfg, "h%d" % view), getattr(engine.cfg, "w%d" % view)) != (win_h, win_w):
            engine.set_input_size(view, win_h, win_w)
        chunk = max(1, min(n, int(max_windows)))
        b1 = engine.alloc(chunk * pool.sheet_dim[0] * pool.sheet_dim[1] * 4)
        b2 = engine.alloc(chunk * pool.spec_dim[0] * pool.spec_dim[1] * 4)
        d_codes = engine.alloc(max(n * 32 * 4, 4))
        try:
            for s in range(0, n, chunk):
                _, _, m = pool.get_device(slice(s, min(n, s + chunk)), out=(b1, b2))
                if view == 1:
                    engine.embed_view1_dev(b1.ptr, _lib.IN_F32_RAW, m, d_codes.offset(s * 32 * 4))
                else:
                    engine.embed_view2_dev(b2.ptr, m, d_codes.offset(s * 32 * 4))
            codes = d_codes.download((n, 32), np.float32)
        finally:
            for b in (b1, b2, d_codes):
                b.free()
        n_pieces = len(pool.images)
        if names is not None and len(names) != n_pieces:
            raise ValueError("%d names for %d pieces" % (len(names), n_pieces))
        id_to_name = {i: (names[i] if names is not None else i) for i in range(n_pieces)}
        snippets = np.zeros((0, win_h // 2, win_w // 2), dtype=np.uint8)
        return cls(engine, codes, pool.train_entities[:, 0], id_to_name, snippets)

    @classmethod
    def _from_arrays(cls, engine, names, arrays, view, win_shape, centre_rows, max_windows):
        names = list(names)
        dev, owned = _to_device(engine, arrays)
        try:
            if len(names) != len(dev.shapes):
                raise ValueError("%d names for %d pieces" % (len(names), len(dev.shapes)))
            if max_windows < 1:
                raise ValueError("max_windows must be >= 1")
            _, desc, ids = db_window_plan(dev.shapes, dev.offsets, win_shape, centre_rows)
            n = len(desc)
            codes = np.zeros((0, 32), np.float32)
            if n:
                win_h, win_w = win_shape
                chunk = min(n, int(max_windows))
                d_win = engine.alloc(chunk * win_h * win_w * 4)
                d_codes = engine.alloc(n * 32 * 4)
                try:
                    embed_windows_dev(engine, view, dev.buf.ptr, dev.buf.nbytes // 4, desc, win_shape, d_win, d_codes,
                                      chunk)
                    codes = d_codes.download((n, 32), np.float32)
                finally:
                    d_win.free()
                    d_codes.free()
        finally:
            if owned:
                dev.buf.free()
        snippets = np.zeros((0, win_shape[0] // 2, win_shape[1] // 2), dtype=np.uint8)
        return cls(engine, codes, ids, {i: name for i, name in enumerate(names)}, snippets)

    @classmethod
    def from_images(cls, engine, names, strips, sheet_shape=(160, 200), max_windows=4096):
        """initialize_sheet_db_from_imges (:447-494): the data base of unrolled score strips (0..255 values).  Per piece
        the windows at columns np.arange(0, W - w, w // 4) of the central sheet_shape[0] rows, cut on the device
        max_windows at a time and embedded with one call per chunk; ids = piece index, id_to_name = {index: name},
        empty snippets (keep_snippets=False).  A strip with W <= w has no window and no codes.  `strips`: a list of
        host arrays (uploaded once) or a DeviceArrays handle."""
        return cls._from_arrays(engine, names, strips, 1, tuple(sheet_shape), True, max_windows)

    @classmethod
    def from_specs(cls, engine, names, spectrograms, spec_shape=(92, 42), max_windows=4096):
        """initialize_audio_db_from_specs (:403-445): as from_images for (bins, frames) spectrograms, stride
        spec_shape[1] // 4, rows from 0."""
        return cls._from_arrays(engine, names, spectrograms, 2, tuple(spec_shape), False, max_windows)

    def save(self, path):
        with open(path, "wb") as fp:
            pickle.dump([self.codes, self.ids.astype(np.int64), self.id_to_name, self.snippets], fp, protocol=2)

    def __len__(self):
        return self.codes.shape[0]


def _detect(engine, db, long_input, view, win_shape, r0, top_k, n_candidates, n_samples):
    long_input = np.ascontiguousarray(long_input, dtype=np.float32)
    rows, T = long_input.shape
    win_h, win_w = win_shape
    if T < win_w:
        raise ValueError("input has %d columns, a window needs %d" % (T, win_w))
    starts = np.linspace(start=0, stop=T - win_w, num=n_samples).astype(np.int32)        # :217-218
    # buffers that live with the data base: the reference's server answers one request after the other, and five
    # hipMalloc / hipFree pairs per request cost more than the retrieval itself
    d_src = db.scratch("src", long_input.nbytes).upload(long_input)
    d_win = db.scratch("win", n_samples * win_h * win_w * 4)
    d_codes = db.scratch("codes", n_samples * 32 * 4)
    d_idx = db.scratch("idx", n_samples * n_candidates * 4)
    d_dist = db.scratch("dist", n_samples * n_candidates * 8)
    engine.slice_windows_dev(d_src.ptr, rows, T, r0, win_h, win_w, starts, d_win.ptr)
    if view == 2:
        if (engine.cfg.h2, engine.cfg.w2) != (win_h, win_w):
            engine.set_input_size(2, win_h, win_w)
        engine.embed_view2_dev(d_win.ptr, n_samples, d_codes.ptr)
    else:
        from . import _lib
        engine.embed_view1_dev(d_win.ptr, _lib.IN_F32_RAW, n_samples, d_codes.ptr)
    db.topk_dev(d_codes.ptr, n_samples, n_candidates, d_idx.ptr, d_dist.ptr)
    pieces, counts = engine.piece_vote_dev(d_idx.ptr, n_samples * n_candidates, db._d_ids.ptr, len(db),
                                           db.n_pieces, top_k)
    names = [db.id_to_name[int(p)] for p in pieces]
    votes = counts.astype(np.float64) / counts.sum() if counts.size else counts.astype(np.float64)
    return names, votes, pieces, counts


def detect_score(engine, sheet_db, spectrogram, top_k=1, n_candidates=1, n_samples=100, spec_shape=(92, 42)):
    """detect piece from audio (:213-251): `spectrogram` (bins, frames) float32 -> (piece names, normalised votes)."""
    names, votes, _, _ = _detect(engine, sheet_db, spectrogram, 2, spec_shape, 0, top_k, n_candidates, n_samples)
    return names, votes


def detect_performance(engine, audio_db, sheet, top_k=1, n_candidates=1, n_samples=100, sheet_shape=(160, 200)):
    """detect performance from an unrolled score strip (:253-300): `sheet` (rows, columns) with the reference's 0..255
    value range (model.prepare divides by 255 - folded into the first kernel); the central `sheet_shape[0]` rows are
    used (:269-271)."""
    sheet = np.asarray(sheet)
    r0 = sheet.shape[0] // 2 - sheet_shape[0] // 2
    names, votes, _, _ = _detect(engine, audio_db, sheet, 1, sheet_shape, r0, top_k, n_candidates, n_samples)
    return names, votes


# ---- full evaluation: every test piece as a query (audio_sheet_server.py / sheet_audio_server.py --full_eval) --------
def window_plan(inputs, win_shape, n_samples, centre_rows):
    """-> (sources concatenated (float32, flat), per input its window starts, gather descriptors (n_inputs * n_samples,
    9)).  starts: the reference's np.linspace(0, T - w, n_samples).astype(int) (:217-218, :273-274); rows: 0.. of a
    spectrogram, the central win_h rows of a sheet (centre_rows, :269-271).  Every input is checked before anything
    runs on the device."""
    win_h, win_w = win_shape
    srcs, starts, desc, off = [], [], [], 0
    for i, x in enumerate(inputs):
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("input %d: expected a 2-d array, got shape %r" % (i, x.shape))
        rows, T = x.shape
        r0 = rows // 2 - win_h // 2 if centre_rows else 0
        if T < win_w:
            raise ValueError("input %d has %d columns, a window needs %d" % (i, T, win_w))
        if r0 < 0 or r0 + win_h > rows:
            raise ValueError("input %d has %d rows, a window needs %d" % (i, rows, win_h))
        st = np.linspace(start=0, stop=T - win_w, num=n_samples).astype(np.int32)
        srcs.append(x.ravel())
        starts.append(st)
        desc.append(_identity_desc(off, rows, T, r0, st))
        off += x.size
    flat = np.concatenate(srcs) if srcs else np.zeros(0, np.float32)
    return flat, starts, (np.concatenate(desc) if desc else np.zeros((0, 9), np.float64))


def _detect_batch(engine, db, inputs, view, win_shape, centre_rows, top_k, n_candidates, n_samples, targets,
                  max_windows, with_ids=False):
    on_device = _is_device(inputs)
    if not on_device:
        inputs = list(inputs)
    n_in = len(inputs[2]) if on_device else len(inputs)
    if n_samples < 1 or n_candidates < 1 or top_k < 1 or max_windows < 1:
        raise ValueError("n_samples, n_candidates, top_k and max_windows must be >= 1")
    if targets is not None and len(targets) != n_in:
        raise ValueError("%d targets for %d inputs" % (len(targets), n_in))
    if on_device:
        dev, _ = _to_device(engine, inputs)
        _, desc = query_window_plan(dev.shapes, dev.offsets, win_shape, n_samples, centre_rows)
        d_src, src_floats = None, dev.buf.nbytes // 4
    else:
        flat, _, desc = window_plan(inputs, win_shape, n_samples, centre_rows)
        src_floats = flat.size
    if n_in == 0:
        return ([], np.zeros(0, np.int32), np.zeros(0, np.float64)) if targets is not None else []
    win_h, win_w = win_shape
    n_win = n_in * n_samples
    chunk = min(n_win, int(max_windows))
    if (getattr(engine.cfg, "h%d" % view), getattr(engine.cfg, "w%d" % view)) != (win_h, win_w):
        engine.set_input_size(view, win_h, win_w)
    if not on_device:
        d_src = engine.alloc(flat.nbytes).upload(flat)
    d_win = engine.alloc(chunk * win_h * win_w * 4)
    d_codes = engine.alloc(n_win * 32 * 4)
    d_idx, d_dist = engine.alloc(n_win * n_candidates * 4), engine.alloc(n_win * n_candidates * 8)

    def topk(s, m):
        db.topk_dev(d_codes.offset(s * 32 * 4), m, n_candidates, d_idx.offset(s * n_candidates * 4),
                    d_dist.offset(s * n_candidates * 8))
    try:
        embed_windows_dev(engine, view, dev.buf.ptr if on_device else d_src.ptr, src_floats, desc, win_shape, d_win,
                          d_codes, chunk, after_chunk=topk)
        pieces, counts, n_out, ranks, ratios = engine.piece_vote_batch_dev(
            d_idx.ptr, n_in, n_samples * n_candidates, db._d_ids.ptr, len(db), db.n_pieces, top_k, targets)
    finally:
        for b in (d_src, d_win, d_codes, d_idx, d_dist):
            if b is not None:
                b.free()
    results = []
    for g in range(n_in):
        c = counts[g, :n_out[g]]
        names = [db.id_to_name[int(p)] for p in pieces[g, :n_out[g]]]
        results.append((names, c.astype(np.float64) / c.sum() if c.size else c.astype(np.float64)) +
                       ((pieces[g, :n_out[g]].copy(),) if with_ids else ()))     # (locate_scores: the piece ids too)
    return (results, ranks, ratios) if targets is not None else results


def detect_scores(engine, sheet_db, spectrograms, top_k=1, n_candidates=1, n_samples=100, spec_shape=(92, 42),
                  targets=None, max_windows=4096):
    """detect_score for a list of spectrograms of any lengths: all windows cut on the device in one gather per chunk of
    max_windows, one embedding and one top-k call per chunk, one asr_piece_vote_batch_dev call for all inputs.
    -> [(piece names, normalised votes)] per input, each equal to detect_score's; with targets (one piece id per
    input): (that list, ranks, ratios) of the reference's full-eval rule (see full_eval_rank).  `spectrograms`: a
    list of host arrays or a DeviceArrays handle (SpectrogramProcessor.process_many_dev) - no upload then."""
    return _detect_batch(engine, sheet_db, spectrograms, 2, spec_shape, False, top_k, n_candidates, n_samples, targets,
                         max_windows)


def detect_performances(engine, audio_db, sheets, top_k=1, n_candidates=1, n_samples=100, sheet_shape=(160, 200),
                        targets=None, max_windows=4096):
    """detect_performance for a list of unrolled score strips (central sheet_shape[0] rows), batched as
    detect_scores.  `sheets`: host arrays or a DeviceArrays handle (load_umc_sheets(..., return_device=True))."""
    return _detect_batch(engine, audio_db, sheets, 1, sheet_shape, True, top_k, n_candidates, n_samples, targets,
                         max_windows)


def full_eval_rank(ret_result, ret_votes, target):
    """the reference's rank of one query (audio_sheet_server.py:640-645, sheet_audio_server.py:85-90): position + 1
    of the target among the returned pieces and its normalised vote, else (number returned, 0.0)"""
    ret_result = list(ret_result)
    if target in ret_result:
        i = ret_result.index(target)
        return i + 1, float(ret_votes[i])
    return len(ret_result), 0.0


def rank_summary(ranks):
    """{'<=1', '<=5', '<=10', '>10': (count, fraction)} - what scripts/eval_piece_retrieval.py:66-70 prints per
    retrieval direction"""
    ranks = np.sort(np.asarray(ranks))
    n = len(ranks)
    out = OrderedDict()
    for thr in (1, 5, 10):
        cnt = int(np.sum(ranks <= thr))
        out["<=%d" % thr] = (cnt, cnt / float(n) if n else 0.0)
    cnt = int(np.sum(ranks > 10))
    out[">10"] = (cnt, cnt / float(n) if n else 0.0)
    return out


# ---- the running vote of the live server (audio_sheet_server.py:83-211 AudioSheetServer.run) ------------------------
M_THRESH = 0.5              # :116


class TrackResult(object):
    """The loop's state after every frame of one recording (or of one block of a stream).
    m_prob (T,) float32 and voiced (T,) bool per frame; frames: the indices of the voiced frames; per voiced frame
    pieces / counts (n_voiced, top_k) int32 (piece -1 / count 0 past n_out), n_out (n_voiced,) int32 and history
    (n_voiced,) = len(all_piece_ids) at that frame; idx: the (n_voiced, n_candidates) data-base indices, on request."""

    def __init__(self, m_prob, voiced, frames, pieces, counts, n_out, history, id_to_name, idx=None):
        self.m_prob, self.voiced, self.frames = m_prob, voiced, frames
        self.pieces, self.counts, self.n_out, self.history = pieces, counts, n_out, history
        self.id_to_name, self.idx = id_to_name, idx

    def ranking(self, i):
        """what the server shows at frame i (:167-170): (piece names, float64 probabilities = counts / len(history)) of
        the last voiced frame <= i - an unvoiced frame changes nothing - or None before the first one"""
        k = int(np.searchsorted(self.frames, i, side="right")) - 1
        if k < 0:
            return None
        n = int(self.n_out[k])
        names = [self.id_to_name[int(p)] for p in self.pieces[k, :n]]
        return names, self.counts[k, :n].astype(np.float64) / float(self.history[k])


def _track_check(top_k, n_candidates, running_frames, max_windows=1):
    if running_frames is None or int(running_frames) != running_frames or running_frames < 1:
        raise ValueError("running_frames must be an int >= 1, got %r (the reference raises on None)" % (running_frames,))
    if top_k < 1 or n_candidates < 1 or max_windows < 1:
        raise ValueError("top_k, n_candidates and max_windows must be >= 1")


def _history_lengths(n_before, n_new, n_candidates, running_frames):
    """len(all_piece_ids) (:126-129) at each of n_new voiced frames that follow n_before earlier ones"""
    return np.minimum(n_before + 1 + np.arange(n_new, dtype=np.int64), running_frames) * n_candidates


class RunningLevel(object):
    """The music gate's level from what has been heard so far, for streams whose end nobody has heard: frame i is gated
    with max(floor, the largest column sum of the last `memory` columns up to its own) in place of
    spec.sum(axis=0).max() of the finished spectrogram (_detect_music, :527) - the reference's rule on the columns so
    far.  memory: None (or 0) for every column so far, else a number of columns between the window width and 2^20 - one
    loud bang then does not deafen the gate for the rest of a session.  floor: None, or a level below which the
    divisor does not fall (a quiet room is not music).  Pass it where a level is expected: track_gate_host,
    track_score_host, track_scores, PieceTrackerBank, live_track_scores, live_follow_scores."""
    MAX_MEMORY = 1 << 20

    def __init__(self, memory=None, floor=None):
        if memory is not None:
            if isinstance(memory, bool) or int(memory) != memory or memory < 0 or memory > self.MAX_MEMORY:
                raise ValueError("memory must be None or an int in 0..2^20, got %r" % (memory,))
        if floor is not None and (np.isnan(floor) or floor == np.inf):
            raise ValueError("floor must be None or a number below +inf, got %r" % (floor,))
        self.memory = int(memory) if memory else None
        self.floor = None if floor is None or floor == -np.inf else float(np.float32(floor))

    @property
    def memory_arg(self):
        """the C calls' `memory`: 0 = unbounded"""
        return self.memory or 0

    @property
    def floor_arg(self):
        """the C calls' `floor`: -inf = none"""
        return -np.inf if self.floor is None else self.floor

    def check_width(self, width):
        """a memory shorter than the window would let the mean read columns the level does not cover"""
        if self.memory is not None and self.memory < width:
            raise ValueError("RunningLevel: memory=%d is shorter than the window of %d columns" % (self.memory, width))

    def state_floats(self):
        """floats of carried state per stream (asr_track_stream_gate_running_dev)"""
        return self.memory - 1 if self.memory else 1

    def levels(self, column_sums):
        """the level of every frame from the float32 column sums of the recording so far (max is exact: no order of
        evaluation changes a bit)"""
        c = np.ascontiguousarray(column_sums, dtype=np.float32)
        if self.memory is None:
            m = np.maximum.accumulate(c) if c.size else c.copy()
        else:
            m, span = c.copy(), 1                           # m[i] = max of the last `span` sums up to i
            while span < self.memory:
                step = min(span, self.memory - span)
                m[step:] = np.maximum(m[step:], m[:-step].copy())
                span += step
        return m if self.floor is None else np.maximum(np.float32(self.floor), m)

    def __repr__(self):
        return "RunningLevel(memory=%r, floor=%r)" % (self.memory, self.floor)


_BANK_HINT = ("a RunningLevel keeps its state on the device: use PieceTrackerBank(engine, sheet_db, RunningLevel(...), "
              "n_streams=1) (live_track_scores: batched=True)")


def track_gate_host(spectrogram, width, level=None):
    """the loop's gate, line by line (:92, :110-117, _detect_music :524-528) -> (m_prob (T,) float32, voiced (T,) bool).
    level: stands in for spec.sum(axis=0).max() (a stream does not know it) - a number, or a RunningLevel: then frame i
    takes the maximum over the columns heard so far (its last `memory` ones), np.maximum.accumulate or a sliding
    maximum of spec.sum(axis=0)."""
    spec = np.ascontiguousarray(spectrogram, dtype=np.float32)
    T = spec.shape[1]
    m_probs, voiced = np.zeros(T, np.float32), np.zeros(T, bool)
    running_spec = np.zeros((spec.shape[0], width), dtype=np.float32)
    norms = None
    if isinstance(level, RunningLevel):
        level.check_width(width)
        # c_j: the rows added one after the other, as running_spec.sum(axis=0) adds them below (numpy sums the only
        # column of a (bins, 1) array pairwise instead, hence the column of zeros)
        norms = level.levels(np.hstack((spec, np.zeros((spec.shape[0], 1), np.float32))).sum(axis=0)[:T])
    else:
        norm = spec.sum(axis=0).max() if level is None else np.float32(level)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i_frame in range(T):
            running_spec = np.hstack((running_spec[:, 1::], spec[:, i_frame:i_frame + 1]))
            music_prob = running_spec.sum(axis=0).mean()
            if norms is not None:
                norm = norms[i_frame]
            music_prob /= (norm * 0.15)
            m_prob = np.clip(music_prob, 0.0, 1.0)
            m_probs[i_frame] = m_prob
            voiced[i_frame] = m_prob > M_THRESH and i_frame >= running_spec.shape[1]
    return m_probs, voiced


def track_vote_host(piece_id_rows, top_k, running_frames):
    """the loop's history and vote (:126-138) over the piece ids of the voiced frames, one row of n_candidates ids per
    frame -> (pieces, counts (n, top_k) int32, n_out (n,) int32, history (n,) int64).  np.argsort(counts)[::-1] leaves
    the order of equal counts open; here the larger piece id comes first (asr_piece_vote_dev's rule)."""
    rows = np.asarray(piece_id_rows, dtype=np.int64)
    n, n_candidates = rows.shape
    pieces, counts = np.full((n, top_k), -1, np.int32), np.zeros((n, top_k), np.int32)
    n_out, history = np.zeros(n, np.int32), np.zeros(n, np.int64)
    all_piece_ids = np.zeros(0, dtype=np.int64)
    for k in range(n):
        all_piece_ids = np.concatenate((all_piece_ids, rows[k]))
        first_idx = running_frames * n_candidates
        if all_piece_ids.shape[0] > first_idx:
            all_piece_ids = all_piece_ids[-first_idx:]
        unique, cnt = np.unique(all_piece_ids, return_counts=True)
        order = np.lexsort((unique, cnt))[::-1][:top_k]
        m = len(order)
        pieces[k, :m], counts[k, :m], n_out[k], history[k] = unique[order], cnt[order], m, all_piece_ids.shape[0]
    return pieces, counts, n_out, history


def track_score_host(engine, sheet_db, spectrogram, top_k=5, n_candidates=5, running_frames=100, spec_shape=(92, 42),
                     level=None):
    """AudioSheetServer.run (:83-211) on one spectrogram, restated in numpy - the yardstick of track_scores and
    PieceTracker.  Gate and vote are track_gate_host / track_vote_host; the window of every voiced frame is embedded
    (compute_view_2, :120) and looked up (:123) on its own with the single-query functions.  -> TrackResult with idx."""
    _track_check(top_k, n_candidates, running_frames)
    spec = np.ascontiguousarray(spectrogram, dtype=np.float32)
    win_h, win_w = spec_shape
    if spec.ndim != 2 or spec.shape[0] != win_h:
        raise ValueError("expected a (%d, frames) spectrogram, got shape %r" % (win_h, spec.shape))
    m_prob, voiced = track_gate_host(spec, win_w, level)
    frames = np.flatnonzero(voiced)
    if (engine.cfg.h2, engine.cfg.w2) != (win_h, win_w):
        engine.set_input_size(2, win_h, win_w)
    idx = np.zeros((len(frames), n_candidates), np.int32)
    for k, i in enumerate(frames):
        running_spec = np.ascontiguousarray(spec[:, i - win_w + 1:i + 1])
        spec_code = engine.embed_view2(running_spec[np.newaxis, np.newaxis, :, :])
        idx[k] = sheet_db.retrieve(spec_code, n_candidates)[0][0]
    pieces, counts, n_out, history = track_vote_host(sheet_db.ids[idx].reshape(len(frames), n_candidates), top_k,
                                                     running_frames)
    return TrackResult(m_prob, voiced, frames, pieces, counts, n_out, history, sheet_db.id_to_name, idx)


def _track_lookup(engine, db, src_ptr, src_floats, desc, win_shape, n_candidates, d_win, d_codes, d_idx, d_dist, chunk,
                  row0=0, stages=None):
    """gather, tower 2 and top-k of the windows `desc`, `chunk` at a time; the index rows go to rows row0.. of d_idx"""
    import time
    win_h, win_w = win_shape
    if (engine.cfg.h2, engine.cfg.w2) != (win_h, win_w):
        engine.set_input_size(2, win_h, win_w)

    def timed(name, fn, *args):
        if stages is None:
            return fn(*args)
        t0 = time.perf_counter()
        fn(*args)
        engine.sync()
        stages[name] = stages.get(name, 0.0) + time.perf_counter() - t0
    n_win = len(desc)
    for s in range(0, n_win, chunk):
        m = min(chunk, n_win - s)
        timed("gather", engine.gather_windows_dev, src_ptr, src_floats, desc[s:s + m], win_h, win_w, d_win.ptr)
        timed("embed", engine.embed_view2_dev, d_win.ptr, m, d_codes.ptr)
        timed("topk", db.topk_dev, d_codes.ptr, m, n_candidates, d_idx.offset((row0 + s) * n_candidates * 4), d_dist.ptr)


def track_scores(engine, sheet_db, spectrograms, top_k=5, n_candidates=5, running_frames=100, spec_shape=(92, 42),
                 max_windows=4096, return_idx=False, stages=None, level=None):
    """The running vote of the reference's live server (AudioSheetServer.run, :83-211) over every frame of a list of
    recordings, in one pass: one asr_track_gate_dev call for all frames; the windows of the voiced frames only are cut,
    embedded and looked up max_windows at a time; one asr_track_vote_batch_dev call slides the vote over the last
    running_frames voiced frames of every recording.  -> one TrackResult per recording, equal to track_score_host's.
    `spectrograms`: (spec_shape[0], frames) host arrays or a DeviceArrays handle.  return_idx: keep the top-k index
    table.  stages: a dict that receives the seconds per stage (gate / gather / embed / topk / vote; synchronises
    after every stage).  level: None - every recording's own spec.sum(axis=0).max() - or a RunningLevel: the causal gate
    of a finished recording (one asr_track_gate_running_dev call), what a live session at that rule computes."""
    import time
    _track_check(top_k, n_candidates, running_frames, max_windows)
    if level is not None and not isinstance(level, RunningLevel):
        raise ValueError("level: None or a RunningLevel, got %r" % (level,))
    if level is not None:
        level.check_width(spec_shape[1])
    if n_candidates > len(sheet_db):
        raise ValueError("n_candidates=%d for a data base of %d codes" % (n_candidates, len(sheet_db)))
    win_h, win_w = spec_shape
    if not _is_device(spectrograms):
        spectrograms = [np.ascontiguousarray(x, dtype=np.float32) for x in spectrograms]
        for i, x in enumerate(spectrograms):
            if x.ndim != 2 or x.shape[0] != win_h or x.shape[1] < 1:
                raise ValueError("input %d: expected a (%d, frames >= 1) array, got shape %r" % (i, win_h, x.shape))
    dev, owned = _to_device(engine, spectrograms)
    bufs = []
    try:
        for i, (rows, T) in enumerate(dev.shapes):
            if rows != win_h or T < 1:
                raise ValueError("input %d: expected a (%d, frames >= 1) array, got shape %r" % (i, win_h, (rows, T)))
        if not dev.shapes:
            return []
        src_floats = dev.buf.nbytes // 4
        t0 = time.perf_counter()
        if level is None:
            m_prob, voiced, _ = engine.track_gate_dev(dev.buf.ptr, src_floats, dev.offsets, dev.shapes, win_w)
        else:
            m_prob, voiced, _ = engine.track_gate_running_dev(dev.buf.ptr, src_floats, dev.offsets, dev.shapes, win_w,
                                                              level.memory_arg, level.floor_arg)
        if stages is not None:
            stages["gate"] = stages.get("gate", 0.0) + time.perf_counter() - t0
        first = np.concatenate([[0], np.cumsum([T for _, T in dev.shapes])])
        frames = [np.flatnonzero(voiced[first[r]:first[r + 1]]) for r in range(len(dev.shapes))]
        desc = np.concatenate([_identity_desc(off, rows, T, 0, f - (win_w - 1))
                               for (rows, T), off, f in zip(dev.shapes, dev.offsets, frames)])
        n_win = len(desc)
        count = np.array([len(f) for f in frames], np.int64)
        row_first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
        idx = np.zeros((0, n_candidates), np.int32)
        if n_win:
            chunk = min(n_win, int(max_windows))
            d_win, d_codes = engine.alloc(chunk * win_h * win_w * 4), engine.alloc(chunk * 32 * 4)
            d_idx, d_dist = engine.alloc(n_win * n_candidates * 4), engine.alloc(chunk * n_candidates * 8)
            bufs += [d_win, d_codes, d_idx, d_dist]
            _track_lookup(engine, sheet_db, dev.buf.ptr, src_floats, desc, spec_shape, n_candidates, d_win, d_codes,
                          d_idx, d_dist, chunk, stages=stages)
            t0 = time.perf_counter()
            pieces, counts, n_out = engine.track_vote_batch_dev(d_idx.ptr, n_win, row_first, count, n_candidates,
                                                                running_frames, sheet_db._d_ids.ptr, len(sheet_db),
                                                                sheet_db.n_pieces, top_k)
            if stages is not None:
                stages["vote"] = stages.get("vote", 0.0) + time.perf_counter() - t0
            if return_idx:
                idx = d_idx.download((n_win, n_candidates), np.int32)
        else:
            pieces = counts = np.zeros((0, top_k), np.int32)
            n_out = np.zeros(0, np.int32)
    finally:
        for b in bufs:
            b.free()
        if owned:
            dev.buf.free()
    results = []
    for r in range(len(dev.shapes)):
        a, b = int(row_first[r]), int(row_first[r] + count[r])
        results.append(TrackResult(m_prob[first[r]:first[r + 1]], voiced[first[r]:first[r + 1]], frames[r], pieces[a:b],
                                   counts[a:b], n_out[a:b], _history_lengths(0, b - a, n_candidates, running_frames),
                                   sheet_db.id_to_name, idx[a:b] if return_idx else None))
    return results


def track_score(engine, sheet_db, spectrogram, top_k=5, n_candidates=5, running_frames=100, spec_shape=(92, 42),
                max_windows=4096, return_idx=False, level=None):
    """track_scores for one recording -> its TrackResult"""
    return track_scores(engine, sheet_db, [spectrogram], top_k, n_candidates, running_frames, spec_shape, max_windows,
                        return_idx, level=level)[0]


class PieceTracker(object):
    """The running vote as a streaming session: push(columns) takes a (bins, n >= 1) block of new spectrogram columns
    and returns the TrackResult of these n frames (frames: indices within the block; idx included), equal to the
    matching slice of track_score on the whole recording when `level` is its spec.sum(axis=0).max() - the normaliser of
    _detect_music (:527), which a stream cannot know.  The session carries the last w - 1 columns and the top-k rows of
    its last running_frames - 1 voiced frames from block to block; every block is one gate call, one gather / tower /
    top-k call over its voiced frames and one vote call in which the carried rows only feed the history."""

    def __init__(self, engine, sheet_db, level, top_k=5, n_candidates=5, running_frames=100, spec_shape=(92, 42)):
        _track_check(top_k, n_candidates, running_frames)
        if isinstance(level, RunningLevel):
            raise ValueError("PieceTracker: " + _BANK_HINT)
        if n_candidates > len(sheet_db):
            raise ValueError("n_candidates=%d for a data base of %d codes" % (n_candidates, len(sheet_db)))
        self.engine, self.db, self.level = engine, sheet_db, np.float32(level)
        self.top_k, self.n_candidates, self.running_frames = int(top_k), int(n_candidates), int(running_frames)
        self.spec_shape = tuple(spec_shape)
        self.n_frames = 0                                   # frames pushed so far
        self.n_voiced = 0                                   # voiced frames so far
        self._tail = np.zeros((spec_shape[0], spec_shape[1] - 1), np.float32)          # running_spec[:, 1:] (:92)
        self._rows = np.zeros((0, self.n_candidates), np.int32)

    def push(self, columns):
        cols = np.ascontiguousarray(columns, dtype=np.float32)
        win_h, win_w = self.spec_shape
        if cols.ndim != 2 or cols.shape[0] != win_h or cols.shape[1] < 1:
            raise ValueError("expected a (%d, n >= 1) block of columns, got shape %r" % (win_h, cols.shape))
        n, C = cols.shape[1], self.n_candidates
        block = np.ascontiguousarray(np.hstack((self._tail, cols)))
        eng, db = self.engine, self.db
        d_src = db.scratch("track_src", block.nbytes).upload(block)
        m_prob, voiced, _ = eng.track_gate_dev(d_src.ptr, block.size, [0], [block.shape], win_w, norm=[self.level],
                                               frame0=[self.n_frames - (win_w - 1)])
        m_prob, voiced = m_prob[win_w - 1:], voiced[win_w - 1:]
        frames = np.flatnonzero(voiced)                     # window of block frame j: block columns j .. j + w - 1
        h, m = len(self._rows), len(frames)
        pieces = counts = np.zeros((0, self.top_k), np.int32)
        n_out, new_rows = np.zeros(0, np.int32), np.zeros((0, C), np.int32)
        if m:
            d_win, d_codes = db.scratch("track_win", m * win_h * win_w * 4), db.scratch("track_codes", m * 32 * 4)
            d_idx, d_dist = db.scratch("track_idx", (h + m) * C * 4), db.scratch("track_dist", m * C * 8)
            if h:
                d_idx.upload(self._rows)
            _track_lookup(eng, db, d_src.ptr, block.size, _identity_desc(0, win_h, block.shape[1], 0, frames),
                          self.spec_shape, C, d_win, d_codes, d_idx, d_dist, m, row0=h)
            pieces, counts, n_out = eng.track_vote_batch_dev(d_idx.ptr, h + m, [0], [h + m], C, self.running_frames,
                                                             db._d_ids.ptr, len(db), db.n_pieces, self.top_k,
                                                             emit_from=[h])
            new_rows = d_idx.download((h + m, C), np.int32)[h:]
            keep = self.running_frames - 1
            self._rows = np.concatenate((self._rows, new_rows))[max(0, h + m - keep):] if keep else new_rows[:0]
        history = _history_lengths(self.n_voiced, m, C, self.running_frames)
        self._tail = np.ascontiguousarray(block[:, block.shape[1] - (win_w - 1):])
        self.n_frames += n
        self.n_voiced += m
        return TrackResult(m_prob, voiced, frames, pieces, counts, n_out, history, db.id_to_name, new_rows)


class PieceTrackerBank(object):
    """PieceTracker for len(levels) parallel streams in one object, with every stream's state on the device: the last
    w - 1 columns of all streams in one buffer and the top-k rows of their last running_frames - 1 voiced frames in
    another (a ring per stream), both updated in place by the two calls of csrc/track_stream_kernels.hip.
    push(columns) takes one (bins, n_i >= 0) block per stream - host arrays, or the DeviceArrays handle of
    AudioStream.push_dev, which it does not free - and returns one TrackResult per stream, equal field for field to
    what a PieceTracker of that stream returns for the block (an empty result where n_i == 0).  One round is one
    asr_track_stream_gate_dev call, one tower and one top-k call over the voiced windows of all streams, one
    asr_track_stream_vote_dev call and one download of the new index rows, whatever the number of streams; a round of
    more than max_windows new frames is cut along the frames into several, which changes no result.  The work buffers
    (windows, codes, index rows, distances) are allocated once and grown when a larger round arrives.
    `levels` may be one RunningLevel for all streams, with n_streams=N: no level is known beforehand, every frame is
    gated at the level of what its stream has brought so far (asr_track_stream_gate_running_dev), the carried column
    sums are a third device buffer, and the results per stream equal track_scores(..., level=that RunningLevel) on the
    stream's columns."""

    def __init__(self, engine, sheet_db, levels, top_k=5, n_candidates=5, running_frames=100, spec_shape=(92, 42),
                 max_windows=4096, n_streams=None):
        _track_check(top_k, n_candidates, running_frames, max_windows)
        if n_candidates > len(sheet_db):
            raise ValueError("n_candidates=%d for a data base of %d codes" % (n_candidates, len(sheet_db)))
        self.running = levels if isinstance(levels, RunningLevel) else None
        if self.running is not None:
            if n_streams is None or int(n_streams) != n_streams or n_streams < 1:
                raise ValueError("a RunningLevel needs n_streams=<number of streams, at least one>, got %r" % (n_streams,))
            self.running.check_width(spec_shape[1])
            self.levels = None
            self.n_streams = int(n_streams)
        else:
            if n_streams is not None:
                raise ValueError("n_streams goes with a RunningLevel; given levels, there is one stream per level")
            self.levels = np.ascontiguousarray(levels, dtype=np.float32)
            if self.levels.ndim != 1 or self.levels.size < 1:
                raise ValueError("levels: expected one gate level per stream (at least one), got shape %r" %
                                 (self.levels.shape,))
            self.n_streams = int(self.levels.size)
        self.engine, self.db = engine, sheet_db
        self.top_k, self.n_candidates, self.running_frames = int(top_k), int(n_candidates), int(running_frames)
        self.spec_shape, self.max_windows = tuple(spec_shape), int(max_windows)
        self.n_frames = [0] * self.n_streams                # frames pushed so far, per stream
        self.n_voiced = [0] * self.n_streams                # voiced frames so far, per stream
        win_h, win_w = self.spec_shape
        tail, ring = win_h * (win_w - 1), (self.running_frames - 1) * self.n_candidates
        self._tail_off = np.arange(self.n_streams, dtype=np.int64) * tail
        self._hist_off = np.arange(self.n_streams, dtype=np.int64) * ring
        self._tail_floats, self._hist_len = self.n_streams * tail, self.n_streams * ring
        self._d_tail = engine.alloc(max(4, self._tail_floats * 4))                      # running_spec[:, 1:] (:92) per stream
        self._d_hist = engine.alloc(self._hist_len * 4) if ring else None
        self._d_level = None
        if self.running is not None:                        # the carried column sums (or the one maximum) per stream
            per = self.running.state_floats()
            self._level_off = np.arange(self.n_streams, dtype=np.int64) * per
            self._level_floats = self.n_streams * per
            self._d_level = engine.alloc(self._level_floats * 4)
        self._work = {}
        #: a dict here receives the seconds per stage (gate / embed / topk / vote / rows; synchronises after every stage)
        self.stages = None

    def _buffer(self, name, nbytes):
        """the work buffer `name`, grown when a larger round arrives"""
        buf = self._work.get(name)
        if buf is None or buf.nbytes < nbytes:
            if buf is not None:
                buf.free()
            buf = self._work[name] = self.engine.alloc(max(4, int(nbytes)))
        return buf

    def _round(self, cols_ptr, cols_floats, col_off, n_new):
        """one round of (bins, n_new[s]) blocks at float col_off[s] of the device buffer -> one TrackResult per stream"""
        import time
        eng, db, C = self.engine, self.db, self.n_candidates
        win_h, win_w = self.spec_shape
        total = int(sum(n_new))
        d_win = self._buffer("win", total * win_h * win_w * 4)

        def timed(name, fn, *args):
            if self.stages is None:
                return fn(*args)
            t0 = time.perf_counter()
            out = fn(*args)
            eng.sync()
            self.stages[name] = self.stages.get(name, 0.0) + time.perf_counter() - t0
            return out
        if self.running is None:
            m_prob, voiced, n_voiced = timed("gate", eng.track_stream_gate_dev, cols_ptr, cols_floats, col_off, n_new,
                                             self.n_frames, self.levels, win_h, win_w, self._d_tail.ptr,
                                             self._tail_floats, self._tail_off, d_win.ptr, total)
        else:
            m_prob, voiced, n_voiced, _ = timed(
                "gate", eng.track_stream_gate_running_dev, cols_ptr, cols_floats, col_off, n_new, self.n_frames,
                self.running.memory_arg, self.running.floor_arg, win_h, win_w, self._d_tail.ptr, self._tail_floats,
                self._tail_off, self._d_level.ptr, self._level_floats, self._level_off, d_win.ptr, total)
        m = int(n_voiced.sum())
        pieces = counts = np.zeros((0, self.top_k), np.int32)
        n_out, idx = np.zeros(0, np.int32), np.zeros((0, C), np.int32)
        if m:
            d_codes, d_idx = self._buffer("codes", m * 32 * 4), self._buffer("idx", m * C * 4)
            d_dist = self._buffer("dist", m * C * 8)
            if (eng.cfg.h2, eng.cfg.w2) != (win_h, win_w):
                eng.set_input_size(2, win_h, win_w)
            timed("embed", eng.embed_view2_dev, d_win.ptr, m, d_codes.ptr)
            timed("topk", db.topk_dev, d_codes.ptr, m, C, d_idx.ptr, d_dist.ptr)
            pieces, counts, n_out = timed(
                "vote", eng.track_stream_vote_dev, d_idx.ptr, m, n_voiced, self.n_voiced, C, self.running_frames,
                db._d_ids.ptr, len(db), db.n_pieces, self.top_k, self._d_hist.ptr if self._d_hist is not None else None,
                self._hist_len, self._hist_off)
            idx = timed("rows", d_idx.download, (m, C), np.int32)
        results, f0, r0 = [], 0, 0
        for s in range(self.n_streams):
            f1, r1 = f0 + int(n_new[s]), r0 + int(n_voiced[s])
            history = _history_lengths(self.n_voiced[s], r1 - r0, C, self.running_frames)
            results.append(TrackResult(m_prob[f0:f1], voiced[f0:f1], np.flatnonzero(voiced[f0:f1]), pieces[r0:r1],
                                       counts[r0:r1], n_out[r0:r1], history, db.id_to_name, idx[r0:r1]))
            self.n_frames[s] += f1 - f0
            self.n_voiced[s] += r1 - r0
            f0, r0 = f1, r1
        return results

    def push(self, columns):
        if self._d_tail is None:
            raise ValueError("the PieceTrackerBank is closed")
        win_h, win_w = self.spec_shape
        if _is_device(columns):
            buf, offsets, shapes = columns
            offsets, shapes = [int(o) for o in offsets], [tuple(int(v) for v in shp) for shp in shapes]
            if len(offsets) != len(shapes):
                raise ValueError("device handle: %d offsets for %d shapes" % (len(offsets), len(shapes)))
        else:
            cols = [np.ascontiguousarray(c, dtype=np.float32) for c in columns]
            shapes = [c.shape for c in cols]
        if len(shapes) != self.n_streams:
            raise ValueError("%d blocks for %d streams" % (len(shapes), self.n_streams))
        for s, shp in enumerate(shapes):
            if len(shp) != 2 or shp[0] != win_h:
                raise ValueError("stream %d: expected a (%d, n >= 0) block of columns, got shape %r" % (s, win_h, shp))
        n_new = [int(shp[1]) for shp in shapes]
        total = sum(n_new)
        if not _is_device(columns):
            offsets = [int(o) for o in np.concatenate([[0], np.cumsum([c.size for c in cols])[:-1]])]
            buf = self._buffer("cols", total * win_h * 4)
            if total:
                buf.upload(np.concatenate([c.ravel() for c in cols]))
        src_floats = buf.nbytes // 4
        if total <= self.max_windows:
            return self._round(buf.ptr, src_floats, offsets, n_new)
        # cut along the frames: every round takes the next columns of each stream, max_windows in all; a column range of
        # a row-major block is not one, so the gather call repacks it
        parts, done = [[] for _ in shapes], [0] * self.n_streams
        d_cut = self._buffer("cut", self.max_windows * win_h * 4)
        while sum(done) < total:
            room, take = self.max_windows, []
            for s in range(self.n_streams):
                take.append(min(n_new[s] - done[s], room))
                room -= take[-1]
            cut_off = [int(o) for o in np.concatenate([[0], np.cumsum(take)[:-1]]) * win_h]
            for s in range(self.n_streams):
                if take[s]:
                    self.engine.gather_windows_dev(buf.ptr, src_floats,
                                                   _identity_desc(offsets[s], win_h, n_new[s], 0, [done[s]]), win_h, take[s],
                                                   d_cut.offset(cut_off[s] * 4))
                    done[s] += take[s]
            for s, r in enumerate(self._round(d_cut.ptr, d_cut.nbytes // 4, cut_off, take)):
                if take[s]:
                    parts[s].append(r)
        return [_concat_track_results(p, self.db.id_to_name, self.top_k, self.n_candidates) for p in parts]

    def reset(self, streams=None):
        """`streams` (default: all) start over: the next push is the first of a new recording.  Only the counters are
        zeroed - the calls do not read the state of a stream without frames."""
        which = range(self.n_streams) if streams is None else [int(s) for s in streams]
        for s in which:
            if not 0 <= s < self.n_streams:
                raise ValueError("stream %d of %d" % (s, self.n_streams))
        for s in which:
            self.n_frames[s], self.n_voiced[s] = 0, 0

    def close(self):
        for buf in [self._d_tail, self._d_hist, self._d_level] + list(self._work.values()):
            if buf is not None:
                buf.free()
        self._d_tail = self._d_hist = self._d_level = None
        self._work = {}


def _concat_track_results(parts, id_to_name, top_k, n_candidates):
    """the TrackResults of consecutive blocks of one recording as one (frames: indices within the recording)"""
    if not parts:
        z = np.zeros((0, top_k), np.int32)
        return TrackResult(np.zeros(0, np.float32), np.zeros(0, bool), np.zeros(0, np.int64), z, z, np.zeros(0, np.int32),
                           np.zeros(0, np.int64), id_to_name, np.zeros((0, n_candidates), np.int32))
    first = np.concatenate([[0], np.cumsum([len(r.m_prob) for r in parts])])
    cat = lambda name: np.concatenate([getattr(r, name) for r in parts])
    return TrackResult(cat("m_prob"), cat("voiced"), np.concatenate([r.frames + first[i] for i, r in enumerate(parts)]),
                       cat("pieces"), cat("counts"), cat("n_out"), cat("history"), id_to_name, cat("idx"))


def live_track_scores(engine, sheet_db, processor, recordings, sample_rates, block_samples, levels=None, top_k=5,
                      n_candidates=5, running_frames=100, spec_shape=(92, 42), integer=None, window_scales=None,
                      batched=False, dft=None):
    """The live server from the samples on: every recording (mono samples at sample_rates[i]) is cut into blocks of
    block_samples input samples (an int, or one per recording) and pushed block by block through an
    audio_frontend.AudioStream - all recordings of one (rate, integer, window scale) group as parallel streams of one
    object, one launch per round of blocks - and each stream's new columns go to its own PieceTracker.  A recording
    that ends is flushed.  -> one TrackResult per recording, the fields of its blocks concatenated (frames: indices
    within the recording; idx included); equal to track_scores on processor.process_many(recordings, ...) at the same
    levels.  levels: per recording the normaliser of the music gate; None takes spec.sum(axis=0).max() of the finished
    spectrogram, as track_scores does - which means computing that spectrogram first: a real stream cannot, and must be
    given a level - or a RunningLevel, with batched=True: then no spectrogram is computed beforehand, every frame is gated
    at the level of what its stream has brought so far, and the results equal track_scores(..., level=that RunningLevel)
    on process_many's spectrograms.  batched=True: the columns of a group stay on the device (AudioStream.push_dev / flush_dev) and one
    PieceTrackerBank takes the place of the group's trackers - the same results, a fixed number of calls per round.
    dft: AudioStream's argument, for either branch - None for a dft="direct" processor, "fft" for a dft="fft" processor,
    whose streams compute the FFT and whose results equal track_scores on that processor's process_many."""
    from .audio_frontend import AudioStream
    running = levels if isinstance(levels, RunningLevel) else None
    if running is not None and not batched:
        raise ValueError("live_track_scores(batched=False): " + _BANK_HINT)
    recs = [np.ascontiguousarray(r, dtype=np.float32).ravel() for r in recordings]
    n = len(recs)
    rates = list(sample_rates)
    flags = [False] * n if integer is None else [bool(f) for f in integer]
    scales = [processor.window_scale] * n if window_scales is None else [float(w) for w in window_scales]
    steps = [int(block_samples)] * n if np.ndim(block_samples) == 0 else [int(b) for b in block_samples]
    if not (len(rates) == len(flags) == len(scales) == len(steps) == n):
        raise ValueError("%d recordings: %d sample rates, %d integer flags, %d window scales, %d block lengths" %
                         (n, len(rates), len(flags), len(scales), len(steps)))
    if any(b < 1 for b in steps):
        raise ValueError("block_samples must be >= 1")
    if levels is None:
        levels = [spec.sum(axis=0).max() if spec.shape[1] else 0.0
                  for spec in processor.process_many(recs, scales, rates, flags)]
    if running is None and len(levels) != n:
        raise ValueError("%d levels for %d recordings" % (len(levels), n))
    parts = [[] for _ in recs]
    for key in sorted(set(zip(rates, flags, scales))):
        sel = [i for i in range(n) if (rates[i], flags[i], scales[i]) == key]
        bank, trackers = None, []
        if running is not None:
            bank = PieceTrackerBank(engine, sheet_db, running, top_k, n_candidates, running_frames, spec_shape,
                                    n_streams=len(sel))
        elif batched:
            bank = PieceTrackerBank(engine, sheet_db, [levels[i] for i in sel], top_k, n_candidates, running_frames,
                                    spec_shape)
        else:
            trackers = [PieceTracker(engine, sheet_db, levels[i], top_k, n_candidates, running_frames, spec_shape)
                        for i in sel]
        stream = AudioStream(processor, len(sel), key[0], key[1], key[2], dft)

        def track_dev(handle):
            try:
                for k, r in enumerate(bank.push(handle)):
                    if len(r.m_prob):
                        parts[sel[k]].append(r)
            finally:
                handle.buf.free()
        try:
            pos = [0] * len(sel)
            while not all(stream.flushed):
                blocks = []
                for k, i in enumerate(sel):
                    blocks.append(recs[i][pos[k]:pos[k] + steps[i]])
                    pos[k] += blocks[-1].size
                if batched:
                    track_dev(stream.push_dev(blocks))
                    ended = [k for k, i in enumerate(sel) if pos[k] >= recs[i].size and not stream.flushed[k]]
                    if ended:
                        track_dev(stream.flush_dev(ended))
                    continue
                results = [stream.push(blocks)]
                ended = [k for k, i in enumerate(sel) if pos[k] >= recs[i].size and not stream.flushed[k]]
                if ended:
                    results.append(stream.flush(ended))
                for columns in results:
                    for k, i in enumerate(sel):
                        if columns[k].shape[1]:
                            parts[i].append(trackers[k].push(columns[k]))
        finally:
            stream.close()
            if bank is not None:
                bank.close()
    return [_concat_track_results(p, sheet_db.id_to_name, top_k, n_candidates) for p in parts]


# ---- where in the score is an excerpt?  piece vote, then subsequence DTW against the candidates' ordered codes ----------
def piece_segments(ids):
    """{piece id: (first data-base row, number of rows)} of a data base whose `ids` list every piece's rows
    contiguously (EmbeddingDB.from_images / from_pool do); ValueError otherwise"""
    ids = np.asarray(ids).reshape(-1)
    segs = {}
    if ids.size == 0:
        return segs
    cuts = np.flatnonzero(np.diff(ids) != 0) + 1
    for first, stop in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [ids.size]])):
        piece = int(ids[first])
        if piece in segs:
            raise ValueError("the data-base rows of piece %d are not contiguous (rows %d.. and %d..): pass `segments`"
                             % (piece, segs[piece][0], first))
        segs[piece] = (int(first), int(stop - first))
    return segs


def default_sheet_columns(ids, w_sheet):
    """strip x-coordinate of every data-base row by EmbeddingDB.from_images' rule: window k of a piece starts at
    k * (w_sheet // 4), so its centre is at k * (w_sheet // 4) + w_sheet // 2"""
    ids = np.asarray(ids).reshape(-1)
    cols = np.zeros(ids.size, np.float64)
    for first, n in piece_segments(ids).values():
        cols[first:first + n] = np.arange(n) * (w_sheet // 4) + w_sheet // 2
    return cols


def locate_window_plan(shapes, offsets, win_shape, step_spec):
    """the query windows of locate_scores: per excerpt the columns np.arange(0, T - w + 1, step_spec), rows 0.. ->
    (per excerpt its window starts, gather descriptors)"""
    win_h, win_w = win_shape
    if step_spec < 1:
        raise ValueError("step_spec must be >= 1")
    starts, desc = [], []
    for i, ((rows, T), off) in enumerate(zip(shapes, offsets)):
        if T < win_w:
            raise ValueError("input %d has %d columns, a window needs %d" % (i, T, win_w))
        if win_h > rows:
            raise ValueError("input %d has %d rows, a window needs %d" % (i, rows, win_h))
        st = np.arange(0, T - win_w + 1, step_spec)
        if len(st) > 1024:
            raise ValueError("input %d gives %d windows; the subsequence DTW takes queries of at most 1024 (raise "
                             "step_spec or cut the excerpt)" % (i, len(st)))
        starts.append(st)
        desc.append(_identity_desc(off, rows, T, 0, st))
    return starts, (np.concatenate(desc) if desc else np.zeros((0, 9), np.float64))


def _score_tables(engine, sheet_db, segments, sheet_columns):
    """the checked (segments, sheet_columns) of locate_scores and the follow routes, with their defaults"""
    segments = piece_segments(sheet_db.ids) if segments is None else {int(k): (int(v[0]), int(v[1]))
                                                                      for k, v in dict(segments).items()}
    for piece, (first, n) in segments.items():
        if first < 0 or n < 1 or first + n > len(sheet_db):
            raise ValueError("segment of piece %d (rows %d..%d) leaves the %d rows of the data base"
                             % (piece, first, first + n, len(sheet_db)))
    if sheet_columns is None:
        sheet_columns = default_sheet_columns(sheet_db.ids, int(engine.cfg.w1))
    sheet_columns = np.asarray(sheet_columns, np.float64).reshape(-1)
    if sheet_columns.size != len(sheet_db):
        raise ValueError("%d sheet_columns for %d data-base rows" % (sheet_columns.size, len(sheet_db)))
    return segments, sheet_columns


def _locate(engine, sheet_db, spectrograms, n_pieces, step_spec, n_candidates, n_samples, spec_shape, segments,
            sheet_columns, max_windows, host):
    segments, sheet_columns = _score_tables(engine, sheet_db, segments, sheet_columns)
    dev, owned = _to_device(engine, spectrograms if _is_device(spectrograms) else list(spectrograms))
    try:
        n_in = len(dev.shapes)
        if n_in == 0:
            return []
        votes = _detect_batch(engine, sheet_db, dev, 2, spec_shape, False, n_pieces, n_candidates, n_samples, None,
                              max_windows, with_ids=True)
        starts, desc = locate_window_plan(dev.shapes, dev.offsets, spec_shape, step_spec)
        n_q = np.array([len(st) for st in starts], np.int64)
        q_at = np.concatenate([[0], np.cumsum(n_q)])
        n_win = int(n_q.sum())
        pairs = []                                           # (excerpt, candidate, piece)
        for e, (_, _, pieces) in enumerate(votes):
            for c, piece in enumerate(pieces):
                if int(piece) not in segments:
                    raise ValueError("piece %d got votes but has no segment" % int(piece))
                pairs.append((e, c, int(piece)))
        chunk = max(1, min(n_win, int(max_windows)))
        d_win = engine.alloc(chunk * spec_shape[0] * spec_shape[1] * 4)
        d_codes = engine.alloc(max(n_win * 32 * 4, 4))
        try:
            embed_windows_dev(engine, 2, dev.buf.ptr, dev.buf.nbytes // 4, desc, spec_shape, d_win, d_codes, chunk)
            if host:
                from . import alignment
                codes = d_codes.download((n_win, 32), np.float32)
                res = []
                for e, _, piece in pairs:
                    first, n = segments[piece]
                    d = alignment.cosine_dists_host(codes[q_at[e]:q_at[e + 1]], sheet_db.codes[first:first + n])
                    cost, start, end, path = alignment.subseq_dtw_host(d)
                    res.append((cost, start, end, alignment.subseq_positions(path, int(n_q[e]))))
            elif pairs:
                cost, start, end, _, pos = engine.dtw_subseq_batch_dev(
                    d_codes.ptr, n_win, sheet_db._d_codes.ptr, len(sheet_db), [q_at[e] for e, _, _ in pairs],
                    [n_q[e] for e, _, _ in pairs], [segments[p][0] for _, _, p in pairs],
                    [segments[p][1] for _, _, p in pairs], 32)
                res = [(float(cost[k]), int(start[k]), int(end[k]), pos[k]) for k in range(len(pairs))]
            else:
                res = []
        finally:
            d_win.free()
            d_codes.free()
    finally:
        if owned:
            dev.buf.free()
    out = [[] for _ in range(n_in)]
    for (e, c, piece), (cost, start, end, pos) in zip(pairs, res):
        first = segments[piece][0]
        names, share, _ = votes[e]
        out[e].append(dict(name=names[c], votes=float(share[c]), vote_rank=c + 1, cost=float(cost), start_row=int(start), end_row=int(end),
                           start_x=float(sheet_columns[first + start]), end_x=float(sheet_columns[first + end]),
                           x=sheet_columns[first + np.asarray(pos, np.int64)]))
    return [sorted(cands, key=lambda cand: cand["cost"]) for cands in out]     # stable: equal costs keep the vote's order


def locate_scores(engine, sheet_db, spectrograms, n_pieces=5, step_spec=2, n_candidates=25, n_samples=100,
                  spec_shape=(92, 42), segments=None, sheet_columns=None, max_windows=4096):
    """Where in which score does each excerpt lie?  The piece vote (detect_scores, top_k = n_pieces) names the
    candidates; every excerpt's windows at columns np.arange(0, T - w + 1, step_spec) are cut and embedded on the
    device, and one asr_dtw_subseq_batch_dev call aligns every excerpt with the ordered codes of each of its candidates
    inside the resident data base (free start and end on the score axis, the excerpt consumed completely).
    segments: {piece id: (first data-base row, rows)}, by default derived from sheet_db.ids, which must list every
    piece's rows contiguously (ValueError otherwise).  sheet_columns: the strip x-coordinate of every data-base row;
    by default EmbeddingDB.from_images' rule, window k of a piece at k * (w_sheet // 4) + w_sheet // 2.
    -> per excerpt its candidates ordered by alignment cost (equal costs keep the vote's order), each a dict of name,
    votes (normalised), vote_rank (1 = most votes), cost, start_row / end_row (rows of the piece's segment), start_x / end_x and x (one strip
    coordinate per query window).  `spectrograms`: host arrays or a DeviceArrays handle.  An excerpt gives at most 1024
    windows."""
    return _locate(engine, sheet_db, spectrograms, n_pieces, step_spec, n_candidates, n_samples, tuple(spec_shape),
                   segments, sheet_columns, max_windows, host=False)


def locate_score(engine, sheet_db, spectrogram, n_pieces=5, step_spec=2, n_candidates=25, n_samples=100,
                 spec_shape=(92, 42), segments=None, sheet_columns=None):
    """locate_scores for one spectrogram -> its candidates"""
    return locate_scores(engine, sheet_db, [spectrogram], n_pieces, step_spec, n_candidates, n_samples, spec_shape,
                         segments, sheet_columns)[0]


def locate_scores_host(engine, sheet_db, spectrograms, n_pieces=5, step_spec=2, n_candidates=25, n_samples=100,
                       spec_shape=(92, 42), segments=None, sheet_columns=None, max_windows=4096):
    """locate_scores with the alignment on the host: the same vote and window codes, downloaded, and per pair
    alignment.subseq_dtw_host on alignment.cosine_dists_host - what the device path is tested against"""
    return _locate(engine, sheet_db, spectrograms, n_pieces, step_spec, n_candidates, n_samples, tuple(spec_shape),
                   segments, sheet_columns, max_windows, host=True)


# ---- where in the score is the music now?  the subsequence DTW carried from block to block (asr_dtw_follow_batch_dev) ----
class FollowResult(object):
    """Score following per query window: frames (n,) the first stream column of each window; per window and candidate
    (n, candidates): cost (float64), row / start_row (rows of the piece's segment where the best path so far ends /
    started), x / start_x (their strip coordinates); best (n,) the candidate of least cost, the earlier one on equal
    costs.  pieces: the candidates' piece ids, names: their names."""

    def __init__(self, frames, cost, row, start_row, x, start_x, pieces, names):
        self.frames, self.cost, self.row, self.start_row, self.x, self.start_x = frames, cost, row, start_row, x, start_x
        self.best = np.argmin(cost, axis=1).astype(np.int64) if cost.shape[1] else np.zeros(len(frames), np.int64)
        self.pieces, self.names = list(pieces), list(names)


def follow_window_plan(n_before, n_new, win_w, step_spec):
    """The bookkeeping of a followed stream, whose windows are those at stream columns k * step_spec whatever the
    block cut: after n_before columns, a block of n_new more completes the windows -> (their stream columns, the
    stream column from which the session carries on: the next unfinished window's start, or the stream's end when
    that start lies further on)"""
    if step_spec < 1 or win_w < 1 or n_before < 0 or n_new < 0:
        raise ValueError("step_spec and win_w must be >= 1, the column counts >= 0")
    done = lambda T: 0 if T < win_w else (T - win_w) // step_spec + 1
    k0, k1, T = done(n_before), done(n_before + n_new), n_before + n_new
    return np.arange(k0, k1, dtype=np.int64) * step_spec, min(k1 * step_spec, T)


def _follow_candidates(sheet_db, pieces, segments):
    """piece ids of a candidate list of ids or names, each with a segment"""
    by_name = {v: k for k, v in sheet_db.id_to_name.items()}
    out = []
    for piece in pieces:
        piece = by_name[piece] if isinstance(piece, str) and piece in by_name else piece
        if isinstance(piece, str) or int(piece) not in segments:
            raise ValueError("candidate %r is no piece of the data base with a segment" % (piece,))
        out.append(int(piece))
    return out


def _follow_result(sheet_db, segments, sheet_columns, pieces, frames, per_cand):
    """FollowResult of per candidate (cost, start, pos) over the windows at `frames`"""
    n = len(frames)
    cost = np.zeros((n, len(pieces)), np.float64)
    row, start_row = np.zeros((n, len(pieces)), np.int32), np.zeros((n, len(pieces)), np.int32)
    x, start_x = np.zeros((n, len(pieces)), np.float64), np.zeros((n, len(pieces)), np.float64)
    for c, (piece, (cst, start, pos)) in enumerate(zip(pieces, per_cand)):
        first = segments[piece][0]
        cost[:, c], row[:, c], start_row[:, c] = cst, pos, start
        x[:, c] = sheet_columns[first + np.asarray(pos, np.int64)]
        start_x[:, c] = sheet_columns[first + np.asarray(start, np.int64)]
    return FollowResult(np.asarray(frames, np.int64), cost, row, start_row, x, start_x, pieces,
                        [sheet_db.id_to_name[p] for p in pieces])


FOLLOW_MAX_ROWS = 1024      # query rows of one pair of one asr_dtw_follow_batch_dev call


class ScoreFollower(object):
    """Score following as a streaming session, the companion of PieceTracker: push(columns) takes a (bins, n >= 1)
    block of new spectrogram columns and returns the FollowResult of the windows this block completes - the windows at
    stream columns k * step_spec, whatever the block cut - against every candidate piece (`pieces`: ids or names, for
    example PieceTracker's current leaders or detect_scores' top few).  Per window and candidate it is what
    locate_scores' alignment gives for the stream so far (subsequence DTW, free start and end on the score axis), but
    a block costs its own rows only: the session keeps, per candidate, the last accumulated row and the path origins
    in two device buffers (asr_dtw_follow_batch_dev's state; never downloaded in push) and the spectrogram columns from
    the next unfinished window's start on.  Every block is one gather and one tower call over its windows and one
    follow call for all candidates (one per 1024 windows).  segments, sheet_columns: as in locate_scores.  close()
    frees the state."""

    def __init__(self, engine, sheet_db, pieces, step_spec=2, spec_shape=(92, 42), segments=None, sheet_columns=None):
        if step_spec < 1 or int(step_spec) != step_spec:
            raise ValueError("step_spec must be an int >= 1")
        self.engine, self.db, self.step_spec, self.spec_shape = engine, sheet_db, int(step_spec), tuple(spec_shape)
        self.segments, self.sheet_columns = _score_tables(engine, sheet_db, segments, sheet_columns)
        self.pieces = _follow_candidates(sheet_db, pieces, self.segments)
        self._r_row = np.array([self.segments[p][0] for p in self.pieces], np.int64)
        self._n_r = np.array([self.segments[p][1] for p in self.pieces], np.int64)
        self._state_off = np.concatenate([[0], np.cumsum(self._n_r)]).astype(np.int64)
        self._state_len = int(self._state_off[-1])
        self._d_acc = engine.alloc(max(self._state_len * 8, 8))
        self._d_org = engine.alloc(max(self._state_len * 4, 4))
        self.n_columns = 0                                  # stream columns pushed so far
        self.n_windows = 0                                  # windows followed so far
        self._col0 = 0                                      # stream column of the first carried column
        self._carry = np.zeros((self.spec_shape[0], 0), np.float32)

    def close(self):
        for b in (self._d_acc, self._d_org):
            if b is not None:
                b.free()
        self._d_acc = self._d_org = None

    def state(self):
        """the downloaded state per candidate: (acc, org, windows followed) - for tests and checkpoints"""
        acc = self._d_acc.download((self._state_len,), np.float64)
        org = self._d_org.download((self._state_len,), np.int32)
        at = self._state_off
        return [(acc[at[c]:at[c + 1]], org[at[c]:at[c + 1]], self.n_windows) for c in range(len(self.pieces))]

    def push(self, columns):
        cols = np.ascontiguousarray(columns, dtype=np.float32)
        win_h, win_w = self.spec_shape
        if cols.ndim != 2 or cols.shape[0] != win_h or cols.shape[1] < 1:
            raise ValueError("expected a (%d, n >= 1) block of columns, got shape %r" % (win_h, cols.shape))
        if self._d_acc is None:
            raise ValueError("the session is closed")
        eng, db, C = self.engine, self.db, len(self.pieces)
        starts, carry_from = follow_window_plan(self.n_columns, cols.shape[1], win_w, self.step_spec)
        block = np.ascontiguousarray(np.hstack((self._carry, cols)))
        m = len(starts)
        per_cand = [(np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32))] * C
        if m and C:
            d_src = db.scratch("follow_src", block.nbytes).upload(block)
            d_win, d_codes = db.scratch("follow_win", m * win_h * win_w * 4), db.scratch("follow_codes", m * 32 * 4)
            embed_windows_dev(eng, 2, d_src.ptr, block.size, _identity_desc(0, win_h, block.shape[1], 0, starts - self._col0),
                              self.spec_shape, d_win, d_codes, m)
            parts = []
            for c0 in range(0, m, FOLLOW_MAX_ROWS):
                mm = min(FOLLOW_MAX_ROWS, m - c0)
                parts.append(eng.dtw_follow_batch_dev(d_codes.ptr, m, db._d_codes.ptr, len(db), [c0] * C, [mm] * C,
                                                      self._r_row, self._n_r, [self.n_windows + c0] * C, 32,
                                                      self._d_acc.ptr, self._d_org.ptr, self._state_len,
                                                      self._state_off[:-1]))
            per_cand = [tuple(np.concatenate([part[c][k] for part in parts]) for k in range(3)) for c in range(C)]
        self.n_columns += cols.shape[1]
        self._carry = np.ascontiguousarray(block[:, carry_from - self._col0:])
        self._col0 = carry_from
        self.n_windows += m
        return _follow_result(db, self.segments, self.sheet_columns, self.pieces, starts, per_cand)


def _follow(engine, sheet_db, spectrograms, pieces, step_spec, spec_shape, segments, sheet_columns, max_windows, host):
    segments, sheet_columns = _score_tables(engine, sheet_db, segments, sheet_columns)
    if step_spec < 1:
        raise ValueError("step_spec must be >= 1")
    win_h, win_w = spec_shape
    dev, owned = _to_device(engine, spectrograms if _is_device(spectrograms) else list(spectrograms))
    try:
        n_in = len(dev.shapes)
        cands = [_follow_candidates(sheet_db, p, segments) for p in pieces]
        if len(cands) != n_in:
            raise ValueError("%d candidate lists for %d recordings" % (len(cands), n_in))
        if n_in == 0:
            return []
        starts, desc = [], []
        for i, ((rows, T), off) in enumerate(zip(dev.shapes, dev.offsets)):
            if rows != win_h:
                raise ValueError("input %d: expected a (%d, frames) array, got shape %r" % (i, win_h, (rows, T)))
            st = follow_window_plan(0, T, win_w, step_spec)[0]
            starts.append(st)
            desc.append(_identity_desc(off, rows, T, 0, st))
        desc = np.concatenate(desc)
        n_q = np.array([len(st) for st in starts], np.int64)
        q_at = np.concatenate([[0], np.cumsum(n_q)])
        n_win = int(n_q.sum())
        pairs = [(e, piece) for e in range(n_in) for piece in cands[e]]
        res = [[] for _ in pairs]
        bufs = []
        try:
            if n_win and pairs:
                chunk = max(1, min(n_win, int(max_windows)))
                d_win = engine.alloc(chunk * win_h * win_w * 4)
                d_codes = engine.alloc(n_win * 32 * 4)
                bufs += [d_win, d_codes]
                embed_windows_dev(engine, 2, dev.buf.ptr, dev.buf.nbytes // 4, desc, spec_shape, d_win, d_codes, chunk)
                if host:
                    from . import alignment
                    codes = d_codes.download((n_win, 32), np.float32)
                    for k, (e, piece) in enumerate(pairs):
                        if n_q[e]:
                            first, n = segments[piece]
                            d = alignment.cosine_dists_host(codes[q_at[e]:q_at[e + 1]], sheet_db.codes[first:first + n])
                            res[k].append(alignment.follow_dtw_host(d)[:3])
                else:
                    n_r = np.array([segments[p][1] for _, p in pairs], np.int64)
                    r_row = np.array([segments[p][0] for _, p in pairs], np.int64)
                    q_of = np.array([e for e, _ in pairs], np.int64)
                    s_off = np.concatenate([[0], np.cumsum(n_r)]).astype(np.int64)
                    d_acc, d_org = engine.alloc(int(s_off[-1]) * 8), engine.alloc(int(s_off[-1]) * 4)
                    bufs += [d_acc, d_org]
                    for c0 in range(0, int(n_q.max()), FOLLOW_MAX_ROWS):
                        live = np.flatnonzero(n_q[q_of] > c0)
                        out = engine.dtw_follow_batch_dev(
                            d_codes.ptr, n_win, sheet_db._d_codes.ptr, len(sheet_db), q_at[q_of[live]] + c0,
                            np.minimum(n_q[q_of[live]] - c0, FOLLOW_MAX_ROWS), r_row[live], n_r[live],
                            np.full(len(live), c0, np.int64), 32, d_acc.ptr, d_org.ptr, int(s_off[-1]), s_off[:-1][live])
                        for k, item in zip(live, out):
                            res[k].append(item)
        finally:
            for b in bufs:
                b.free()
    finally:
        if owned:
            dev.buf.free()
    empty = (np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32))
    results, k = [], 0
    for e in range(n_in):
        per_cand = []
        for _ in cands[e]:
            per_cand.append(tuple(np.concatenate([part[j] for part in res[k]]) for j in range(3)) if res[k] else empty)
            k += 1
        results.append(_follow_result(sheet_db, segments, sheet_columns, cands[e], starts[e], per_cand))
    return results


def follow_scores(engine, sheet_db, spectrograms, pieces, step_spec=2, spec_shape=(92, 42), segments=None,
                  sheet_columns=None, max_windows=4096):
    """Score following over whole recordings of any length: `pieces` is one candidate list (ids or names) per
    recording.  One embedding pass over all windows (columns np.arange(0, T - w + 1, step_spec) of every recording),
    then ceil(max windows / 1024) asr_dtw_follow_batch_dev calls over all recordings x candidates.  -> one FollowResult
    per recording, equal to what a ScoreFollower returns over any block cut of it.  A recording shorter than a window
    gives an empty result."""
    return _follow(engine, sheet_db, spectrograms, pieces, step_spec, tuple(spec_shape), segments, sheet_columns,
                   max_windows, host=False)


def follow_scores_host(engine, sheet_db, spectrograms, pieces, step_spec=2, spec_shape=(92, 42), segments=None,
                       sheet_columns=None, max_windows=4096):
    """follow_scores with the alignment on the host: the same window codes, downloaded, and per pair
    alignment.follow_dtw_host on alignment.cosine_dists_host - what the device path is tested against"""
    return _follow(engine, sheet_db, spectrograms, pieces, step_spec, tuple(spec_shape), segments, sheet_columns,
                   max_windows, host=True)


# ---- where in which score are many live streams now?  ScoreFollower for parallel streams, candidates from the vote ------
def follow_slot_plan(slots, wanted, segments=None):
    """The candidate policy of ScoreFollowerBank, a pure function: `slots` holds per slot a piece id or None, `wanted`
    the pieces a stream is to be followed against (at most len(slots), no piece twice; with `segments` each must have
    one).  A piece already in a slot keeps its slot (and its state); a slot whose piece is not wanted is freed; the
    remaining wanted pieces, in the given order, take the free slots in ascending slot index; an empty `wanted` leaves
    the slots as they are.  -> (the new slots, the indices of the newly taken ones)"""
    slots = [None if p is None else int(p) for p in slots]
    wanted = [int(p) for p in wanted]
    if len(set(wanted)) != len(wanted):
        raise ValueError("a piece is wanted twice: %r" % (wanted,))
    if len(wanted) > len(slots):
        raise ValueError("%d pieces wanted for %d slots" % (len(wanted), len(slots)))
    if segments is not None:
        for piece in wanted:
            if piece not in segments:
                raise ValueError("candidate %r is no piece of the data base with a segment" % (piece,))
    if not wanted:
        return slots, []
    new = [p if p in wanted else None for p in slots]
    free = [k for k, p in enumerate(new) if p is None]
    taken = []
    for piece in wanted:
        if piece not in new:
            k = free.pop(0)
            new[k] = piece
            taken.append(k)
    return new, taken


class BankFollowResult(object):
    """Score following of one stream of a ScoreFollowerBank per query window: frames (n,) the first stream column of each
    window; per window and slot (n, n_slots): piece (int32, -1: the slot is empty), cost (float64, +inf for an empty
    slot) - the accumulated cost divided by the windows followed since `since`, so slots that entered at different
    times compare -, row / start_row (int32, rows of the piece's segment where the best path so far ends / started; -1
    for an empty slot), x / start_x (their strip coordinates; NaN for an empty slot), since (int64, the stream's window
    index from which the slot follows its piece; -1 for an empty slot); best (n,) the occupied slot of least cost, the
    lower slot on equal costs, -1 where no slot is occupied.  names: {piece id: name}."""

    def __init__(self, frames, piece, cost, row, start_row, x, start_x, since, names=None, best=None):
        self.frames, self.piece, self.cost, self.row, self.start_row = frames, piece, cost, row, start_row
        self.x, self.start_x, self.since, self.names = x, start_x, since, names
        if best is not None:                                # a slice of a larger result's
            self.best = best
            return
        occupied = piece >= 0
        least = np.argmin(np.where(occupied, cost, np.inf), axis=1) if piece.shape[0] else np.zeros(0, np.int64)
        self.best = np.where(occupied.any(axis=1), least, -1).astype(np.int64)


def _bank_follow_result(frames, n_slots, names):
    """a BankFollowResult of len(frames) windows with every slot empty"""
    n = len(frames)
    return BankFollowResult(np.asarray(frames, np.int64), np.full((n, n_slots), -1, np.int32), np.full((n, n_slots), np.inf),
                            np.full((n, n_slots), -1, np.int32), np.full((n, n_slots), -1, np.int32),
                            np.full((n, n_slots), np.nan), np.full((n, n_slots), np.nan), np.full((n, n_slots), -1, np.int64),
                            names)


def _fill_bank_slot(res, k, piece, since, cost, start, pos, first, sheet_columns):
    """slot k of `res` <- one piece's (cost, start, pos) over all its windows"""
    res.piece[:, k], res.since[:, k], res.cost[:, k], res.row[:, k], res.start_row[:, k] = piece, since, cost, pos, start
    res.x[:, k] = sheet_columns[first + np.asarray(pos, np.int64)]
    res.start_x[:, k] = sheet_columns[first + np.asarray(start, np.int64)]


def _concat_bank_results(parts, n_slots, names):
    """the BankFollowResults of consecutive rounds of one stream as one"""
    if not parts:
        return _bank_follow_result(np.zeros(0, np.int64), n_slots, names)
    cat = lambda name: np.concatenate([getattr(r, name) for r in parts])
    return BankFollowResult(cat("frames"), cat("piece"), cat("cost"), cat("row"), cat("start_row"), cat("x"), cat("start_x"),
                            cat("since"), names)


def follow_bank_host(codes_per_stream, window_counts_per_round, candidate_schedule, db_codes, segments, n_slots=5,
                     catch_up=64, sheet_columns=None, step_spec=2):
    """ScoreFollowerBank restated in numpy.  codes_per_stream: per stream the (windows, dim) codes of all its windows;
    window_counts_per_round: per round the windows every stream completes in it; candidate_schedule:
    {round: {stream: pieces}}, the wishes recorded (set_candidates) before that round's push.  Slots follow
    follow_slot_plan; a newly taken slot enters at the first round in which its stream completes a window, from
    min(windows so far, catch_up) windows back (`since`); per slot occupancy the values are alignment.follow_dtw_host
    on alignment.cosine_dists_host of the stream's window codes from `since` on against db_codes[segment], the
    catch-up rows' outputs dropped.  -> (one BankFollowResult per stream over all rounds, frames = window index *
    step_spec; per stream and slot None or (piece, since, pending, follow_dtw_host's state or None))"""
    from . import alignment
    n_streams = len(codes_per_stream)
    db_codes = np.asarray(db_codes, np.float32)
    if sheet_columns is None:
        sheet_columns = np.zeros(len(db_codes), np.float64)
    sheet_columns = np.asarray(sheet_columns, np.float64)
    slots = [[None] * n_slots for _ in range(n_streams)]
    info = [[None] * n_slots for _ in range(n_streams)]      # per occupied slot [since, pending, state]
    done = [0] * n_streams
    parts = [[] for _ in range(n_streams)]
    for rnd, counts in enumerate(window_counts_per_round):
        if len(counts) != n_streams:
            raise ValueError("round %d: %d window counts for %d streams" % (rnd, len(counts), n_streams))
        for s, wanted in dict(candidate_schedule.get(rnd, {})).items():
            new, taken = follow_slot_plan(slots[s], wanted, segments)
            for k in range(n_slots):
                if new[k] is None:
                    info[s][k] = None
                elif k in taken:
                    info[s][k] = [-1, True, None]
            slots[s] = new
        for s in range(n_streams):
            m, W = int(counts[s]), done[s]
            if m == 0:
                continue
            if W + m > len(codes_per_stream[s]):
                raise ValueError("stream %d: %d windows scheduled, %d codes" % (s, W + m, len(codes_per_stream[s])))
            res = _bank_follow_result(np.arange(W, W + m, dtype=np.int64) * step_spec, n_slots, None)
            K = min(W, int(catch_up))
            for k, piece in enumerate(slots[s]):
                if piece is None:
                    continue
                first, n = segments[piece]
                if info[s][k][1]:
                    info[s][k] = [W - K, False, None]
                    q0, drop = W - K, K
                else:
                    q0, drop = W, 0
                d = alignment.cosine_dists_host(codes_per_stream[s][q0:W + m], db_codes[first:first + n])
                cost, start, pos, info[s][k][2] = alignment.follow_dtw_host(d, info[s][k][2])
                _fill_bank_slot(res, k, piece, info[s][k][0], cost[drop:], start[drop:], pos[drop:], first, sheet_columns)
            parts[s].append(BankFollowResult(res.frames, res.piece, res.cost, res.row, res.start_row, res.x, res.start_x,
                                             res.since, None))
            done[s] = W + m
    state = [[None if slots[s][k] is None else (slots[s][k],) + tuple(info[s][k]) for k in range(n_slots)]
             for s in range(n_streams)]
    return [_concat_bank_results(p, n_slots, None) for p in parts], state


class ScoreFollowerBank(object):
    """ScoreFollower for n_streams parallel streams in one object whose candidates may change while the streams run,
    with every stream's state on the device: the last w - 1 columns of all streams in one buffer, the codes of their
    last windows in another (a linear log per stream of catch_up + the per-round row limit rows, the query buffer of
    the follow call) and per (stream, slot) an accumulated row and its path origins sized for the longest segment of
    the data base.  set_candidates(stream, pieces) names the pieces a stream is followed against (for example
    PieceTrackerBank's current leaders); follow_slot_plan assigns them to the stream's n_slots slots at the next push.
    A newly taken slot is pending and enters at the first round in which its stream completes a window, catch_up
    windows back (fewer when the stream is younger): the stream's window index `since`.  push(columns) takes one
    (bins, n_i >= 0) block per stream - host arrays, or the DeviceArrays handle of AudioStream.push_dev, which it does
    not free - and returns one BankFollowResult per stream for the windows the block completes (those at stream
    columns k * step_spec, whatever the block cut).  Per window i an occupied slot's values are what
    asr_dtw_subseq_batch_dev gives for the stream's windows since .. i against the slot's piece, the cost divided by
    i - since + 1.  One round is one asr_follow_stream_windows_dev call, one tower call over the windows of all
    streams, one asr_follow_stream_log_dev call and one asr_dtw_follow_batch_dev call over all occupied (stream, slot)
    pairs with the download that call makes, whatever the number of streams; a stream without an occupied slot still
    has its windows embedded and logged.  A round takes at most 1024 - catch_up columns per stream (the follow call's
    limit of 1024 query rows) and max_windows columns in all; a larger push is cut along the columns into several
    rounds, which changes no result.  The work buffers are allocated once and grown when a larger round arrives."""

    def __init__(self, engine, sheet_db, n_streams, n_slots=5, step_spec=2, spec_shape=(92, 42), catch_up=64,
                 segments=None, sheet_columns=None, max_windows=4096):
        if step_spec < 1 or int(step_spec) != step_spec:
            raise ValueError("step_spec must be an int >= 1")
        if n_streams < 1 or n_slots < 1 or max_windows < 1:
            raise ValueError("n_streams, n_slots and max_windows must be >= 1")
        if catch_up < 0 or catch_up > FOLLOW_MAX_ROWS // 2 or int(catch_up) != catch_up:
            raise ValueError("catch_up must be an int in 0..%d" % (FOLLOW_MAX_ROWS // 2))
        self.engine, self.db, self.n_streams, self.n_slots = engine, sheet_db, int(n_streams), int(n_slots)
        self.step_spec, self.spec_shape, self.catch_up = int(step_spec), tuple(spec_shape), int(catch_up)
        self.max_windows = int(max_windows)
        self.round_rows = FOLLOW_MAX_ROWS - self.catch_up    # columns (so at most that many windows) per stream and round
        self.segments, self.sheet_columns = _score_tables(engine, sheet_db, segments, sheet_columns)
        if not self.segments:
            raise ValueError("the data base has no piece with a segment")
        self.dim = int(np.asarray(sheet_db.codes).shape[1])
        win_h, win_w = self.spec_shape
        tail, self._log_rows = win_h * (win_w - 1), FOLLOW_MAX_ROWS
        self._seg_max = max(n for _, n in self.segments.values())
        self._tail_off = np.arange(self.n_streams, dtype=np.int64) * tail
        self._log_off = np.arange(self.n_streams, dtype=np.int64) * (self._log_rows * self.dim)
        self._tail_floats, self._log_floats = self.n_streams * tail, self.n_streams * self._log_rows * self.dim
        self._state_len = self.n_streams * self.n_slots * self._seg_max
        self._d_tail = engine.alloc(max(4, self._tail_floats * 4))
        self._d_log = engine.alloc(self._log_floats * 4)
        self._d_acc, self._d_org = engine.alloc(self._state_len * 8), engine.alloc(self._state_len * 4)
        self._work = {}
        #: a dict here receives the seconds per stage (windows / embed / log / follow; synchronises after every stage)
        self.stages = None
        self.reset()

    def reset(self, streams=None):
        """`streams` (default: all) start over: the next push is the first of a new recording, with every slot empty
        and no wish recorded.  Only the host's counters are zeroed - the calls do not read the state of a new stream."""
        which = range(self.n_streams) if streams is None else [int(s) for s in streams]
        for s in which:
            if not 0 <= s < self.n_streams:
                raise ValueError("stream %d of %d" % (s, self.n_streams))
        if streams is None:
            self.n_columns, self.n_windows = [0] * self.n_streams, [0] * self.n_streams
            self._in_log = [0] * self.n_streams             # valid rows at the front of the stream's log
            self._slots = [[None] * self.n_slots for _ in range(self.n_streams)]
            self._since = [[-1] * self.n_slots for _ in range(self.n_streams)]
            self._pending = [[False] * self.n_slots for _ in range(self.n_streams)]
            self._wish = [None] * self.n_streams
        for s in which:
            self.n_columns[s] = self.n_windows[s] = self._in_log[s] = 0
            self._slots[s], self._since[s] = [None] * self.n_slots, [-1] * self.n_slots
            self._pending[s], self._wish[s] = [False] * self.n_slots, None

    def close(self):
        for buf in [self._d_tail, self._d_log, self._d_acc, self._d_org] + list(self._work.values()):
            if buf is not None:
                buf.free()
        self._d_tail = self._d_log = self._d_acc = self._d_org = None
        self._work = {}

    def set_candidates(self, stream, pieces):
        """stream `stream` is to be followed against `pieces` (ids or names, at most n_slots, each with a segment) from
        its next push on; only the last wish before a push counts, and an empty list leaves the slots as they are"""
        stream = int(stream)
        if not 0 <= stream < self.n_streams:
            raise ValueError("stream %d of %d" % (stream, self.n_streams))
        wanted = _follow_candidates(self.db, pieces, self.segments)
        follow_slot_plan(self._slots[stream], wanted, self.segments)          # refuses what the push would refuse
        self._wish[stream] = wanted

    def slots(self, stream):
        """per slot of `stream` the piece id or None, the recorded wish applied"""
        wish = self._wish[int(stream)]
        return follow_slot_plan(self._slots[int(stream)], wish)[0] if wish else list(self._slots[int(stream)])

    def _state_off(self, s, k):
        return (s * self.n_slots + k) * self._seg_max

    def state(self):
        """downloaded, for tests and checkpoints: per stream and slot None (empty) or (piece, since, pending, (acc, org,
        rows consumed) or None while pending); a recorded wish is not applied before the next push"""
        acc = self._d_acc.download((self._state_len,), np.float64)
        org = self._d_org.download((self._state_len,), np.int32)
        out = []
        for s in range(self.n_streams):
            row = []
            for k, piece in enumerate(self._slots[s]):
                if piece is None:
                    row.append(None)
                elif self._pending[s][k]:
                    row.append((piece, -1, True, None))
                else:
                    o, n = self._state_off(s, k), self.segments[piece][1]
                    row.append((piece, self._since[s][k], False,
                                (acc[o:o + n].copy(), org[o:o + n].copy(), self.n_windows[s] - self._since[s][k])))
            out.append(row)
        return out

    _buffer = PieceTrackerBank._buffer

    def _apply_wishes(self):
        for s, wanted in enumerate(self._wish):
            if wanted:
                new, taken = follow_slot_plan(self._slots[s], wanted, self.segments)
                for k in range(self.n_slots):
                    if new[k] is None or k in taken:
                        self._since[s][k], self._pending[s][k] = -1, new[k] is not None
                self._slots[s] = new
            self._wish[s] = None

    def _round(self, cols_ptr, cols_floats, col_off, n_new):
        """one round of (bins, n_new[s]) blocks at float col_off[s] of the device buffer -> one BankFollowResult per
        stream"""
        import time
        eng, db, dim = self.engine, self.db, self.dim
        win_h, win_w = self.spec_shape
        starts = [follow_window_plan(self.n_columns[s], int(n_new[s]), win_w, self.step_spec)[0]
                  for s in range(self.n_streams)]
        m = np.array([len(st) for st in starts], np.int32)
        total = int(m.sum())
        d_win = self._buffer("win", total * win_h * win_w * 4)

        def timed(name, fn, *args):
            if self.stages is None:
                return fn(*args)
            t0 = time.perf_counter()
            out = fn(*args)
            eng.sync()
            self.stages[name] = self.stages.get(name, 0.0) + time.perf_counter() - t0
            return out
        n_win = timed("windows", eng.follow_stream_windows_dev, cols_ptr, cols_floats, col_off, n_new, self.n_columns,
                      win_h, win_w, self.step_spec, self._d_tail.ptr, self._tail_floats, self._tail_off, d_win.ptr, total)
        if not np.array_equal(n_win, m):
            raise RuntimeError("the windows call completed %r windows, the plan %r" % (n_win.tolist(), m.tolist()))
        # one result over the windows of all streams, filled pair by pair and cut into the streams' at the end
        res = _bank_follow_result(np.concatenate(starts), self.n_slots, db.id_to_name)
        w_at = np.concatenate([[0], np.cumsum(m)])
        if total:
            d_codes = self._buffer("codes", total * dim * 4)
            if (eng.cfg.h2, eng.cfg.w2) != (win_h, win_w):
                eng.set_input_size(2, win_h, win_w)
            timed("embed", eng.embed_view2_dev, d_win.ptr, total, d_codes.ptr)
            kept = np.minimum(self._in_log, self.catch_up)
            in_log = timed("log", eng.follow_stream_log_dev, d_codes.ptr, total, m, self._in_log, self.catch_up, dim,
                           self._d_log.ptr, self._log_floats, self._log_off)
            pairs, q_row, n_q, before = [], [], [], []       # pairs: (stream, slot, catch-up rows whose outputs are dropped)
            for s in range(self.n_streams):
                if not m[s]:
                    continue
                K, W = int(kept[s]), self.n_windows[s]
                for k, piece in enumerate(self._slots[s]):
                    if piece is None:
                        continue
                    if self._pending[s][k]:                  # enters: from K windows back, a fresh state
                        self._since[s][k], self._pending[s][k] = W - K, False
                        pairs.append((s, k, K)), q_row.append(s * self._log_rows), n_q.append(K + int(m[s])), before.append(0)
                    else:
                        pairs.append((s, k, 0)), q_row.append(s * self._log_rows + K), n_q.append(int(m[s]))
                        before.append(W - self._since[s][k])
            if pairs:
                seg = [self.segments[self._slots[s][k]] for s, k, _ in pairs]
                out = timed("follow", eng.dtw_follow_batch_dev, self._d_log.ptr, self.n_streams * self._log_rows,
                            db._d_codes.ptr, len(db), q_row, n_q, [f for f, _ in seg], [n for _, n in seg], before, dim,
                            self._d_acc.ptr, self._d_org.ptr, self._state_len, [self._state_off(s, k) for s, k, _ in pairs])
                first = np.zeros((total, self.n_slots), np.int64)
                for (s, k, drop), (f, _), (cost, start, pos) in zip(pairs, seg, out):
                    a, b = w_at[s], w_at[s + 1]
                    res.piece[a:b, k], res.since[a:b, k], first[a:b, k] = self._slots[s][k], self._since[s][k], f
                    res.cost[a:b, k], res.row[a:b, k], res.start_row[a:b, k] = cost[drop:], pos[drop:], start[drop:]
                occupied = res.piece >= 0
                res.x = np.where(occupied, self.sheet_columns[first + np.maximum(res.row, 0)], np.nan)
                res.start_x = np.where(occupied, self.sheet_columns[first + np.maximum(res.start_row, 0)], np.nan)
            self._in_log = [int(v) for v in in_log]
        for s in range(self.n_streams):
            self.n_columns[s] += int(n_new[s])
            self.n_windows[s] += int(m[s])
        res = BankFollowResult(res.frames, res.piece, res.cost, res.row, res.start_row, res.x, res.start_x, res.since)
        cut = lambda x, s: x[w_at[s]:w_at[s + 1]]
        return [BankFollowResult(cut(res.frames, s), cut(res.piece, s), cut(res.cost, s), cut(res.row, s), cut(res.start_row, s),
                                 cut(res.x, s), cut(res.start_x, s), cut(res.since, s), db.id_to_name, cut(res.best, s))
                for s in range(self.n_streams)]

    def push(self, columns):
        if self._d_tail is None:
            raise ValueError("the ScoreFollowerBank is closed")
        win_h, win_w = self.spec_shape
        if _is_device(columns):
            buf, offsets, shapes = columns
            offsets, shapes = [int(o) for o in offsets], [tuple(int(v) for v in shp) for shp in shapes]
            if len(offsets) != len(shapes):
                raise ValueError("device handle: %d offsets for %d shapes" % (len(offsets), len(shapes)))
        else:
            cols = [np.ascontiguousarray(c, dtype=np.float32) for c in columns]
            shapes = [c.shape for c in cols]
        if len(shapes) != self.n_streams:
            raise ValueError("%d blocks for %d streams" % (len(shapes), self.n_streams))
        for s, shp in enumerate(shapes):
            if len(shp) != 2 or shp[0] != win_h:
                raise ValueError("stream %d: expected a (%d, n >= 0) block of columns, got shape %r" % (s, win_h, shp))
        n_new = [int(shp[1]) for shp in shapes]
        total = sum(n_new)
        if not _is_device(columns):
            offsets = [int(o) for o in np.concatenate([[0], np.cumsum([c.size for c in cols])[:-1]])]
            buf = self._buffer("cols", total * win_h * 4)
            if total:
                buf.upload(np.concatenate([c.ravel() for c in cols]))
        self._apply_wishes()
        src_floats = buf.nbytes // 4
        if total <= self.max_windows and max(n_new) <= self.round_rows:
            return self._round(buf.ptr, src_floats, offsets, n_new)
        # cut along the columns: every round takes the next columns of each stream, round_rows of one and max_windows in
        # all; a column range of a row-major block is not one, so the gather call repacks it
        parts, done = [[] for _ in shapes], [0] * self.n_streams
        d_cut = self._buffer("cut", self.max_windows * win_h * 4)
        while sum(done) < total:
            room, take = self.max_windows, []
            for s in range(self.n_streams):
                take.append(min(n_new[s] - done[s], self.round_rows, room))
                room -= take[-1]
            cut_off = [int(o) for o in np.concatenate([[0], np.cumsum(take)[:-1]]) * win_h]
            for s in range(self.n_streams):
                if take[s]:
                    self.engine.gather_windows_dev(buf.ptr, src_floats,
                                                   _identity_desc(offsets[s], win_h, n_new[s], 0, [done[s]]), win_h, take[s],
                                                   d_cut.offset(cut_off[s] * 4))
                    done[s] += take[s]
            for s, r in enumerate(self._round(d_cut.ptr, d_cut.nbytes // 4, cut_off, take)):
                parts[s].append(r)
        return [_concat_bank_results(p, self.n_slots, self.db.id_to_name) for p in parts]


def live_follow_scores(engine, sheet_db, specs, levels, block_frames=20, n_slots=5, top_k=5, n_candidates=5,
                       running_frames=100, step_spec=2, catch_up=64, spec_shape=(92, 42), segments=None,
                       sheet_columns=None):
    """Which piece is every live stream playing, and where in its score is it now?  All streams run in parallel through
    one PieceTrackerBank and one ScoreFollowerBank.  `specs`: one (bins, frames) spectrogram per stream, pushed in
    rounds of block_frames columns (a stream that has ended brings empty blocks) - or any iterable of rounds, each one
    block per stream as host arrays or as the DeviceArrays handle of AudioStream.push_dev (not freed here).  levels:
    per stream the normaliser of the music gate, or one RunningLevel for all streams (the number of streams is then
    taken from `specs`: its length, or that of its first round).  Per round: the tracker bank takes the blocks; per stream the leaders
    of its last voiced frame of the round (at most n_slots of the top_k) go to set_candidates - nothing where the round
    had no voiced frame -; the follower bank takes the same blocks.  -> (one TrackResult per stream, one
    BankFollowResult per stream), the fields of the rounds concatenated."""
    running = levels if isinstance(levels, RunningLevel) else None
    if running is None:
        levels = np.ascontiguousarray(levels, dtype=np.float32)
        n = int(levels.size)
    if block_frames < 1:
        raise ValueError("block_frames must be >= 1")
    if isinstance(specs, (list, tuple)) and all(isinstance(x, np.ndarray) and x.ndim == 2 for x in specs):
        whole = [np.ascontiguousarray(x, dtype=np.float32) for x in specs]
        longest = max([x.shape[1] for x in whole] + [0])
        rounds = ([np.ascontiguousarray(x[:, f:f + block_frames]) for x in whole] for f in range(0, longest, block_frames))
        if running is not None:
            n = len(whole)
    else:
        rounds = iter(specs)
        if running is not None:
            import itertools
            first = next(rounds, None)
            if first is None:
                raise ValueError("live_follow_scores: no rounds, so no number of streams for the RunningLevel")
            n = len(first[2]) if _is_device(first) else len(first)
            rounds = itertools.chain([first], rounds)
    tracker = PieceTrackerBank(engine, sheet_db, levels, top_k, n_candidates, running_frames, spec_shape,
                               n_streams=n if running is not None else None)
    follower = None
    tracks, follows = [[] for _ in range(n)], [[] for _ in range(n)]
    try:
        follower = ScoreFollowerBank(engine, sheet_db, n, n_slots, step_spec, spec_shape, catch_up, segments, sheet_columns)
        for blocks in rounds:
            tracked = tracker.push(blocks)
            for s, r in enumerate(tracked):
                if len(r.m_prob):
                    tracks[s].append(r)
                if len(r.frames):
                    leaders = [int(p) for p in r.pieces[-1][:int(r.n_out[-1])] if int(p) in follower.segments]
                    follower.set_candidates(s, leaders[:n_slots])
            for s, r in enumerate(follower.push(blocks)):
                follows[s].append(r)
    finally:
        tracker.close()
        if follower is not None:
            follower.close()
    return ([_concat_track_results(p, sheet_db.id_to_name, top_k, n_candidates) for p in tracks],
            [_concat_bank_results(p, n_slots, sheet_db.id_to_name) for p in follows])
