"""Bars and pages for score positions.

Everything that answers "where in the score?" - locate_scores, ScoreFollower, ScoreFollowerBank, audio2sheet_align -
answers with x, a column of the strip unwrap_systems made of a piece.  A ScoreMap holds, per piece, the table of
measures asr_score_map_dev builds from the bar network's maps while the pages are unrolled (include/asr_hip.h carries
the definition, sheet_utils/omr.score_map_host restates it) and turns any strip coordinate into (bar, page, system,
page row, page column).  Bars, pages and systems count from 0 here; reports add 1 to the bar.

A measure is one int32 row: x0, x1 (strip columns, half open), page (within the piece), system (on its page), col0,
col1, row0, row1 (page coordinates of the pages the networks saw).  The rows of a piece are contiguous on the strip:
x0 of the first is 0, x1 of the last the strip's width."""
from __future__ import print_function

import numpy as np

X0, X1, PAGE, SYSTEM, COL0, COL1, ROW0, ROW1 = range(8)
FIELDS = ("bar", "page", "system", "page_row", "page_col")


class ScoreMap(object):
    """names: the pieces, in the order of the loaders; tables: per piece its (n, 8) int32 measures; widths: the strips'
    widths.  A piece without a kept system has no measure and a strip of width 0: every position in it is -1."""

    def __init__(self, names, tables, widths):
        self.names = [str(n) for n in names]
        self.tables = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 8) for t in tables]
        self.widths = np.asarray(widths, np.int64).reshape(-1)
        if not (len(self.names) == len(self.tables) == self.widths.size):
            raise ValueError("%d names, %d tables, %d widths" % (len(self.names), len(self.tables), self.widths.size))
        if len(set(self.names)) != len(self.names):
            raise ValueError("a piece is named twice")
        self._index = {n: i for i, n in enumerate(self.names)}
        for name, t, w in zip(self.names, self.tables, self.widths):
            ends = np.concatenate([[0], t[:, X1]])
            if np.any(t[:, X0] != ends[:-1]) or ends[-1] != w or np.any(t[:, X1] <= t[:, X0]):
                raise ValueError("the measures of %s do not tile its strip of %d columns" % (name, w))

    @classmethod
    def from_table(cls, names, measures, piece_first, widths):
        """from what asr_score_map_dev / score_map_host return: the pieces' rows back to back and their first rows"""
        measures = np.asarray(measures, np.int32).reshape(-1, 8)
        piece_first = np.asarray(piece_first, np.int64)
        if piece_first.size != len(names) + 1:
            raise ValueError("%d pieces, piece_first has %d entries" % (len(names), piece_first.size))
        return cls(names, [measures[a:b] for a, b in zip(piece_first[:-1], piece_first[1:])], widths)

    def __len__(self):
        return len(self.names)

    def piece_index(self, piece):
        """index of a piece given by name or by index"""
        if isinstance(piece, str):
            if piece not in self._index:
                raise KeyError("no piece %r in the score map" % piece)
            return self._index[piece]
        i = int(piece)
        if not 0 <= i < len(self.names):
            raise KeyError("no piece %d in the score map of %d" % (i, len(self.names)))
        return i

    def n_bars(self, piece):
        return len(self.tables[self.piece_index(piece)])

    def n_pages(self, piece):
        """pages of the piece up to the last one with a measure"""
        t = self.tables[self.piece_index(piece)]
        return int(t[:, PAGE].max()) + 1 if len(t) else 0

    def at(self, piece, x):
        """strip coordinates x (any shape; floats are floored, positions beyond the strip's ends go to its first / last
        column) -> (bar, page, system, page_row, page_col), int64 arrays in the shape of x: the measure by a search on
        x0, page_col = col0 + (x - x0), page_row = (row0 + row1) // 2.  -1 where x is NaN or the piece has no measure."""
        t = self.tables[self.piece_index(piece)]
        xf = np.asarray(x, np.float64)
        valid = np.isfinite(xf) & (len(t) > 0)
        out = [np.full(xf.shape, -1, np.int64) for _ in FIELDS]
        if len(t) and valid.any():
            xi = np.clip(np.floor(np.where(valid, xf, 0.0)), 0, int(t[-1, X1]) - 1).astype(np.int64)
            bar = np.searchsorted(t[:, X0].astype(np.int64), xi, side="right") - 1
            m = t[bar].astype(np.int64)
            vals = (bar, m[..., PAGE], m[..., SYSTEM], (m[..., ROW0] + m[..., ROW1]) // 2, m[..., COL0] + (xi - m[..., X0]))
            for o, v in zip(out, vals):
                o[valid] = v[valid]
        return tuple(out)

    def measure_box(self, piece, bar):
        """(page, system, row0, row1, col0, col1) of a bar: its box on the page, rows and columns half open"""
        t = self.tables[self.piece_index(piece)]
        bar = int(bar)
        if not 0 <= bar < len(t):
            raise IndexError("piece %s has bars 0 .. %d, not %d" % (self.names[self.piece_index(piece)], len(t) - 1, bar))
        m = t[bar]
        return int(m[PAGE]), int(m[SYSTEM]), int(m[ROW0]), int(m[ROW1]), int(m[COL0]), int(m[COL1])

    def rows(self, sheet_db, sheet_columns=None, w_sheet=200):
        """at() for every row of a sheet data base whose id_to_name names this map's pieces: -> (bar, page, system,
        page_row, page_col), int64 (len(sheet_db),).  sheet_columns: the strip coordinate of every row; by default
        EmbeddingDB.from_images' rule for windows of w_sheet columns (piece_identification.default_sheet_columns)."""
        from .piece_identification import default_sheet_columns
        ids = np.asarray(sheet_db.ids).reshape(-1)
        cols = default_sheet_columns(ids, w_sheet) if sheet_columns is None else np.asarray(sheet_columns, np.float64)
        if cols.shape != ids.shape:
            raise ValueError("%d sheet_columns for %d data-base rows" % (cols.size, ids.size))
        out = [np.full(ids.shape, -1, np.int64) for _ in FIELDS]
        for piece in np.unique(ids):
            sel = ids == piece
            for o, v in zip(out, self.at(sheet_db.id_to_name[int(piece)], cols[sel])):
                o[sel] = v
        return tuple(out)

    def _at_named(self, names, x):
        """at() where every column c of x (n, c) belongs to names[c]; None: an empty column"""
        x = np.asarray(x, np.float64)
        out = [np.full(x.shape, -1, np.int64) for _ in FIELDS]
        for c, name in enumerate(names):
            if name is None:
                continue
            for o, v in zip(out, self.at(name, x[:, c])):
                o[:, c] = v
        return dict(zip(FIELDS, out))

    def annotate(self, result):
        """bars and pages of a result: a candidate dict of locate_scores (name, x, start_x, end_x), a FollowResult or a
        BankFollowResult.  -> {"x": {bar, page, system, page_row, page_col}, "start_x": {...}} (a candidate dict also
        gives "end_x"), int64 arrays in the shape the result's x / start_x have; -1 in empty slots."""
        if isinstance(result, dict):
            keys = [k for k in ("x", "start_x", "end_x") if k in result]
            return {k: dict(zip(FIELDS, self.at(result["name"], result[k]))) for k in keys}
        if hasattr(result, "piece"):                         # BankFollowResult: the slots change their pieces
            piece = np.asarray(result.piece)
            out = {k: {f: np.full(piece.shape, -1, np.int64) for f in FIELDS} for k in ("x", "start_x")}
            for p in np.unique(piece[piece >= 0]):
                sel = piece == p
                for k in ("x", "start_x"):
                    for f, v in zip(FIELDS, self.at(result.names[int(p)], np.asarray(getattr(result, k))[sel])):
                        out[k][f][sel] = v
            return out
        return {k: self._at_named(result.names, getattr(result, k)) for k in ("x", "start_x")}

    # -- files ----------------------------------------------------------------------------------------------------------
    def save(self, path):
        """one .npz: names, widths, the tables back to back and their first rows"""
        counts = np.asarray([len(t) for t in self.tables], np.int64)
        np.savez(path, names=np.asarray(self.names, dtype=np.str_), widths=self.widths,
                 piece_first=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                 measures=np.concatenate(self.tables) if self.tables else np.zeros((0, 8), np.int32))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as f:
            return cls.from_table([str(n) for n in f["names"]], f["measures"], f["piece_first"], f["widths"])

    @staticmethod
    def path_for(db_file):
        """the map's file next to a data-base file: <stem>_score_map.npz"""
        import os
        return os.path.splitext(db_file)[0] + "_score_map.npz"
