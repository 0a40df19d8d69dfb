"""The tile store restated in Python: what sits between
BatchingProcessor.forward and the tile files of AnonymisingProcessor in the streaming reporter.
Rows are built by oracle.tiles.stream_rows_from_reports and kept in arrival order; the flush
sorts every file as Collections.sort does (stable, Segment.compareTo) and cleans it with
oracle.tiles.java_clean, which tests/golden/cull_cases.json pins to the reference loop.  A helper
module (no tests, no fixtures): tests/test_tile_store_cpu.py pins what it computes and what the
script below covers, tests/test_gpu_tile_store.py holds the device store equal to it.

A "reports" dict is the layout of a session result: rep_off (n_windows + 1), id, next_id, t0, t1,
length, queue_length."""
import numpy as np

from oracle import tiles as T

NO_ID = T.NO_ID
REPORT_TYPES = (('id', np.uint64), ('next_id', np.uint64), ('t0', np.float64), ('t1', np.float64),
                ('length', np.int32), ('queue_length', np.int32))
FLUSH_ARRAYS = ('rows', 'file', 'row_off', 'n_unclean')
FLUSH_COUNTS = ('n_rows_in', 'n_rows', 'n_files', 'n_files_empty')


def valid(t0, t1, length, queue):
    """Segment.valid (Segment.java:38-40), term by term."""
    return t0 > 0 and t1 > 0 and t1 > t0 and length > 0 and queue >= 0


def rows_of(reports, q):
    return T.stream_rows_from_reports({'trace_rep_off': np.asarray(reports['rep_off']), 'rep_id': reports['id'],
                                       'rep_next': reports['next_id'], 'rep_t0': reports['t0'],
                                       'rep_t1': reports['t1'], 'rep_length': reports['length'],
                                       'rep_queue': reports['queue_length']}, q)


class Store:
    def __init__(self, max_rows, quantisation, privacy):
        self.max_rows, self.q, self.privacy = int(max_rows), int(quantisation), int(privacy)
        self.held = []   # arrival-order row arrays since the last flush

    @property
    def n_rows(self):
        return sum(len(r) for r in self.held)

    def _append(self, rows):
        if self.n_rows + len(rows) > self.max_rows:
            raise ValueError('the add would take the store beyond max_rows')
        self.held.append(rows)

    def add_reports(self, reports):
        """The counts of otr_tile_add_result; ValueError past max_rows, the store as it was."""
        rows = rows_of(reports, self.q)
        n_valid = sum(1 for k in range(len(reports['id'])) if valid(
            float(reports['t0'][k]), float(reports['t1'][k]), int(reports['length'][k]),
            int(reports['queue_length'][k])))
        self._append(rows)
        return {'n_reports': len(reports['id']), 'n_valid': n_valid, 'n_rows_added': len(rows),
                'n_rows': self.n_rows}

    def add_rows(self, rows):
        rows = np.asarray(rows, T.TILE_ROW)
        self._append(rows)
        return {'n_reports': 0, 'n_valid': 0, 'n_rows_added': len(rows), 'n_rows': self.n_rows}

    def arrival_rows(self):
        return np.concatenate(self.held + [np.zeros(0, T.TILE_ROW)])

    def flush(self):
        """The arrays and counts of otr_tile_flush_result; the store is empty afterwards."""
        rows = self.arrival_rows()
        self.held = []
        kept, files, off, unclean, empty = [], [], [0], [], 0
        for f in sorted(set(rows['file'].tolist())):
            v = [r for r in rows if int(r['file']) == f]                      # arrival order
            v = sorted(v, key=lambda r: (int(r['id']), int(r['next_id'])))    # stable, as Collections.sort
            k = T.java_clean(v, self.privacy)
            if not k:
                empty += 1
                continue
            kept += k
            files.append(f)
            off.append(len(kept))
            unclean.append(len(v))
        return {'rows': np.array(kept, T.TILE_ROW) if kept else np.zeros(0, T.TILE_ROW),
                'file': np.array(files, np.uint64), 'row_off': np.array(off, np.int64),
                'n_unclean': np.array(unclean, np.int64), 'n_rows_in': len(rows), 'n_rows': len(kept),
                'n_files': len(files), 'n_files_empty': empty, 'quantisation': self.q}


def differing(got, want):
    """What differs between two flushes: the arrays bit for bit, the counts by value."""
    bad = []
    for k in FLUSH_ARRAYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append('%s: got %s %s want %s %s' % (k, a.shape, a.tolist()[:4], b.shape, b.tolist()[:4]))
    for k in FLUSH_COUNTS:
        if int(got[k]) != int(want[k]):
            bad.append('%s: got %d want %d' % (k, got[k], want[k]))
    return bad


def reports_of(windows):
    """windows: lists of (id, next_id, t0, t1, length, queue_length) -> a reports dict."""
    reps = [r for w in windows for r in w]
    out = {'rep_off': np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.int64)}
    for j, (k, dt) in enumerate(REPORT_TYPES):
        out[k] = np.array([r[j] for r in reps], dt)
    return out


# tests/sessions_ref.py's city stream yields three valid reports, at seconds 35.2-52.9, 28.4-40.0
# and 8.5-14.7 of their minutes: none crosses a 60 s bucket boundary.  With every time this many
# seconds later the first one does (45.2-62.9) and no other (38.4-50.0, 18.5-24.7)
CITY_SHIFT = 10


# ---- the hand-built script: GPU jobs `scripted`, `persistence`, `capacity`, `rows` and the CPU pins
SCRIPT_Q = 60
T0 = 1500000000           # a bucket start: 25,000,000 * 60
SCRIPT_FLUSH_AFTER = (2, 3, 4)   # adds 0-2, flush; add 3, flush; add 4, flush


def sid(level, tile, index):
    """An OSMLR id: level (3 bits) | tile (22) | index (21)."""
    return level | (tile << 3) | (index << 25)


def script_adds():
    """Five adds of reports (what tests/test_tile_store_cpu.py::test_script_coverage lists)."""
    X, Y = (1, 1000), (0, 1000)            # two tiles that differ only in level
    # add 0, window 0: 65 reports on tile X, five pairs in turn (arrival order is not pair order);
    # the reports at positions 63 and 64 (either side of a 64-report chunk) span three buckets
    w0 = []
    for k in range(65):
        t0 = T0 + 2 + 0.25 * k
        t1 = t0 + 1.5 + (k % 3)             # 1.5, 2.5 (a tie of Math.round), 3.5
        if k in (63, 64):
            t0, t1 = T0 + 50 + (k - 63), T0 + 170.5
        w0.append((sid(*X, k % 5), sid(*X, (k + 1) % 5), t0, t1, 40 + k, k % 4))
    # window 2: 129 reports on tile Y, seven pairs; positions 127 and 128 span two buckets
    w2 = []
    for k in range(129):
        t0 = T0 + 61 + 0.125 * k
        t1 = t0 + 4.25 if k < 127 else T0 + 121.75
        w2.append((sid(*Y, k % 7), sid(*Y, (k + 3) % 7), t0, t1, 500 - k, 0))
    # window 3: one report failing each term of Segment.valid, and a next_id of none
    bad = [(sid(2, 70, 1), sid(2, 70, 2), -5.0, T0 + 9.0, 10, 0),           # t0 > 0
           (sid(2, 70, 1), sid(2, 70, 2), T0 + 1.0, -1.0, 10, 0),           # t1 > 0
           (sid(2, 70, 1), sid(2, 70, 2), T0 + 7.0, T0 + 7.0, 10, 0),       # t1 > t0 (equal)
           (sid(2, 70, 1), sid(2, 70, 2), T0 + 1.0, T0 + 9.0, 0, 0),        # length > 0
           (sid(2, 70, 1), sid(2, 70, 2), T0 + 1.0, T0 + 9.0, 10, -1)]      # queue_length >= 0
    w3 = bad + [(sid(2, 70, 3), NO_ID, T0 + 3.0, T0 + 8.75, 33, 2)]
    # the pair P on tile (2, 77): one row in each of adds 0, 1, 2, durations 10, 20, 31
    P = (sid(2, 77, 1), sid(2, 77, 2))
    # tile (2, 79): rows A (add 0) and B (add 2) of different pairs, nothing else: clean's last
    # range [A, B] keeps both at privacy 2
    A = (sid(2, 79, 1), sid(2, 79, 2), T0 + 10.0, T0 + 14.0, 90, 0)
    B = (sid(2, 79, 3), NO_ID, T0 + 11.0, T0 + 17.0, 91, 1)
    add0 = [w0, [], w2, w3, [P + (T0 + 20.0, T0 + 30.0, 120, 0), A]]
    # add 1: P again, and tile (2, 78) with a single row: cleaned to nothing at privacy 2
    add1 = [[P + (T0 + 25.0, T0 + 45.4, 120, 1)],
            [(sid(2, 78, 5), sid(2, 78, 6), T0 + 30.0, T0 + 33.0, 60, 0)]]
    add2 = [[B], [], [P + (T0 + 28.0, T0 + 58.5, 120, 0)]]
    # add 3 (the second interval): tile X again; a pair seen twice around a singleton in sort order
    add3 = [[(sid(*X, 2), sid(*X, 3), T0 + 600.0, T0 + 604.0, 44, 0),
             (sid(*X, 1), sid(*X, 2), T0 + 601.0, T0 + 603.0, 45, 0),
             (sid(*X, 2), sid(*X, 3), T0 + 602.0, T0 + 609.0, 46, 0),
             (sid(*X, 0), sid(*X, 1), T0 + 603.0, T0 + 605.0, 47, 0),
             (sid(*X, 0), sid(*X, 1), T0 + 604.0, T0 + 606.0, 48, 0)]]
    # add 4 (the third): two windows over a bucket boundary
    add4 = [[(sid(*Y, 1), sid(*Y, 2), T0 + 1259.0, T0 + 1261.0, 70, 0)],
            [(sid(*Y, 1), sid(*Y, 2), T0 + 1258.5, T0 + 1262.0, 71, 3),
             (sid(*Y, 4), NO_ID, T0 + 1201.0, T0 + 1202.0, 72, 0)]]
    return [reports_of(a) for a in (add0, add1, add2, add3, add4)]


def script_flushes(privacy, max_rows=1 << 20):
    """(per-add counts, the flushes) of the script through the restatement."""
    ref = Store(max_rows, SCRIPT_Q, privacy)
    adds, flushes = [], []
    for i, a in enumerate(script_adds()):
        adds.append(ref.add_reports(a))
        if i in SCRIPT_FLUSH_AFTER:
            flushes.append(ref.flush())
    return adds, flushes
