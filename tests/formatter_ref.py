"""The stream formatter's rule restated in plain Python: what
KeyedFormattingProcessor.java:32-43 does with Formatter.formatSV / formatJSON
(Formatter.java:97-124) to one message.  Every message ends kept (a point), dropped (the
reference certainly throws) or unsupported (the reference might produce a point that cannot be
reproduced without a JVM).  Over a message any drop beats any unsupported reading; within a
class the first in the reference's evaluation order (lat, lon, time, accuracy, uuid) is the
reason.  This file is the authority for the table; the device code (otr_formatter.h) and its
host build are compared with it.

Numbers: a decimal is read as its first 19 significant digits w and an exponent q, with a
flag when a nonzero digit was cut; its double is the correctly rounded one (exact rational
arithmetic here), and when digits were cut the value counts as decidable only if w and w + 1
round to the same double (K11's rule, otr_ingest.h dec_to_double).  The one thing not restated
is Eisel-Lemire's own give-up case, which no input of at most 19 digits is known to reach.
"""
import datetime
import re
from fractions import Fraction

import numpy as np

KEPT, DROPPED, UNSUPPORTED = 0, 1, 2
# reasons (include/otr.h OTR_FORMAT_D_* / OTR_FORMAT_U_*): below 32 dropped, from 32 unsupported
D_FIELDS, D_FLOAT, D_INT, D_TIME, D_ACCURACY, D_JSON, D_ROOT, D_MISSING = 1, 2, 3, 4, 5, 6, 7, 8
U_PRECISION, U_ACCURACY, U_DEPTH, U_TRAILING, U_ESCAPE, U_NUMBER, U_KIND, U_NO_ID = 32, 33, 34, 35, 36, 37, 38, 39
REASONS = (D_FIELDS, D_FLOAT, D_INT, D_TIME, D_ACCURACY, D_JSON, D_ROOT, D_MISSING,
           U_PRECISION, U_ACCURACY, U_DEPTH, U_TRAILING, U_ESCAPE, U_NUMBER, U_KIND, U_NO_ID)
TIME_EPOCH, TIME_YMDHMS = 0, 1
NO_ID = 0xFFFFFFFFFFFFFFFF
MAX_DEPTH = 64

# the formats of FormatterTest.java:30-31, the README's JSON spec and a plain epoch CSV
SPECS = {'psv': ',sv,\\|,1,9,10,0,5,yyyy-MM-dd HH:mm:ss', 'json_ymd': '@json@id@la@lo@t@a@yyyy-MM-dd HH:mm:ss',
         'json': '@json@id@latitude@longitude@timestamp@accuracy', 'csv': ';sv;,;0;1;2;3;4'}
FORMATS = {
    'psv': {'type': 'sv', 'separator': '|', 'uuid_index': 1, 'lat_index': 9, 'lon_index': 10, 'time_index': 0,
            'accuracy_index': 5, 'time_format': TIME_YMDHMS},
    'csv': {'type': 'sv', 'separator': ',', 'uuid_index': 0, 'lat_index': 1, 'lon_index': 2, 'time_index': 3,
            'accuracy_index': 4, 'time_format': TIME_EPOCH},
    'json_ymd': {'type': 'json', 'uuid_key': 'id', 'lat_key': 'la', 'lon_key': 'lo', 'time_key': 't',
                 'accuracy_key': 'a', 'time_format': TIME_YMDHMS},
    'json': {'type': 'json', 'uuid_key': 'id', 'lat_key': 'latitude', 'lon_key': 'longitude',
             'time_key': 'timestamp', 'accuracy_key': 'accuracy', 'time_format': TIME_EPOCH},
}

_WS = b' \t\n\x0b\x0c\r'
_DEC = re.compile(rb'[ \t\n\x0b\x0c\r]*([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?[ \t\n\x0b\x0c\r]*')
_INT = re.compile(rb'[ \t\n\x0b\x0c\r]*[+-]?[0-9]+[ \t\n\x0b\x0c\r]*')
_LONG = re.compile(rb'[+-]?[0-9]+')


def uuid_hash(b):
    """K11's key: FNV-1a over the bytes, then a splitmix64 finaliser."""
    h, m = 0xcbf29ce484222325, (1 << 64) - 1
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & m
    h ^= h >> 30
    h = (h * 0xbf58476d1ce4e5b9) & m
    h ^= h >> 27
    h = (h * 0x94d049bb133111eb) & m
    return h ^ (h >> 31)


def _dec(text):
    """(negative, w, q, cut) of a finite decimal in Python's float() grammar, or None."""
    m = _DEC.fullmatch(text)
    if not m:
        return None
    sign, ip, fp, fp_only, ex = m.groups()
    ip, fp = (ip or b''), (fp if fp is not None else (fp_only or b''))
    digits = (ip + fp).lstrip(b'0')
    q = -len(fp) + (max(-1000000, min(1000000, int(ex))) if ex else 0)
    cut = False
    if len(digits) > 19:
        cut = digits[19:].strip(b'0') != b''
        q += len(digits) - 19
        digits = digits[:19]
    return sign == b'-', int(digits or b'0'), max(-1000000, min(1000000, q)), cut


def _exact(w, q):
    if w == 0:
        return 0.0
    if q > 400:
        return float('inf')
    if q < -400:
        return 0.0
    try:
        return float(Fraction(w) * Fraction(10) ** q)
    except OverflowError:
        return float('inf')


def _double(d):
    """The double of a _dec, or None where the cut digits leave the rounding undecided."""
    neg, w, q, cut = d
    v = _exact(w, q)
    if cut and _exact(w + 1, q) != v:
        return None
    return -v if neg else v


def _f32(v):
    with np.errstate(over='ignore'):
        return np.float32(v)


def _coord_text(text):
    """(reason, float32): floatFormatter.parse(text).floatValue() under K11's JAVA_SV reading."""
    d = _dec(text)
    if d is None:
        return D_FLOAT, None
    v = _double(d)
    if v is None:
        return U_PRECISION, None
    if v != v or v in (float('inf'), float('-inf')):
        return D_FLOAT, None
    return 0, _f32(v)


def _ceil_acc(x):
    """(reason, int): (int)Math.ceil(x) with Java's saturating cast, then K11's bound."""
    if x != x:
        return U_ACCURACY, None
    if x in (float('inf'), float('-inf')):
        a = 2147483647 if x > 0 else -2147483648
    else:
        a = max(-2147483648, min(2147483647, int(np.ceil(x))))
    return (U_ACCURACY, None) if abs(a) > 16777216 else (0, a)


def _time_text(text):
    """(reason, seconds) of K11's fast 'yyyy-MM-dd HH:mm:ss': six slices, separators unchecked."""
    v = []
    for lo, hi in ((0, 4), (5, 7), (8, 10), (11, 13), (14, 16), (17, 19)):
        piece = text[lo:hi]
        if not _INT.fullmatch(piece):
            return D_INT, None
        v.append(int(piece.strip(_WS)))
    if not (1 <= v[0] <= 9999 and 1 <= v[1] <= 12):
        return D_TIME, None
    days = datetime.date(v[0], v[1], 1).toordinal() - 719163 + v[2] - 1
    return 0, ((days * 24 + v[3]) * 60 + v[4]) * 60 + v[5]


def _long(text):
    """Long.parseLong / an integer within int64, or None."""
    if not _LONG.fullmatch(text):
        return None
    x = int(text)
    return x if -(1 << 63) <= x < (1 << 63) else None


class _Verdict:
    def __init__(self):
        self.drop = self.unsup = 0

    def add(self, r):
        if r and r < UNSUPPORTED_FROM:
            self.drop = self.drop or r
        elif r:
            self.unsup = self.unsup or r


UNSUPPORTED_FROM = 32


def _result(reason, uuid=None, lat=None, lon=None, acc=None, tm=None):
    if reason:
        return (DROPPED if reason < UNSUPPORTED_FROM else UNSUPPORTED), reason, None, None, None, None, None
    return KEPT, 0, uuid, lat, lon, acc, tm


def format_sv(msg, fmt):
    """(status, reason, uuid bytes, float32 lat, float32 lon, acc, time) of one SV message."""
    parts = msg.split(fmt['separator'].encode('latin-1'))
    while parts and parts[-1] == b'':   # String.split drops the trailing empty strings
        parts.pop()
    idx = {k: fmt[k + '_index'] for k in ('uuid', 'lat', 'lon', 'time', 'accuracy')}
    if any(i >= len(parts) for i in idx.values()):
        return _result(D_FIELDS)
    v = _Verdict()
    r, lat = _coord_text(parts[idx['lat']])
    v.add(r)
    r, lon = _coord_text(parts[idx['lon']])
    v.add(r)
    if fmt['time_format'] == TIME_YMDHMS:
        r, tm = _time_text(parts[idx['time']])
    else:
        tm = _long(parts[idx['time']])
        r = D_INT if tm is None else 0
    v.add(r)
    acc = None
    d = _dec(parts[idx['accuracy']])
    if d is None:
        v.add(D_ACCURACY)
    else:
        x = _double(d)
        if x is None:
            v.add(U_PRECISION)
        else:
            r, acc = _ceil_acc(float(_f32(x)))   # through float: floatValue()
            v.add(r)
    uuid = parts[idx['uuid']]
    if uuid_hash(uuid) == NO_ID:
        v.add(U_NO_ID)
    return _result(v.drop or v.unsup, uuid, lat, lon, acc, tm)


# ---- JSON: a raw scanner of one RFC 8259 value ------------------------------------------------
class _Invalid(Exception):
    pass


class _Deep(Exception):
    pass


_JWS = b' \t\n\r'
_NUMBER = re.compile(rb'-?(?:0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?')
_STRING = re.compile(rb'"((?:[^"\\\x00-\x1f]|\\["\\/bfnrt]|\\u[0-9a-fA-F]{4})*)"')


class Scanner:
    """Validates one value and keeps the root object's members as raw text: a list of
    (key bytes without quotes, kind, raw value bytes) with kind one of 'string' (raw: inside
    the quotes), 'number' (the token), 'literal', 'container'."""

    def __init__(self, text, max_depth=MAX_DEPTH):
        self.s, self.max_depth = text, max_depth
        self.members, self.root = [], None

    def ws(self, p):
        while p < len(self.s) and self.s[p] in _JWS:
            p += 1
        return p

    def scan(self):
        """The position after the root value (whitespace before it skipped)."""
        return self.value(self.ws(0), 0)

    def string(self, p):
        m = _STRING.match(self.s, p)
        if not m:
            raise _Invalid(p)
        return m.group(1), m.end()

    def value(self, p, depth):
        s = self.s
        if p >= len(s):
            raise _Invalid(p)
        c = s[p:p + 1]
        if depth == 0:
            self.root = 'object' if c == b'{' else 'other'
        if c in (b'{', b'['):
            if depth == self.max_depth:
                raise _Deep(p)
            return self.object(p + 1, depth + 1) if c == b'{' else self.array(p + 1, depth + 1)
        if c == b'"':
            return self.string(p)[1]
        if c == b'-' or c.isdigit():
            m = _NUMBER.match(s, p)
            if not m:
                raise _Invalid(p)
            return m.end()
        for word in (b'true', b'false', b'null'):
            if s.startswith(word, p):
                return p + len(word)
        raise _Invalid(p)

    def kind_of(self, p, end):
        c = self.s[p:p + 1]
        if c == b'"':
            return 'string', self.s[p + 1:end - 1]
        if c in (b'{', b'['):
            return 'container', self.s[p:end]
        if c in (b't', b'f', b'n'):
            return 'literal', self.s[p:end]
        return 'number', self.s[p:end]

    def object(self, p, depth):
        p = self.ws(p)
        if self.s[p:p + 1] == b'}':
            return p + 1
        while True:
            p = self.ws(p)
            key, p = self.string(p)
            p = self.ws(p)
            if self.s[p:p + 1] != b':':
                raise _Invalid(p)
            p = self.ws(p + 1)
            if depth == 1:
                # recorded when the value starts, as a container may end the scan inside it
                slot = len(self.members)
                self.members.append((key, 'container', b''))
            end = self.value(p, depth)
            if depth == 1:
                self.members[slot] = (key,) + self.kind_of(p, end)
            p = self.ws(end)
            c = self.s[p:p + 1]
            if c == b'}':
                return p + 1
            if c != b',':
                raise _Invalid(p)
            p += 1

    def array(self, p, depth):
        p = self.ws(p)
        if self.s[p:p + 1] == b']':
            return p + 1
        while True:
            p = self.ws(self.value(self.ws(p), depth))
            c = self.s[p:p + 1]
            if c == b']':
                return p + 1
            if c != b',':
                raise _Invalid(p)
            p += 1


def json_valid(text, max_depth=10 ** 6):
    """(valid, end of the root value) of the restatement's grammar alone (the grammar pin)."""
    sc = Scanner(text, max_depth)
    try:
        return True, sc.scan()
    except _Invalid:
        return False, None


def _number_flags(tok):
    m = _NUMBER.fullmatch(tok)
    return m.group(1) is None and m.group(2) is None, m.group(2) is not None   # integer, exponent


def _json_coord(member):
    if member is None:
        return D_MISSING, None
    kind, raw = member
    if kind == 'string':
        return (U_ESCAPE, None) if b'\\' in raw else _coord_text(raw)
    if kind != 'number':
        return U_KIND, None
    if _number_flags(raw)[1]:
        return U_NUMBER, None
    v = _double(_dec(raw))
    if v is None:
        return U_PRECISION, None
    # beyond [1e-3, 1e7) Double.toString prints E-notation, which DecimalFormat reads to the 'E'
    if not (v == 0 or 1e-3 <= abs(v) < 1e7):
        return U_NUMBER, None
    return 0, _f32(v)


def _json_time(member, time_format):
    if member is None:
        return D_MISSING, None
    kind, raw = member
    if time_format == TIME_YMDHMS:
        if kind == 'string':
            return (U_ESCAPE, None) if b'\\' in raw else _time_text(raw)
        return (D_TIME if kind == 'number' else U_KIND), None
    if kind != 'number':
        return U_KIND, None
    x = _long(raw) if _number_flags(raw)[0] else None
    return (U_NUMBER, None) if x is None else (0, x)


def _json_acc(member):
    if member is None:
        return D_MISSING, None
    kind, raw = member
    if kind != 'number':
        return U_KIND, None
    v = _double(_dec(raw))
    return (U_PRECISION, None) if v is None else _ceil_acc(v)   # the double, not a float as in SV


def _json_uuid(member):
    if member is None:
        return D_MISSING, None
    kind, raw = member
    if kind == 'string':
        return (U_ESCAPE, None) if b'\\' in raw else (0, raw)
    if kind != 'number':
        return U_KIND, None
    if not _number_flags(raw)[0] or _long(raw) is None or raw == b'-0':
        return U_NUMBER, None
    return 0, raw


def format_json(msg, fmt):
    """(status, reason, uuid bytes, float32 lat, float32 lon, acc, time) of one JSON message."""
    sc = Scanner(msg)
    try:
        end = sc.scan()
    except _Invalid:
        return _result(D_JSON)
    except _Deep:
        return _result(U_DEPTH)
    if sc.root != 'object':
        return _result(D_ROOT)
    if any(b'\\' in key for key, _, _ in sc.members):
        return _result(U_ESCAPE)
    last = {}
    for key, kind, raw in sc.members:   # ObjectNode replaces: the last duplicate wins
        last[key] = (kind, raw)
    get = lambda name: last.get(fmt[name + '_key'].encode('latin-1'))
    v = _Verdict()
    r, lat = _json_coord(get('lat'))
    v.add(r)
    r, lon = _json_coord(get('lon'))
    v.add(r)
    r, tm = _json_time(get('time'), fmt['time_format'])
    v.add(r)
    r, acc = _json_acc(get('accuracy'))
    v.add(r)
    r, uuid = _json_uuid(get('uuid'))
    v.add(r)
    if v.drop:
        return _result(v.drop)
    if msg[end:].strip(_JWS):
        return _result(U_TRAILING)   # readTree stops after the first value
    if v.unsup:
        return _result(v.unsup)
    if uuid_hash(uuid) == NO_ID:
        return _result(U_NO_ID)
    return _result(0, uuid, lat, lon, acc, tm)


def format_message(msg, fmt):
    return format_json(msg, fmt) if fmt['type'] == 'json' else format_sv(msg, fmt)


def split_lines(text):
    """K11's line rule: '\\n'-separated, a final fragment without '\\n' counts."""
    parts = text.split(b'\n')
    return parts[:-1] if parts[-1] == b'' else parts


def to_points(results, timestamps):
    """The kept messages as session points in arrival order, with 'message' (arrival index) and
    'uuid' (bytes) per point, and 'status' (0 or the reason) per message."""
    kept = [(i, r) for i, r in enumerate(results) if r[0] == KEPT]
    ts = np.broadcast_to(np.asarray(timestamps, np.int64), (len(results),))
    return {'key': np.array([uuid_hash(r[2]) for _, r in kept], np.uint64),
            'lat': np.array([r[3] for _, r in kept], np.float32), 'lon': np.array([r[4] for _, r in kept], np.float32),
            'accuracy': np.array([r[5] for _, r in kept], np.int32), 'time': np.array([r[6] for _, r in kept], np.int64),
            'timestamp': np.array([ts[i] for i, _ in kept], np.int64),
            'message': np.array([i for i, _ in kept], np.int64), 'uuid': [r[2] for _, r in kept],
            'status': np.array([r[1] for r in results], np.int32),
            'n_dropped': sum(r[0] == DROPPED for r in results),
            'n_unsupported': sum(r[0] == UNSUPPORTED for r in results)}


# ---- renderers: a point stream as messages ----------------------------------------------------
def render_float(x):
    """'%.9g' of a float32 without exponent: nine significant digits give its bits back."""
    s = '%.9g' % float(x)
    if 'e' in s or 'inf' in s or 'nan' in s:
        s = np.format_float_positional(float(x), precision=9, unique=False, fractional=False, trim='-')
    return s


def render_time(t, time_format):
    if time_format == TIME_EPOCH:
        return '%d' % t
    d = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=int(t))
    return d.strftime('%Y-%m-%d %H:%M:%S')


def uuid_of_key(key):
    return ('veh-%d' % int(key)).encode()


def render_sv(points, fmt):
    """One SV message per point; the fields no index names hold filler."""
    idx = {fmt[k + '_index']: k for k in ('uuid', 'lat', 'lon', 'time', 'accuracy')}
    out = []
    for i in range(len(points['key'])):
        val = {'uuid': uuid_of_key(points['key'][i]).decode(), 'lat': render_float(points['lat'][i]),
               'lon': render_float(points['lon'][i]), 'time': render_time(points['time'][i], fmt['time_format']),
               'accuracy': '%d' % points['accuracy'][i]}
        out.append(fmt['separator'].join(val[idx[j]] if j in idx else ('x' if j % 3 else '')
                                         for j in range(max(idx) + 1)).encode())
    return out


def render_json(points, fmt):
    """One JSON message per point: numbers as number tokens, a quoted time under a pattern, the
    members rotated from message to message and a nested filler member on every third."""
    out = []
    for i in range(len(points['key'])):
        tm = render_time(points['time'][i], fmt['time_format'])
        members = [(fmt['uuid_key'], '"%s"' % uuid_of_key(points['key'][i]).decode()),
                   (fmt['lat_key'], render_float(points['lat'][i])), (fmt['lon_key'], render_float(points['lon'][i])),
                   (fmt['time_key'], '"%s"' % tm if fmt['time_format'] == TIME_YMDHMS else tm),
                   (fmt['accuracy_key'], '%d' % points['accuracy'][i])]
        if i % 3 == 0:
            members.append(('extra', '{"%s": [1, {"x": null}], "s": "a\\"b"}' % fmt['lat_key']))
        members = members[i % len(members):] + members[:i % len(members)]
        sep = ', ' if i % 2 else ','
        out.append(('{' + sep.join('"%s":%s' % kv for kv in members) + '}').encode())
    return out


def rendered_keys(points):
    """The points with the keys their rendered uuids hash to."""
    out = dict(points)
    out['key'] = np.array([uuid_hash(uuid_of_key(k)) for k in points['key']], np.uint64)
    return out


# ---- the corpus ---------------------------------------------------------------------------------
def _deep(n):
    return b'{"id":"u","la":1,"lo":2,"t":"2017-01-01 00:00:00","a":1,"z":' + b'[' * (n - 1) + b']' * (n - 1) + b'}'


def corpus():
    """(format name, message) pairs: every row of the table at least once."""
    sv = [b'2017-01-01 06:05:40|w00t||||6.5||||0.0|0.0',                       # FormatterTest.java:34
          b'2017-01-01 06:05:40|w00t||||6.5||||52.5|13.4|',                    # a trailing empty field
          b'2017-01-01 06:05:40|w00t||||6.5||||52.5|13.4|||',
          b'2017-01-01 06:05:40|w00t||||6.5||||52.5|',                         # lon is a dropped trailing empty
          b'2017-01-01 06:05:40|w00t||||6.5||||52.5',
          b'', b'|', b'||||||||||', b'a|b',
          b'2017-01-01 06:05:40|w00t||||6.5||||north|13.4',
          b'2017-01-01 06:05:40|w00t||||6.5||||52.5|1e999',
          b'2017-01-01 06:05:40|w00t||||6.5|||| 5.25e1 |+13.4',
          b'2017-01-01 06:05:40|w00t||||6.5||||.5|5.',
          b'2017-01-01 06:05:40|w00t||||6.5||||52.123456789012345678901|13.4',  # > 19 digits, decidable
          b'2017-01-01 06:05:40|w00t||||6.5||||9007199254740993.00000000000000000001|13.4',  # cut digits decide
          b'2017-01-01 06:05:40|w00t||||x||||52.5|13.4',
          b'2017-01-01 06:05:40|w00t||||||||52.5|13.4',
          b'2017-01-01 06:05:40|w00t||||16777216.5||||52.5|13.4',              # through float: 16777216
          b'2017-01-01 06:05:40|w00t||||16777217.5||||52.5|13.4',              # float 16777218: beyond 2^24
          b'2017-01-01 06:05:40|w00t||||-16777216||||52.5|13.4',
          b'2017-01-01 06:05:40|w00t||||-1e30||||52.5|13.4',
          b'2017-01-01 06:05:40|w00t||||1e999||||52.5|13.4',
          b'2017-01-01 06:05:40|w00t||||-0.5||||52.5|13.4',
          b'2017-01-01 06:05:40|w00t||||1.00000000000000000000001||||52.5|13.4',
          b'2017-13-01 06:05:40|w00t||||6.5||||52.5|13.4',
          b'2017-01-01 06:0x:40|w00t||||6.5||||52.5|13.4',
          b'2017-01-01|w00t||||6.5||||52.5|13.4',
          b'2017/01/99T25:61:61 and more|w00t||||6.5||||52.5|13.4',
          b'0000-01-01 00:00:00|w00t||||6.5||||52.5|13.4',
          b'2017-01-01 06:05:40|||||6.5||||52.5|13.4',                          # an empty uuid
          b'2017-01-01 06:05:40|v\xc3\xa9hicule \xff||||6.5||||52.5|13.4',
          b'2017-13-01 06:05:40|w00t||||16777217.5||||52.5|13.4',              # a drop beats an unsupported
          b'2017-01-01 06:05:40|w00t||||x||||52.123456789012345678905e-300|13.4']
    csv = [b'u1,52.5,13.4,1483250740,5', b'u1,52.5,13.4,+1483250740,5.01', b'u1,52.5,13.4, 1483250740,5',
           b'u1,52.5,13.4,9223372036854775807,5', b'u1,52.5,13.4,9223372036854775808,5',
           b'u1,52.5,13.4,-9223372036854775808,5', b'u1,52.5,13.4,12.0,5', b'u1,52.5,13.4,,5', b'u1,52.5,13.4,1483250740',
           b'u1,52.5,13.4,1483250740,5,,,', b',52.5,13.4,1483250740,5']
    ymd = [b'{"t":"2017-01-01 06:05:40","id":"w00t","la":0.0,"lo":0.0,"a":6.5}',    # FormatterTest.java:38
           b' {"t" : "2017-01-01 06:05:40" ,\t"id":"w00t",\r\n"la":52.5,"lo":13.4,"a":6.5 } ',
           b'{"t":"2017-01-01 06:05:40","id":"first","la":1,"lo":2,"a":6.5,"id":"last","la":"3.5","a":7}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":5.0E-4,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":0.0005,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":0.001,"lo":9999999.5,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":10000000,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":-0.0,"lo":-0,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":1e1,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":"1e1","lo":" 13.4 ","a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":"north","lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":"5\\u0032","lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":true,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":null,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":[52.5],"lo":{"v":13.4},"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.123456789012345678901,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":9007199254740993.00000000000000000001,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","x":{"la":52.5},"lo":13.4,"a":6.5}',
           b'{"t":1483250740,"id":"w00t","la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":false,"id":"w00t","la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-13-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:4x","id":"w00t","la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01\\t06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":16777216.5}',   # ceil of the double: 16777217
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":16777215.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":-16777216.9}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":1e999}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":-0.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":"6.5"}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":1.00000000000000000000001}',
           b'{"t":"2017-01-01 06:05:40","id":12345,"la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":-0,"la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":-7,"la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":1.5,"la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":9223372036854775808,"la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":null,"la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w\\"t","la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"","la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"v\xc3\xa9hicule \xff","la":52.5,"lo":13.4,"a":6.5}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":6.5,"k\\u0061":1}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":6.5,"z":{"k\\n":"\\u00e9\\/"}}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":6.5} x',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","la":52.5,"lo":13.4,"a":6.5}{}',
           b'{"t":"2017-01-01 06:05:40","id":"w00t","lo":13.4,"a":6.5} x',               # missing beats trailing
           b'[1,2] x', b'5', b'"text"', b'[]', b'null', b'{}', b'', b' ', b'{', b'{"a"}', b'{"a":}', b'{"a":1,}',
           b'{,}', b'[1,]', b'{"a":01}', b'{"a":1.}', b'{"a":.5}', b'{"a":+1}', b'{"a":1e}', b'{"a":-}',
           b'{"a":tru}', b'{"a":True}', b'{"a":NaN}', b'{"a":Infinity}', b'{"a":-Infinity}', b"{'a':1}",
           b'{"a":"\x01"}', b'{"a":"\\x"}', b'{"a":"\\u12g4"}', b'{"a":"unterminated}', b'{"a":1 "b":2}',
           b'{"a":[1 2]}', b'{"a":1}}', b'{"a":[}]}', b'{"a":{]}}', b'{1:2}', b'{"a":1,"a"}', b'\xef\xbb\xbf{}',
           _deep(64), _deep(65), _deep(65)[:-3] + b'x', b'[' * 64 + b']' * 64, b'[' * 65 + b']' * 65]
    js = [b'{"id":"u1","latitude":52.5,"longitude":13.4,"timestamp":1483250740,"accuracy":5}',
          b'{"id":"u1","latitude":52.5,"longitude":13.4,"timestamp":-5,"accuracy":5}',
          b'{"id":"u1","latitude":52.5,"longitude":13.4,"timestamp":9223372036854775807,"accuracy":5}',
          b'{"id":"u1","latitude":52.5,"longitude":13.4,"timestamp":9223372036854775808,"accuracy":5}',
          b'{"id":"u1","latitude":52.5,"longitude":13.4,"timestamp":1483250740.0,"accuracy":5}',
          b'{"id":"u1","latitude":52.5,"longitude":13.4,"timestamp":1e9,"accuracy":5}',
          b'{"id":"u1","latitude":52.5,"longitude":13.4,"timestamp":"1483250740","accuracy":5}',
          b'{"id":"u1","latitude":52.5,"longitude":13.4,"timestamp":null,"accuracy":5}',
          b'{"id":"u1","latitude":52.5,"longitude":13.4,"accuracy":5}']
    return ([('psv', m) for m in sv] + [('csv', m) for m in csv] + [('json_ymd', m) for m in ymd] +
            [('json', m) for m in js])
