"""Edge cases of the probe ingest (K11, reporter_amd/csrc/otr_ingest.h and Matcher::ingest):
numerals whose path through the number parsers is known, and hand-built texts, each named for
the one edge it is there for.  tests/test_ingest_cases_cpu.py pins what they reach;
tests/test_gpu_ingest_edges.py runs them on the device.  TEST INFRASTRUCTURE ONLY.

The restatement (parse_dec, eisel_lemire, dec_to_double, py2_str_roundtrip below) follows the
device code line by line in Python integers over the table of tools/gen_pow5.entries(), and says
for one numeral which branches it takes (a set of tags) and whether the device code refuses it.
It only classifies: every expected value comes from Python's float() and oracle/ingest.py.

Tags of dec_to_double: zero (w == 0 or q < -342), clinger_mul / clinger_div, clinger_miss (one
step outside Clinger's limits: w == 2^53 + 1, |q| == 23, or a cut digit with |q| <= 22), second
and carry (the second product and its carry into hi), tie_even (the round-to-even line fires: a
binary midpoint over an even neighbour), tie_odd (a midpoint over an odd neighbour: the plain
rounding goes up), subnormal, sub2normal (the subnormal rounding carries into the first normal),
subzero (shifted out whole), mant_carry, inf, inexact_agree / inexact_refuse (more than 19
digits: w and w + 1 give one double, or not), exp_long (an exponent of seven or more digits, or
one beyond 9999 that the value needs in full).  tie_outside is set by the corpus builder, not by
the restatement: w is an odd 54-bit integer (a midpoint between two doubles as an integer) and q
is -6, -5, 24 or 25, where w * 10^q cannot be a midpoint (w * 5^|q| would need more than 54 bits,
or w more than 19 digits), so that the round-to-even line's range test alone keeps them from it.
Tags of py2_str_roundtrip: py2_zero, py2_short, py2_side (with py2_side_lo / py2_side_hi),
py2_exact (with py2_exact_lt / _gt / _eq: the 128-bit comparison decides), py2_refuse.

py2_refuse is reachable with at most 19 digits, in three of its branches: a subnormal v
(py2_refuse_sub), j >= 0 (py2_refuse_j0: a 13-digit integer ending in 5) and -j > 27
(py2_refuse_j27).  Each needs |v| equal to the double of its own 13-digit midpoint.  The other
three (e2 >= 0, sh > 10, -sh > 83) cannot be met once 0 < -j <= 27 holds: the midpoint is below
10^13 < 2^53, and sh = e2 - j stays within [-76, -10] there.  Not covered: eisel_lemire's give-up
line (lo == ~0 outside [-27, 55]); no input is known to reach it.

The separate lists hold 26 numerals, not the 24 first planned: 12 grammar rejects, 8
inexact_refuse, 3 py2_refuse (one per reachable branch) and 3 non-finite (a fourth, '1e400', is
met in the bbox texts and is not given a text of its own).  The plan of 24 counted py2_refuse
as unreachable.
"""
import functools
import math
import random
import struct

from oracle import ingest as oi
from tools import gen_pow5

M64 = (1 << 64) - 1
INF_BITS = 0x7FF << 52
POW5 = list(gen_pow5.entries())
Q_MIN, Q_MAX = -342, 308
SPACE = b' \t\n\x0b\x0c\r'
MAX_CORPUS = 4096


# ---- the restatement -----------------------------------------------------------------------------
def parse_dec(s, tags=None):
    """otr_ingest.h parse_dec over bytes: (neg, w, q, inexact), or None where the grammar fails."""
    tags = set() if tags is None else tags
    s = s.strip(SPACE)
    b, e = 0, len(s)
    neg = False
    if b < e and s[b] in b'+-':
        neg = s[b] == ord('-')
        b += 1
    w = nd = ndig = q = 0
    inexact = False
    while b < e and 48 <= s[b] <= 57:
        c = s[b] - 48
        b += 1
        ndig += 1
        if nd < 19:
            if nd > 0 or c:
                w = w * 10 + c
                nd += 1
        else:
            q += 1
            inexact |= c != 0
    if b < e and s[b] == ord('.'):
        b += 1
        while b < e and 48 <= s[b] <= 57:
            c = s[b] - 48
            b += 1
            ndig += 1
            if nd < 19:
                if nd > 0 or c:
                    w = w * 10 + c
                    nd += 1
                q -= 1
            else:
                inexact |= c != 0
    if ndig == 0:
        return None
    if b < e and s[b] in b'eE':
        b += 1
        eneg = False
        if b < e and s[b] in b'+-':
            eneg = s[b] == ord('-')
            b += 1
        ed = x = 0
        while b < e and 48 <= s[b] <= 57:
            if x < 1000000:
                x = x * 10 + (s[b] - 48)
            b += 1
            ed += 1
        if ed == 0:
            return None
        if ed >= 7 or x >= 10000:
            tags.add('exp_long')
        q += -x if eneg else x
    if b != e:
        return None
    return neg, w, max(-1000000, min(1000000, q)), inexact


def eisel_lemire(w, q, tags):
    """otr_ingest.h eisel_lemire: the bits, or None on its give-up line."""
    if w == 0 or q < Q_MIN:
        tags.add('zero')
        return 0
    if q > Q_MAX:
        tags.add('inf')
        return INF_BITS
    lz = 64 - w.bit_length()
    w <<= lz
    c = POW5[q - Q_MIN]
    p = w * (c >> 64)
    hi, lo = p >> 64, p & M64
    if hi & 0x1FF == 0x1FF:
        tags.add('second')
        hi2 = (w * (c & M64)) >> 64
        lo = (lo + hi2) & M64
        if hi2 > lo:
            hi += 1
            tags.add('carry')
    if lo == M64 and (q < -27 or q > 55):
        tags.add('giveup')
        return None
    upper = hi >> 63
    m = hi >> (upper + 9)
    p2 = (((152170 + 65536) * q) >> 16) + 63 + upper - lz + 1023
    if p2 <= 0:
        if -p2 + 1 >= 64:
            tags.add('subzero')
            return 0
        tags.add('subnormal')
        m >>= -p2 + 1
        m += m & 1
        m >>= 1
        if m >= 1 << 52:
            tags.add('sub2normal')
        return ((0 if m < 1 << 52 else 1) << 52) | (m & ((1 << 52) - 1))
    if lo <= 1 and -4 <= q <= 23 and (m << (upper + 9)) == hi:
        if m & 3 == 1:
            tags.add('tie_even')
            m &= ~1
        elif m & 3 == 3:
            tags.add('tie_odd')
    m += m & 1
    m >>= 1
    if m >= 2 << 52:
        tags.add('mant_carry')
        m = 1 << 52
        p2 += 1
    m &= ~(1 << 52)
    if p2 >= 0x7FF:
        tags.add('inf')
        return INF_BITS
    return (p2 << 52) | m


def _bits(x):
    return struct.unpack('<Q', struct.pack('<d', x))[0]


def _double(b):
    return struct.unpack('<d', struct.pack('<Q', b))[0]


def dec_to_double(d, tags):
    """otr_ingest.h dec_to_double: the bits, or None where the device code refuses."""
    neg, w, q, inexact = d
    sign = (1 << 63) if neg else 0
    if w == 0:
        tags.add('zero')
        return sign
    if not inexact and w <= 1 << 53 and -22 <= q <= 22:
        # one correctly rounded IEEE operation on exact operands, as on the device
        tags.add('clinger_div' if q < 0 else 'clinger_mul')
        x = float(w)
        return _bits(x / float(10 ** -q) if q < 0 else x * float(10 ** q)) | sign
    if (w == (1 << 53) + 1 and -22 <= q <= 22) or (w <= 1 << 53 and abs(q) == 23 and not inexact) or (
            inexact and -22 <= q <= 22):
        tags.add('clinger_miss')
    bits = eisel_lemire(w, q, tags)
    if bits is None:
        return None
    if inexact:
        b2 = eisel_lemire(w + 1, q, set())
        if b2 is None or b2 != bits:
            tags.add('inexact_refuse')
            return None
        tags.add('inexact_agree')
    return bits | sign


def py2_str_roundtrip(d, vbits, tags):
    """otr_ingest.h py2_str_roundtrip of the decimal d whose double has the bits vbits."""
    neg, w, q, inexact = d
    if w == 0:
        tags.add('py2_zero')
        return vbits
    if not inexact:
        while w % 10 == 0:
            w //= 10
            q += 1
    nd = len(str(w))
    if nd <= 12 and not inexact:
        tags.add('py2_short')
        return vbits
    k = nd - 12
    w12 = w // 10 ** k
    mid_w, j = w12 * 10 + 5, q + k - 1
    dm = dec_to_double((False, mid_w, j, False), set())
    if dm is None:
        tags.update(('py2_refuse', 'py2_refuse_mid'))
        return None
    av = vbits & ~(1 << 63)
    if av != dm:
        side = -1 if av < dm else 1   # non-negative doubles order as their bits
        tags.update(('py2_side', 'py2_side_lo' if side < 0 else 'py2_side_hi'))
    else:
        ex = (av >> 52) & 0x7FF
        why = None
        if ex == 0 or ex == 0x7FF:
            why = 'sub'
        m = (av & ((1 << 52) - 1)) | (1 << 52)
        e2 = ex - 1075
        if why is None and j >= 0:
            why = 'j0'
        if why is None and -j > 27:
            why = 'j27'
        if why is None and e2 >= 0:
            why = 'e2'
        sh = e2 - j
        if why is None and sh > 10:
            why = 'sh_hi'
        if why is None and -sh > 83:
            why = 'sh_lo'
        if why:
            tags.update(('py2_refuse', 'py2_refuse_' + why))
            return None
        lhs, rhs = m * 5 ** -j, mid_w
        if sh >= 0:
            lhs <<= sh
        else:
            rhs <<= -sh
        assert lhs < 1 << 128 and rhs < 1 << 128
        side = -1 if lhs < rhs else (1 if lhs > rhs else 0)
        tags.update(('py2_exact', 'py2_exact_' + {-1: 'lt', 1: 'gt', 0: 'eq'}[side]))
    r = w12 if side < 0 else (w12 + 1 if side > 0 else w12 + (w12 & 1))
    return dec_to_double((neg, r, q + k, False), set())


def classify(s):
    """(bits or None-if-refused, tags) of dec_to_double for the numeral s (str); (None, {'reject'})
    where the grammar fails."""
    tags = set()
    d = parse_dec(s.encode('latin-1'), tags)
    if d is None:
        return None, {'reject'}
    return dec_to_double(d, tags), tags


def classify_py2(s):
    """(bits or None-if-refused, tags) of py2_str_roundtrip after dec_to_double."""
    tags = set()
    d = parse_dec(s.encode('latin-1'))
    if d is None:
        return None, {'reject'}
    v = dec_to_double(d, set())
    if v is None:
        return None, {'inexact_refuse'}
    return py2_str_roundtrip(d, v, tags), tags


def digits(s):
    """Significant digits of a numeral (leading zeros not counted, trailing ones are)."""
    t = s.strip().lstrip('+-').lower().split('e')[0].replace('.', '').lstrip('0')
    return len(t)


# ---- numerals --------------------------------------------------------------------------------------
GRAMMAR_ACCEPTED = ['+.5', '1.', '00000.000001', '1E5', '\t12\x0b', '1e0000000005', '1e-9999999', '-1e+0000000',
                    ' 1.5 ', '-0', '5.e-1', '.5E+1']
GRAMMAR_REJECTED = ['1e', '.', 'e5', '1e+', '0x10', '', '--1', '1.2.3', '1_0', 'inf', 'nan', '1e5x']
NON_FINITE = ['1e309', '1.7976931348623159e308', '-123456789e301']
TEXT_NUMERALS = ['1e400']       # non-finite too: met in the bbox texts, not in a text of its own


def _exp_long():
    """Values that need every digit of a long exponent: 10^-10000 scaled back to 1, 100 and 0.01."""
    return ['0.' + '0' * 9999 + '1e10000', '-0.' + '0' * 10001 + '1e10004', '1' + '0' * 11000 + 'e-11002']


def _dec_str(n, q):
    """The integer n times 10^q written without an exponent."""
    s = str(n)
    if q >= 0:
        return s + '0' * q
    s = s.rjust(-q + 1, '0')
    return s[:q] + '.' + s[q:]


def _search(rng, want, draw, limit):
    """Numerals from draw() until every tag in want ({tag: count}) has been met that often."""
    out, have = [], {t: 0 for t in want}
    for _ in range(limit):
        if all(have[t] >= n for t, n in want.items()):
            break
        s = draw(rng)
        _, tags = classify(s)
        hit = [t for t in want if t in tags and have[t] < want[t]]
        if hit:
            out.append(s)
            for t in want:
                have[t] += t in tags
    assert all(have[t] >= n for t, n in want.items()), have
    return out


def _clinger(rng):
    out = []
    for w in ((1 << 53), (1 << 53) - 1, 1, 3, 123456789):
        for q in (22, -22, 0, 1, -1):
            out.append('%de%d' % (w, q))
    for _ in range(30):
        w, q = rng.randrange(1, 1 << 53), rng.randrange(-22, 23)
        out.append('%de%d' % (w, q) if rng.random() < .5 else _dec_str(w, q))
    miss = ['%de%d' % ((1 << 53) + 1, q) for q in (0, 22, -22, 5, -7)]
    miss += ['%de%d' % (w, q) for w in ((1 << 53), (1 << 53) - 1, 7) for q in (23, -23)]
    miss += [_dec_str((1 << 53) - 1, -3) + '0' * 4 + d for d in '139']       # a cut nonzero digit
    miss += ['1.' + '0' * 18 + '7', '25' + '0' * 18 + '.5', '3' + '0' * 18 + '1e-20']
    return out + miss


def _midpoints(rng):
    """Exact binary midpoints of at most 19 digits with q in [-4, 23] that Clinger's path does not
    take (w > 2^53, or q == 23), over even and odd neighbours; and the tie_outside numerals."""
    out = ['9007199254740993', '9007199254740995', '1e23', '9e22', '8e23', '4503599627370496e23']
    for q in range(0, 23):      # odd * 5^q is an odd integer of 54 bits; w = odd * 2^a
        lo, hi = -(-(1 << 53) // 5 ** q), ((1 << 54) - 1) // 5 ** q
        for want in (1, 3):
            for _ in range(400):
                odd = rng.randrange(lo, hi + 1) | 1
                a = max(0, 54 - odd.bit_length()) + rng.randrange(0, 4)
                if lo <= odd <= hi and (odd * 5 ** q) & 3 == want and odd << a < 10 ** 19:
                    out.append('%de%d' % (odd << a, q))
                    break
    for j in range(1, 5):       # (2 M + 1) / 2^j: j decimal places
        for want in (1, 3):
            mid = ((rng.randrange(1 << 52, (1 << 53) - 1) << 1) | 1) & ~3 | want
            if mid * 5 ** j < 10 ** 19:
                out.append(_dec_str(mid * 5 ** j, -j))
    outside = []
    for q in (-6, -5, 24, 25):
        for want in (1, 3):
            mid = ((rng.randrange(1 << 52, 1 << 53) << 1) | 1) & ~3 | want
            outside.append('%de%d' % (mid, q))
    return out, outside


def _small(rng):
    out = ['5e-324', '4e-320', '2.4703282292062328e-324', '2.47e-324', '2.2250738585072011e-308',
           '2.2250738585072014e-308', '2.225073858507201e-308', '1e-342', '9e-342', '1234e-345', '1e-343', '1e-400',
           '0e999', '-0.0', '0', '-0e-999', '0.000', '4.9406564584124654e-324', '2.2250738585072009e-308',
           '2.2250738585072012e-308']
    out += _search(rng, {'subnormal': 40}, lambda r: '%de%d' % (r.randrange(1, 10 ** r.randrange(1, 20)),
                                                                  r.randrange(-342, -305)), 4000)
    out += _search(rng, {'sub2normal': 3}, lambda r: '2.2250738585072%04de-308' % r.randrange(10000), 4000)
    return out


def _big(rng):
    out = ['9007199254740991.5', '18014398509481983', '4503599627370495.75', '1.7976931348623157e308',
           '1.7976931348623158e308', '179769313486231570e291', '36028797018963967', '72057594037927935e3']
    for k in range(4):          # 2^(54+k) - 1 and neighbours: the rounding carries out of the mantissa
        out.append(str((1 << (54 + 3 * k)) - 1))
    return out


def _draw_19(rng):
    return '%de%d' % (rng.randrange(10 ** 18, 10 ** 19), rng.randrange(-345, 292))


def _long_digits(rng):
    """20 to 60 significant digits."""
    out = ['52.123456789012345678901', '1.00000000000000000000001', '0.1000000000000000055511151231257827',
           '123456789012345678901234567890', '3.14159265358979323846264338327950288419716939937510582097494']
    for _ in range(80):
        n = rng.randrange(20, 61)
        ds = str(rng.randrange(1, 10)) + ''.join(rng.choice('0123456789') for _ in range(n - 2))
        ds += str(rng.randrange(1, 10))
        p = rng.randrange(0, n)
        s = ds[:p] + '.' + ds[p:]
        if rng.random() < .4:
            s += 'e%d' % rng.randrange(-300, 280)
        out.append(rng.choice(['', '-']) + s)
    return out


def _refused():
    """Decimals of a binary midpoint cut after the 19th digit: w below, w + 1 above the midpoint."""
    from fractions import Fraction
    out = ['9007199254740993.00000000000000000001']
    for m, e in ((1 << 53) + 1, -53), ((1 << 53) + 3, -53), ((1 << 53) + 12345, -60), ((3 << 52) + 1, -40), (
            (1 << 53) + 7, -12), ((1 << 54) - 1, -57), ((1 << 53) + 99, -100):
        x = Fraction(m) * Fraction(2) ** e     # an odd 54-bit integer times 2^e: a midpoint
        n, q = x.numerator * 10 ** 80 // x.denominator, -80   # exact: the denominator is a power of two <= 2^100
        if e < -80:
            n, q = x.numerator * 10 ** 120 // x.denominator, -120
        out.append(_dec_str(n, q).rstrip('0'))
    assert all(classify(s)[0] is None and digits(s) > 19 for s in out)
    return out


def _py2(rng):
    short = ['1.5', '-0.25', '180', '123456789012', '1234567890.12', '1.23456789012e-5', '1200000000000000',
             '0.000000000001', '-99999999999.9', '5e-324', '1e22', '12345678901200000e5', '7', '0.1', '-179.999999999',
             '1e300']
    side = []
    for _ in range(40):
        side.append(repr(rng.uniform(-180, 180)))
        side.append('%.17g' % (rng.uniform(-1, 1) * 10 ** rng.randrange(-8, 8)))
    exact = []
    for _ in range(12):
        w = rng.randrange(10 ** 11, 10 ** 12)
        for tail in ('5', '49999', '50001', '4999999', '5000000'):
            s = str(w) + tail
            exact.append(rng.choice(['', '-']) + s[:2] + '.' + s[2:])
    # exact ties: 13 digits ending in 5 that are dyadic, over an even and an odd 12th digit
    exact += ['123456789012.5', '123456789013.5', '-12345678901.25', '12345678902.75', '1234567890.125',
              '1.5000000000005e0', '99999999999.95e1', '0.5000000000005']
    exact += ['%s.%s5' % (w[:3], w[3:]) for w in (str(rng.randrange(10 ** 11, 10 ** 12)) for _ in range(24))]
    return short, side, exact


PY2_REFUSED = ['2.000000000005e-310', '1234567890125', '1.234567890125e-20']


@functools.lru_cache(maxsize=None)
def numerals():
    """{'main': [...], 'refused': [...], 'py2_refused': [...], 'rejected': [...], 'non_finite': [...],
    'tie_outside': [...]} of str.  main: accepted, finite, refused by no rule set; at most 4096."""
    rng = random.Random(20)
    mid, outside = _midpoints(rng)
    short, side, exact = _py2(rng)
    main = list(GRAMMAR_ACCEPTED) + _exp_long() + _clinger(rng) + mid + outside + _small(rng) + _big(rng)
    main += _search(rng, {'second': 40, 'carry': 10}, _draw_19, 200000)
    main += _long_digits(rng) + short + side + exact
    for _ in range(400):        # the generator's own forms and doubles of every magnitude
        main.append(repr(rng.uniform(-180, 180)))
        main.append('%.*f' % (rng.randrange(0, 16), rng.uniform(-180, 180)))
        main.append(repr(_double(rng.getrandbits(64) & ~(0x7FF << 52) | (rng.randrange(1, 0x7FF) << 52))))
        main.append('%de%d' % (rng.getrandbits(rng.randrange(1, 64)), rng.randrange(-40, 40)))
    seen, out = set(), []
    for s in main:
        if s in seen:
            continue
        seen.add(s)
        b1, t1 = classify(s)
        b2, t2 = classify_py2(s)
        if b1 is None or b2 is None or 'inf' in t1 or math.isinf(_double(b1)):
            continue            # kept out: the pin checks that none of these is in main
        out.append(s)
    assert len(out) <= MAX_CORPUS
    return {'main': out, 'refused': _refused(), 'py2_refused': list(PY2_REFUSED), 'rejected': list(GRAMMAR_REJECTED),
            'non_finite': list(NON_FINITE), 'in_texts': list(TEXT_NUMERALS), 'tie_outside': outside}


def tag_counts(which=('main', 'refused', 'py2_refused', 'non_finite', 'in_texts')):
    """{tag: how many numerals of the lists carry it} (tie_outside from its own list)."""
    n = numerals()
    out = {}
    for name in which:
        for s in n[name]:
            for t in classify(s)[1] | classify_py2(s)[1]:
                out[t] = out.get(t, 0) + 1
    out['tie_outside'] = sum(1 for s in n['tie_outside'] if s in n['main'])
    return out


REQUIRED = {'clinger_mul': 32, 'clinger_div': 32, 'clinger_miss': 16, 'second': 32, 'carry': 8, 'tie_even': 16,
            'tie_odd': 8, 'tie_outside': 8, 'subnormal': 32, 'sub2normal': 2, 'subzero': 2, 'zero': 4,
            'mant_carry': 4, 'inf': 4, 'inexact_agree': 64, 'inexact_refuse': 8, 'exp_long': 4, 'py2_short': 16,
            'py2_side': 64, 'py2_side_lo': 8, 'py2_side_hi': 8, 'py2_exact': 16, 'py2_exact_lt': 2,
            'py2_exact_gt': 2, 'py2_exact_eq': 2, 'py2_refuse': 2, 'py2_refuse_sub': 1, 'py2_refuse_j0': 1,
            'py2_refuse_j27': 1}
UNREACHED = ('giveup', 'py2_refuse_mid', 'py2_refuse_e2', 'py2_refuse_sh_hi', 'py2_refuse_sh_lo')


# ---- texts -----------------------------------------------------------------------------------------
SHARD, RAW, JAVA = 'shard', 'raw', 'java'
EPOCH, YMDHMS = 'epoch', 'ymdhms'
DEFAULT_IDX = (1, 0, 9, 10, 5)      # uuid, time, lat, lon, accuracy


class Case:
    """One text and how it is ingested.  idx: (uuid, time, lat, lon, accuracy) field positions;
    refusal: (line, 'precision') where only the device code refuses (the oracle accepts)."""

    def __init__(self, name, text, rules=SHARD, inactivity=120, idx=DEFAULT_IDX, sep='|', bbox=None,
                 time_format=None, refusal=None):
        self.name, self.text, self.rules, self.inactivity = name, text, rules, inactivity
        self.idx, self.sep, self.bbox, self.refusal = tuple(idx), sep, bbox, refusal
        self.time_format = time_format or (EPOCH if rules == SHARD else YMDHMS)

    def records(self):
        """The oracle's kept points in line order (raises oi.IngestError)."""
        sep = self.sep if isinstance(self.sep, str) else chr(self.sep)
        if self.rules == SHARD:
            return oi.shard_records(self.text)
        if self.rules == RAW:
            return oi.shard_records(oi.raw_to_shard_text(self.text, idx=self.idx, sep=sep, bbox=self.bbox,
                                                         time_format=self.time_format))
        return oi.java_sv_records(self.text, idx=self.idx, sep=sep, time_format=self.time_format)

    def expected(self):
        """{'error': 'line N: reason'} or {'windows', 'soa', 'n_lines', 'n_kept', 'n_uuids', 'n_traces',
        'n_probes'} from oracle/ingest.py (and the device-only refusal where the case names one)."""
        try:
            recs = self.records()
        except oi.IngestError as e:
            assert self.refusal is None
            return {'error': str(e), 'line': e.line, 'reason': e.reason}
        if self.refusal is not None:
            return {'error': 'line %d: %s' % self.refusal, 'line': self.refusal[0], 'reason': self.refusal[1]}
        win = oi.group_windows(recs, self.inactivity)
        return {'windows': win, 'soa': oi.to_soa(win), 'n_lines': len(oi._lines(self.text)), 'n_kept': len(recs),
                'n_uuids': len({u for u, _ in recs}), 'n_traces': len(win), 'n_probes': sum(len(p) for _, p in win)}

    def ingest_kw(self):
        """Keyword arguments of Matcher.ingest (the constants of reporter_amd/_lib.py by value)."""
        kw = {'rules': {SHARD: 0, RAW: 1, JAVA: 2}[self.rules], 'inactivity': self.inactivity}
        if self.rules != SHARD:
            u, t, la, lo, a = self.idx
            kw.update(separator=self.sep, uuid_index=u, time_index=t, lat_index=la, lon_index=lo, accuracy_index=a,
                      time_format={EPOCH: 0, YMDHMS: 1}[self.time_format])
            if self.bbox is not None:
                kw['bbox'] = list(self.bbox)
        return kw


def shard_line(uuid, t, lat='1.5', lon='2.5', acc='5'):
    return ('%s,%s,%s,%s,%s' % (uuid, t, lat, lon, acc)).encode('latin-1')


def raw_line(uuid, t, lat='1.5', lon='2.5', acc='5', sep='|'):
    """The default valuer's layout: time, uuid, ..., accuracy at 5, ..., lat at 9, lon at 10."""
    f = [''] * 11
    f[0], f[1], f[5], f[9], f[10] = str(t), uuid, acc, lat, lon
    return sep.join(f).encode('latin-1')


def _join(lines, final_newline=True):
    return b'\n'.join(lines) + (b'\n' if final_newline else b'')


def newline_lanes():
    """SHARD lines padded with blanks so that '\\n' falls on byte 0, 1, ..., 15 of a 16-byte chunk,
    then on byte 15 twice more (a line that starts on byte 0 after a newline on byte 15), then 10-byte
    lines (two newlines in one chunk); every third line is 32 bytes longer (chunks of no newline)."""
    out, pos = [], 0
    for i, k in enumerate(list(range(16)) + [15, 15, 10, 5, 0, 11]):
        line = shard_line('ab'[i % 2], 10 * i, '%d.25' % i) if i < 18 else shard_line('ab'[i % 2], i, '1', '2', '5')
        line += b' ' * ((k - (pos + len(line))) % 16 + (32 if i < 18 and i % 3 == 0 else 0))
        out.append(line)
        pos += len(line) + 1
    return _join(out)


def nl_positions(text):
    return [i for i, c in enumerate(text) if c == 10]


def _padded(n_bytes, final_newline):
    """Three SHARD lines in exactly n_bytes bytes."""
    lines = [shard_line('u', 5), shard_line('u', 6, '1.75'), shard_line('v', 7)]
    text = _join(lines, final_newline)
    lines[1] += b' ' * (n_bytes - len(text))
    text = _join(lines, final_newline)
    assert len(text) == n_bytes
    return text


UUID300 = ''.join(chr(33 + (7 * i) % 90) for i in range(300)).replace(',', ';').replace('|', '/')


def _n_lines(n):
    """n SHARD lines over 7 uuids, times out of order: every uuid's window crosses block edges."""
    return _join([shard_line('u%d' % (i % 7), (i * 37) % n, '%d.5' % (i % 90), '%d.125' % (i % 180), str(i % 9))
                  for i in range(n)], final_newline=n % 2 == 0)


def _groups_text():
    uu = ['a', 'aa', 'a ', 'A', '', UUID300]
    lines = []
    for i in range(30):         # interleaved, first appearance: aa, A, a, '', 'a ', the long one
        u = ['aa', 'A', 'a', '', 'a ', UUID300][i % 6]
        lines.append(shard_line(u, 100 - i, '%d.5' % i))          # times descending in the file
    for i in range(12):         # equal times in file order, a distinct latitude each
        lines.append(shard_line(uu[i % 3], 100 - (i % 3), '%d.25' % (40 + i)))
    lines += [shard_line('neg', t) for t in (-5, -300, -7, -301, 3)]
    lines += [shard_line('z', t) for t in (9223372036854775807, -9223372036854775808, -9223372036854775807,
                                            9223372036854775806)]
    return _join(lines)


def _window_texts():
    def text(times_by_uuid):
        return _join([shard_line(u, t, '%d.5' % i) for u, ts in times_by_uuid for i, t in enumerate(ts)])
    lone = [('s', [0, 1000, 1001]), ('m', [0, 1, 500, 1000, 1001]), ('e', [0, 1, 1000]), ('none', [0, 1000, 2000]),
            ('k', [7, 8])]
    return [Case('gap_at_limit', text([('a', [10, 130, 250]), ('b', [10, 11, 132, 133])])),
            Case('gap_at_limit_0', text([('a', [5, 5, 5, 6, 6, 8, 9, 9])]), inactivity=0),
            Case('lone_windows', text(lone)),
            Case('all_dropped', text([('a', [0, 1000, 2000]), ('b', [5]), ('c', [1, 500])])),
            Case('last_kept', text([('a', [0, 1000]), ('b', [5, 6])])),
            Case('last_dropped', text([('a', [0, 1]), ('b', [5, 6, 1000])]))]


BBOX = (10.5, 20.25, 30.75, 40.125)


def _bbox_texts():
    below, above = repr(math.nextafter(10.5, 0.0)), repr(math.nextafter(40.125, 100.0))
    t = '2017-01-01 06:05:%02d'
    lines = [raw_line('u', t % 1, '10.5', '20.25'), raw_line('u', t % 2, '30.75', '40.125'),
             raw_line('u', t % 3, below, '30'), raw_line('u', t % 4, '20', above),
             raw_line('u', 'no time', '50', '30', 'no accuracy'), raw_line('u', t % 5, '1e400', '30'),
             raw_line('u', t % 6, '20.000000000000004', '30.123456789012345'),
             raw_line('u', '0000-00-00', '20', '-1e400', 'x')]
    bad_lat = lines[:4] + [raw_line('u', t % 7, 'north', '30')]
    return [Case('bbox_edges', _join(lines), RAW, bbox=BBOX),
            Case('bbox_bad_latitude', _join(bad_lat), RAW, bbox=BBOX),
            Case('bbox_none_overflow', _join(lines[:2] + lines[5:6]), RAW)]


def _accuracy_texts():
    def raw(accs, rules=RAW):
        return Case('x', _join([raw_line('u', i, acc=a) for i, a in enumerate(accs)]), rules, time_format=EPOCH)
    out = [Case('shard_acc_kept', _join([shard_line('u', i, acc=a) for i, a in enumerate(
        ('16777216', '-16777216', '0', '-0', '+7', ' 12 '))])),
           Case('shard_acc_over', _join([shard_line('u', 0), shard_line('u', 1, acc='16777217')])),
           Case('shard_acc_under', _join([shard_line('u', 0), shard_line('u', 1, acc='-16777217')])),
           Case('shard_acc_2_63', _join([shard_line('u', 0), shard_line('u', 1, acc='9223372036854775808')]))]
    named = [('raw_acc_kept', raw(['-0.5', '999.1', '1000.0000001', '1e300', '-16777216.5', '999.0', '1000', '1e-320',
                                   '-1e-320', '16777217.5', '9' * 25])),
             ('raw_acc_under', raw(['1', '-16777217.5'])), ('raw_acc_inf', raw(['1', '2', 'inf'])),
             ('raw_acc_overflow', raw(['1', '1e999'])),
             ('java_acc_kept', raw(['16777216.5', '-16777216.5', '-0.5', '6.5', '16777215.5', '1e-50'], JAVA)),
             ('java_acc_over', raw(['1', '16777217.5'], JAVA)), ('java_acc_3e9', raw(['1', '3e9'], JAVA)),
             ('java_acc_minus_3e9', raw(['-3e9', '1'], JAVA))]
    for name, c in named:
        c.name = name
        out.append(c)
    return out


def _time_texts():
    ok = ['2017x01y01z06q05r40', '2017-01-01 06:05:41 and more', '2017-01-00 06:05:40', '2017-01-45 06:05:40',
          '2017-01-01 99:05:40', '2017-01--5 06:05:40', '2017-01- 5 06:05:40', '2017-01-01 06:05:4 ',
          '2017-01-01 06:05:4',
          '+017-01-01 06:-5:40', '9999-12-31 23:59:59', '0001-01-01 00:00:00', '9999-12-31 23:59:58']
    out = [Case('ymdhms_accepted', _join([raw_line('u', t, '%d.5' % i) for i, t in enumerate(ok)]), RAW,
                inactivity=(1 << 31) - 1),
           Case('ymdhms_accepted_java', _join([raw_line('u', t, '%d.5' % i) for i, t in enumerate(ok)]), JAVA,
                inactivity=(1 << 31) - 1)]
    for name, t in (('ymdhms_17_bytes', '2017-01-01 06:05:'), ('ymdhms_10_bytes', '2017-01-01'),
                    ('ymdhms_year_0', '0000-01-01 06:05:40'),
                    ('ymdhms_month_13', '2017-13-01 06:05:40'), ('ymdhms_empty', '')):
        out.append(Case(name, _join([raw_line('u', ok[0]), raw_line('u', t)]), RAW))
    ep = [' 12 ', '+5', '-3', '0012']
    out.append(Case('epoch_raw_blanks', _join([raw_line('u', t) for t in ep]), RAW, time_format=EPOCH))
    out.append(Case('epoch_java_blanks', _join([raw_line('u', t) for t in ep[1:] + ep[:1]]), JAVA, time_format=EPOCH))
    out.append(Case('epoch_java_plus', _join([raw_line('u', t) for t in ep[1:]]), JAVA, time_format=EPOCH))
    for rules in (RAW, JAVA):
        out.append(Case('epoch_%s_2_63' % rules, _join([raw_line('u', '9223372036854775807'),
                                                        raw_line('u', '9223372036854775808')]), rules,
                        time_format=EPOCH))
    return out


def _field_texts():
    out = [Case('shard_4_fields', _join([shard_line('u', 1), b'u,2,1.5,2.5'])),
           Case('shard_6_fields', _join([shard_line('u', 1), b'u,2,1.5,2.5,5,'])),
           Case('shard_blanks', b' \ta, 1 ,\t1.5 , 2.5\x0b,\x0c5 \r\n\x0ba,\t2\t,+1.75,\t-2.5e0 , -0 \n'
                                b'  b ,3,1,2,3\n b ,+4,1,2,3  ')]
    idx = (3, 4, 0, 2, 1)       # out of order: lat, acc, lon, uuid, time
    def line(u, t, sep, la='1.5', lo='2.5', a='5', tail=()):
        return sep.join([la, a, lo, u, str(t)] + list(tail)).encode('latin-1')
    for rules in (RAW, JAVA):
        for sep in (';', 9):
            s = sep if isinstance(sep, str) else chr(sep)
            out.append(Case('%s_idx_sep_%s' % (rules, ord(s)),
                            _join([line('u', 5, s), line('v', 6, s, tail=['x', '']), line('u', 7, s), line('v', 8, s)]),
                            rules, idx=idx, sep=sep, time_format=EPOCH))
        wide = ['f'] * 41
        def wl(u, t):
            f = list(wide)
            f[40], f[0], f[1], f[2], f[3] = u, str(t), '1.5', '2.5', '5'
            return '|'.join(f).encode('latin-1')
        out.append(Case('%s_uuid_index_40' % rules, _join([wl('u', 1), wl('w', 2), wl('u', 3), wl('w', 4)]), rules,
                        idx=(40, 0, 1, 2, 3), time_format=EPOCH))
        out.append(Case('%s_index_at_count' % rules, _join([wl('u', 1), b'|'.join([b'f'] * 40)]), rules,
                        idx=(40, 0, 1, 2, 3), time_format=EPOCH))
        # trailing empty fields with a wanted index among them: the uuid (RAW accepts), the accuracy
        out.append(Case('%s_trailing_uuid' % rules, b'1|1.5|2.5|5||\n2|1.5|2.5|5||\n', rules, idx=(4, 0, 1, 2, 3),
                        time_format=EPOCH))
        out.append(Case('%s_trailing_accuracy' % rules, b'u|1|1.5|2.5|7\nu|2|1.5|2.5||\n', rules, idx=(0, 1, 2, 3, 4),
                        time_format=EPOCH))
    return out


def _error_texts():
    good = shard_line('u', 1)
    long_digits = numerals()['refused'][1]
    out = [Case('reason_fields', _join([good, b'u,2'])), Case('reason_float', _join([good, shard_line('u', 2, 'x')])),
           Case('reason_int', _join([good, shard_line('u', '2.0')])),
           Case('reason_time', _join([raw_line('u', '2017-00-01 00:00:00')]), RAW),
           Case('reason_accuracy', _join([raw_line('u', 1, acc='north')]), RAW, time_format=EPOCH),
           Case('reason_uuid', _join([raw_line('u', 1), raw_line(' \tu,v', 2)]), RAW, time_format=EPOCH),
           Case('reason_precision', _join([good, good, shard_line('u', 3, lon=long_digits)]), refusal=(2, 'precision')),
           Case('reason_precision_py2', _join([raw_line('u', 1), raw_line('u', 2, PY2_REFUSED[1])]), RAW,
                time_format=EPOCH, refusal=(1, 'precision')),
           Case('newline_only', b'\n'), Case('raw_newline_only', b'\n', RAW), Case('java_newline_only', b'\n', JAVA)]
    lines = [shard_line('u%d' % (i % 5), i) for i in range(800)]
    lines[700] = shard_line('u', 700, 'x')
    lines[3] = shard_line('u', '3.5')
    out.append(Case('lowest_bad_line', _join(lines)))
    lines = [shard_line('u%d' % (i % 5), i) for i in range(800)]
    lines[511] = shard_line('u', 511, acc='16777217')     # the lower line wins over the lower reason code
    lines[512] = b'u,512'
    out.append(Case('lowest_bad_line_not_reason', _join(lines)))
    out.append(Case('first_reason_float', _join([shard_line('u', 'x', 'north', '2.5', 'y')])))
    out.append(Case('first_reason_float_raw', _join([raw_line('u,v', 'x', '1.5', 'east', 'y')]), RAW))
    out.append(Case('first_reason_float_java', _join([raw_line('u', 'x', '1.5', 'east', 'y')]), JAVA))
    out.append(Case('accuracy_before_uuid', _join([raw_line('u,v', 1, acc='y')]), RAW, time_format=EPOCH))
    out.append(Case('time_before_accuracy', _join([raw_line('u,v', 'x', acc='y')]), RAW, time_format=EPOCH))
    return out


def _chunk_texts():
    out = [Case('newline_lanes', newline_lanes())]
    for r in (0, 1, 15):
        for final in (True, False):
            out.append(Case('len_%d_%s' % (r, 'nl' if final else 'open'), _padded(64 + r, final)))
    crlf = b'\r\n'.join([shard_line('u', 1), shard_line('v', 2), shard_line('u', 3), shard_line('v', 4)]) + b'\r\n'
    out.append(Case('crlf', crlf))
    out.append(Case('crlf_raw', b'\r\n'.join([raw_line('u', i, lon='2.5') for i in range(4)]) + b'\r\n', RAW,
                    time_format=EPOCH))
    out.append(Case('uuid_300', _join([shard_line(UUID300, 1), shard_line(UUID300[:299], 2), shard_line(UUID300, 3),
                                       shard_line(UUID300[:299], 4)])))
    for n in (1, 2, 255, 256, 257, 513):
        out.append(Case('lines_%d' % n, _n_lines(n)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """Every hand-built text, by name."""
    out = _chunk_texts() + [Case('groups', _groups_text())] + _window_texts() + _field_texts() + _bbox_texts()
    out += _accuracy_texts() + _time_texts() + _error_texts()
    names = [c.name for c in out]
    assert len(set(names)) == len(names), names
    return {c.name: c for c in out}


def reuse_sequence():
    """[(case, fresh)]: ingests for ONE matcher, in this order.  A long accepted text with '\\n' on
    the one padding byte of the short text's last chunk, the short text; a long rejected text
    with '\\n' on every padding byte of a second short text's last chunk, that short text."""
    short1 = _padded(64 + 15, False)
    lines = [shard_line('w', i, '%d.5' % i) for i in range(40)]
    lines[3] += b' ' * (79 - len(_join(lines[:4], False)))
    long1 = _join(lines)
    assert long1[79:80] == b'\n' and len(long1) > 400
    short2 = _padded(48 + 3, False)
    long2 = long1[:51] + b'\n' * 13 + long1[64:]
    return [Case('reuse_long', long1), Case('reuse_short', short1), Case('reuse_long_rejected', long2),
            Case('reuse_short_after_reject', short2)]


# ---- the numeral texts of the GPU test ---------------------------------------------------------------
def corpus_case(rules, nums, uuids=1, seed=None, field='coord'):
    """The numerals as the latitude of one line and the longitude of the next (field='coord'), or
    as the accuracy, under times rising by 1; over several uuids the lines are shuffled."""
    n = len(nums)
    order = list(range(n))
    if seed is not None:
        random.Random(seed).shuffle(order)
    lines = []
    for k, i in enumerate(order):
        u = 'u%d' % (i % uuids)
        if field == 'coord':
            la, lo, a = nums[i], nums[i - 1], '5'
        else:
            la, lo, a = '1.5', '2.5', nums[i]
        lines.append(shard_line(u, i, la, lo, a) if rules == SHARD else raw_line(u, i, la, lo, a))
    return Case('corpus_%s_%s' % (rules, field), _join(lines), rules, time_format=EPOCH, inactivity=n)


def accuracy_numerals(rules):
    """The main corpus numerals that the oracle accepts as an accuracy under the rule set."""
    out = []
    for s in numerals()['main']:
        try:
            Case('x', raw_line('u', 1, acc=s), rules, time_format=EPOCH).records()
            out.append(s)
        except oi.IngestError:
            pass
    return out


def single_numeral_case(s, rules=SHARD):
    """A text of its own for a numeral that ends the ingest: two good lines, then the numeral as
    latitude."""
    mk = shard_line if rules == SHARD else raw_line
    return Case('numeral', _join([mk('u', 1), mk('u', 2), mk('u', 3, s)]), rules, time_format=EPOCH)
