// otr_formatter.h — K16: the streaming reporter's first stage, raw messages → keyed points
// in HBM (include/otr.h otr_format_messages).  What
// KeyedFormattingProcessor.java:32-43 does with Formatter.formatSV / formatJSON
// (Formatter.java:97-124): every message becomes a point, or is dropped (the reference
// certainly throws), or is unsupported (the reference might produce a point that cannot be
// reproduced without a JVM: counted apart, never approximated).
//
// One thread per message, K11's shape.  A JSON message is a sequential state machine over
// ~100 bytes (string / escape state, nesting, member boundaries); a wave-cooperative scan
// would have to carry that state through prefix operations over 64 bytes at a time for
// messages barely longer than one such step, while the lanes of a one-thread-per-message
// wave run the same byte loop over messages of much the same length, so they diverge only
// at the field rules.  Neighbouring lanes read lines ~100 bytes apart: every 64-byte line
// they fetch is consumed whole by the following iterations out of the vector L1.
//
// The per-message functions are __host__ __device__ so that tests/ can compare them on the
// CPU with the restatement tests/formatter_ref.py (tools/libformatcheck.so, test
// infrastructure only).  The number parsers are K11's (otr_ingest.h), shared, not copied.
#pragma once
#include "otr_ingest.h"

namespace otr {

// the order of K11's IngestFmt::idx
enum { FM_UUID = 0, FM_TIME = 1, FM_LAT = 2, FM_LON = 3, FM_ACC = 4 };

struct MsgFmt {
  int type, sep, tfmt;
  int idx[5];           // SV field positions
  int klen[5];          // JSON key lengths
  const uint8_t* keys;  // JSON: 5 keys of 64 bytes each
};

struct MsgPoint {
  uint64_t hash;
  int64_t uoff, time;
  int32_t ulen, acc;
  float lat, lon;
};

// A field's verdict: 0, or a reason.  Over a message any dropped reason (the reference
// certainly throws) beats any unsupported one; within a class the first in the reference's
// evaluation order (lat, lon, time, accuracy, uuid) is reported.
struct Verdict {
  int drop, unsup;
  OTR_HD void add(int r) {
    if (r == 0) return;
    if (r < OTR_FORMAT_UNSUPPORTED) {
      if (!drop) drop = r;
    } else if (!unsup) {
      unsup = r;
    }
  }
  OTR_HD int reason() const { return drop ? drop : unsup; }
};

// floatFormatter.parse(text).floatValue() under K11's JAVA_SV reading: Python's float()
// grammar, the double nearest the decimal, narrowed to float
OTR_HD int fm_coord_text(const uint8_t* s, int64_t b, int64_t e, float& out) {
  Dec d;
  double v = 0;
  if (!parse_dec(s, b, e, d)) return OTR_FORMAT_D_FLOAT;
  if (!dec_to_double(d, v)) return OTR_FORMAT_U_PRECISION;
  if (!(v - v == 0.0)) return OTR_FORMAT_D_FLOAT;
  out = (float)v;
  return 0;
}

// (int)Math.ceil(x): the saturating cast, then K11's bound of ±2^24
OTR_HD int fm_ceil_acc(double x, int32_t& out) {
  const double c = ceil(x);
  const int64_t a = !(c == c) ? 0 : (c >= 2147483647.0 ? 2147483647 : (c <= -2147483648.0 ? -2147483647 - 1 : (int64_t)c));
  if (!(c == c) || a > 16777216 || a < -16777216) return OTR_FORMAT_U_ACCURACY;
  out = (int32_t)a;
  return 0;
}

OTR_HD int fm_time_text(const uint8_t* s, int64_t b, int64_t e, int64_t& t) {
  const int r = parse_ymdhms(s, b, e, t);
  return r == 0 ? 0 : (r == OTR_INGEST_E_INT ? OTR_FORMAT_D_INT : OTR_FORMAT_D_TIME);
}

// Formatter.formatSV (Formatter.java:97-109) under K11's OTR_INGEST_JAVA_SV rules
OTR_HD int format_sv(const uint8_t* s, int64_t b, int64_t e, const MsgFmt& f, MsgPoint& p) {
  int64_t fb[5] = {0, 0, 0, 0, 0}, fe[5] = {0, 0, 0, 0, 0};
  bool have[5] = {false, false, false, false, false};
  const uint8_t sep = (uint8_t)f.sep;
  int nf = 0, last_nonempty = -1;
  int64_t st = b;
  for (int64_t q = b; q <= e; ++q) {
    if (q == e || s[q] == sep) {
#pragma unroll
      for (int k = 0; k < 5; ++k)
        if (f.idx[k] == nf) {
          fb[k] = st;
          fe[k] = q;
          have[k] = true;
        }
      if (q > st) last_nonempty = nf;
      ++nf;
      st = q + 1;
    }
  }
  bool ok = true;  // String.split drops the trailing empty fields before indexing
#pragma unroll
  for (int k = 0; k < 5; ++k) ok = ok && have[k] && f.idx[k] <= last_nonempty;
  if (!ok) return OTR_FORMAT_D_FIELDS;
  Verdict v{0, 0};
  v.add(fm_coord_text(s, fb[FM_LAT], fe[FM_LAT], p.lat));
  v.add(fm_coord_text(s, fb[FM_LON], fe[FM_LON], p.lon));
  if (f.tfmt == OTR_TIME_YMDHMS) v.add(fm_time_text(s, fb[FM_TIME], fe[FM_TIME], p.time));
  else if (!parse_int(s, fb[FM_TIME], fe[FM_TIME], p.time, true)) v.add(OTR_FORMAT_D_INT);
  {
    Dec d;
    double av = 0;
    if (!parse_dec(s, fb[FM_ACC], fe[FM_ACC], d)) v.add(OTR_FORMAT_D_ACCURACY);
    else if (!dec_to_double(d, av)) v.add(OTR_FORMAT_U_PRECISION);
    else v.add(fm_ceil_acc((double)(float)av, p.acc));  // through float: floatValue()
  }
  p.uoff = fb[FM_UUID];
  p.ulen = (int32_t)(fe[FM_UUID] - fb[FM_UUID]);
  p.hash = uuid_hash(s, fb[FM_UUID], fe[FM_UUID]);
  if (p.hash == OTR_NO_ID) v.add(OTR_FORMAT_U_NO_ID);
  return v.reason();
}

// ---- JSON ---------------------------------------------------------------------------------
enum { JV_NONE = 0, JV_STRING, JV_NUMBER, JV_LITERAL, JV_CONTAINER };
enum { JF_INT = 1, JF_EXP = 2, JF_ESCAPE = 4 };  // number: no fraction and no exponent / an exponent; string: a backslash

OTR_HD bool json_ws(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
OTR_HD bool json_hex(uint8_t c) {
  return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F');
}

// s[q] == '"': the string's closing quote position, or -1 (RFC 8259 §7; bytes >= 0x80 pass)
OTR_HD int64_t json_string(const uint8_t* s, int64_t q, int64_t e, bool& escape) {
  escape = false;
  for (++q; q < e; ++q) {
    const uint8_t c = s[q];
    if (c == '"') return q;
    if (c < 0x20) return -1;
    if (c == '\\') {
      escape = true;
      if (++q >= e) return -1;
      const uint8_t x = s[q];
      if (x == 'u') {
        if (q + 4 >= e || !json_hex(s[q + 1]) || !json_hex(s[q + 2]) || !json_hex(s[q + 3]) || !json_hex(s[q + 4]))
          return -1;
        q += 4;
      } else if (!(x == '"' || x == '\\' || x == '/' || x == 'b' || x == 'f' || x == 'n' || x == 'r' || x == 't')) {
        return -1;
      }
    }
  }
  return -1;
}

// a number token at q (RFC 8259 §6): the end of its longest valid prefix ("1e" and "1."
// end after the 1, and what follows decides), or -1
OTR_HD int64_t json_number(const uint8_t* s, int64_t q, int64_t e, int& flags) {
  flags = JF_INT;
  if (q < e && s[q] == '-') ++q;
  if (q >= e || s[q] < '0' || s[q] > '9') return -1;
  if (s[q] == '0') ++q;
  else
    while (q < e && s[q] >= '0' && s[q] <= '9') ++q;
  if (q + 1 < e && s[q] == '.' && s[q + 1] >= '0' && s[q + 1] <= '9') {
    flags = 0;
    ++q;
    while (q < e && s[q] >= '0' && s[q] <= '9') ++q;
  }
  if (q < e && (s[q] == 'e' || s[q] == 'E')) {
    int64_t x = q + 1;
    if (x < e && (s[x] == '+' || s[x] == '-')) ++x;
    if (x < e && s[x] >= '0' && s[x] <= '9') {
      flags = JF_EXP;
      while (x < e && s[x] >= '0' && s[x] <= '9') ++x;
      q = x;
    }
  }
  return q;
}

// the member values the formatter reads, as the scan leaves them (the last duplicate wins)
struct JsonFields {
  int kind[5], flags[5];
  int64_t vb[5], ve[5];  // string: inside the quotes; number: the token
};

// One RFC 8259 value, validated whole, with the top-level members picked out.  Returns 0
// or the reason that ends the message at once; trailing: non-whitespace follows the root.
OTR_HD int json_scan(const uint8_t* s, int64_t b, int64_t e, const MsgFmt& f, JsonFields& J, bool& trailing) {
  enum { V, V_OR_CLOSE, K_OR_CLOSE, K, COLON, AFTER };
  uint64_t stack = 0;  // bit d - 1: level d is an object
  int depth = 0, st = V, mask = 0;
  bool root_object = false, key_escape = false;
  int64_t q = b;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    J.kind[k] = JV_NONE;
    J.flags[k] = 0;
    J.vb[k] = J.ve[k] = 0;
  }
  for (;;) {
    if (st == AFTER && depth == 0) break;
    while (q < e && json_ws(s[q])) ++q;
    if (q >= e) return OTR_FORMAT_D_JSON;
    const uint8_t c = s[q];
    bool close = false;
    if (st == K_OR_CLOSE && c == '}') close = true;
    else if (st == V_OR_CLOSE && c == ']') close = true;
    else if (st == K_OR_CLOSE || st == K) {
      if (c != '"') return OTR_FORMAT_D_JSON;
      bool esc;
      const int64_t r = json_string(s, q, e, esc);
      if (r < 0) return OTR_FORMAT_D_JSON;
      if (depth == 1) {
        key_escape |= esc;
        mask = 0;
        const int64_t n = r - q - 1;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          bool same = n == f.klen[k];
          for (int64_t j = 0; same && j < n; ++j) same = s[q + 1 + j] == f.keys[64 * k + j];
          mask |= same ? 1 << k : 0;
        }
      }
      q = r + 1;
      st = COLON;
    } else if (st == COLON) {
      if (c != ':') return OTR_FORMAT_D_JSON;
      ++q;
      st = V;
    } else if (st == AFTER) {
      const bool in_object = (stack >> (depth - 1)) & 1;
      if (c == ',') {
        ++q;
        st = in_object ? K : V;
      } else if (c == (in_object ? '}' : ']')) {
        close = true;
      } else {
        return OTR_FORMAT_D_JSON;
      }
    } else {  // a value starts
      const bool member = depth == 1 && root_object;
      int kind = JV_NONE, flags = 0;
      int64_t vb = 0, ve = 0;
      if (c == '{' || c == '[') {
        if (depth == 64) return OTR_FORMAT_U_DEPTH;
        if (depth == 0) root_object = c == '{';
        stack = (stack & ~(1ull << depth)) | ((uint64_t)(c == '{') << depth);
        ++depth;
        ++q;
        st = c == '{' ? K_OR_CLOSE : V_OR_CLOSE;
        kind = JV_CONTAINER;
      } else if (c == '"') {
        bool esc;
        const int64_t r = json_string(s, q, e, esc);
        if (r < 0) return OTR_FORMAT_D_JSON;
        kind = JV_STRING;
        flags = esc ? JF_ESCAPE : 0;
        vb = q + 1;
        ve = r;
        q = r + 1;
        st = AFTER;
      } else if (c == '-' || (c >= '0' && c <= '9')) {
        const int64_t r = json_number(s, q, e, flags);
        if (r < 0) return OTR_FORMAT_D_JSON;
        kind = JV_NUMBER;
        vb = q;
        ve = r;
        q = r;
        st = AFTER;
      } else {
        const int n = c == 't' ? 4 : (c == 'f' ? 5 : (c == 'n' ? 4 : 0));
        const char* w = c == 't' ? "true" : (c == 'f' ? "false" : "null");
        if (n == 0 || q + n > e) return OTR_FORMAT_D_JSON;
        for (int j = 1; j < n; ++j)
          if (s[q + j] != (uint8_t)w[j]) return OTR_FORMAT_D_JSON;
        kind = JV_LITERAL;
        q += n;
        st = AFTER;
      }
      if (member) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
          if ((mask >> k) & 1) {
            J.kind[k] = kind;
            J.flags[k] = flags;
            J.vb[k] = vb;
            J.ve[k] = ve;
          }
      }
    }
    if (close) {
      ++q;
      --depth;
      st = AFTER;
    }
  }
  if (!root_object) return OTR_FORMAT_D_ROOT;
  while (q < e && json_ws(s[q])) ++q;
  trailing = q < e;
  return key_escape ? OTR_FORMAT_U_ESCAPE : 0;
}

// lat / lon: node.asText() then floatFormatter.parse(...).floatValue() (Formatter.java:116-117)
OTR_HD int json_coord(const uint8_t* s, int kind, int flags, int64_t b, int64_t e, float& out) {
  if (kind == JV_NONE) return OTR_FORMAT_D_MISSING;
  if (kind == JV_STRING) return (flags & JF_ESCAPE) ? OTR_FORMAT_U_ESCAPE : fm_coord_text(s, b, e, out);
  if (kind != JV_NUMBER) return OTR_FORMAT_U_KIND;
  if (flags & JF_EXP) return OTR_FORMAT_U_NUMBER;
  Dec d;
  double v = 0;
  parse_dec(s, b, e, d);  // the token's grammar is inside parse_dec's
  if (!dec_to_double(d, v)) return OTR_FORMAT_U_PRECISION;
  const double a = v < 0 ? -v : v;
  // beyond [1e-3, 1e7) Double.toString prints E-notation, which DecimalFormat reads only as
  // far as the 'E'
  if (!(a == 0.0 || (a >= 1e-3 && a < 1e7))) return OTR_FORMAT_U_NUMBER;
  out = (float)v;
  return 0;
}

OTR_HD int json_time(const uint8_t* s, int tfmt, int kind, int flags, int64_t b, int64_t e, int64_t& t) {
  if (kind == JV_NONE) return OTR_FORMAT_D_MISSING;
  if (tfmt == OTR_TIME_YMDHMS) {  // DateTime.parse(node.asText(), pattern)
    if (kind == JV_STRING) return (flags & JF_ESCAPE) ? OTR_FORMAT_U_ESCAPE : fm_time_text(s, b, e, t);
    return kind == JV_NUMBER ? OTR_FORMAT_D_TIME : OTR_FORMAT_U_KIND;
  }
  if (kind != JV_NUMBER) return OTR_FORMAT_U_KIND;  // node.asLong()
  return ((flags & JF_INT) && parse_int(s, b, e, t, true)) ? 0 : OTR_FORMAT_U_NUMBER;
}

// (int)Math.ceil(node.asDouble()): through the double, not through float as in SV
OTR_HD int json_acc(const uint8_t* s, int kind, int64_t b, int64_t e, int32_t& a) {
  if (kind == JV_NONE) return OTR_FORMAT_D_MISSING;
  if (kind != JV_NUMBER) return OTR_FORMAT_U_KIND;
  Dec d;
  double v = 0;
  parse_dec(s, b, e, d);
  if (!dec_to_double(d, v)) return OTR_FORMAT_U_PRECISION;
  return fm_ceil_acc(v, a);
}

OTR_HD int json_uuid(const uint8_t* s, int kind, int flags, int64_t b, int64_t e) {
  if (kind == JV_NONE) return OTR_FORMAT_D_MISSING;
  if (kind == JV_STRING) return (flags & JF_ESCAPE) ? OTR_FORMAT_U_ESCAPE : 0;
  if (kind != JV_NUMBER) return OTR_FORMAT_U_KIND;
  int64_t x;
  if (!(flags & JF_INT) || !parse_int(s, b, e, x, true)) return OTR_FORMAT_U_NUMBER;
  return (e - b == 2 && s[b] == '-' && s[b + 1] == '0') ? OTR_FORMAT_U_NUMBER : 0;
}

// Formatter.formatJSON (Formatter.java:111-124)
OTR_HD int format_json(const uint8_t* s, int64_t b, int64_t e, const MsgFmt& f, MsgPoint& p) {
  JsonFields J;
  bool trailing = false;
  const int r = json_scan(s, b, e, f, J, trailing);
  if (r) return r;
  Verdict v{0, 0};
  v.add(json_coord(s, J.kind[FM_LAT], J.flags[FM_LAT], J.vb[FM_LAT], J.ve[FM_LAT], p.lat));
  v.add(json_coord(s, J.kind[FM_LON], J.flags[FM_LON], J.vb[FM_LON], J.ve[FM_LON], p.lon));
  v.add(json_time(s, f.tfmt, J.kind[FM_TIME], J.flags[FM_TIME], J.vb[FM_TIME], J.ve[FM_TIME], p.time));
  v.add(json_acc(s, J.kind[FM_ACC], J.vb[FM_ACC], J.ve[FM_ACC], p.acc));
  v.add(json_uuid(s, J.kind[FM_UUID], J.flags[FM_UUID], J.vb[FM_UUID], J.ve[FM_UUID]));
  if (v.drop) return v.drop;
  if (trailing) return OTR_FORMAT_U_TRAILING;  // readTree stops after the first value
  if (v.unsup) return v.unsup;
  p.uoff = J.vb[FM_UUID];
  p.ulen = (int32_t)(J.ve[FM_UUID] - J.vb[FM_UUID]);
  p.hash = uuid_hash(s, J.vb[FM_UUID], J.ve[FM_UUID]);
  return p.hash == OTR_NO_ID ? OTR_FORMAT_U_NO_ID : 0;
}

OTR_HD int format_message(const uint8_t* s, int64_t b, int64_t e, const MsgFmt& f, MsgPoint& p) {
  return f.type == OTR_FORMAT_JSON ? format_json(s, b, e, f, p) : format_sv(s, b, e, f, p);
}

// ---- kernels --------------------------------------------------------------------------------
#ifndef OTR_INGEST_PARSE_ONLY

struct FormatMsgs {
  const uint8_t* text;
  int64_t len;
  const int64_t* nl;   // positions of '\n' (off == nullptr)
  int64_t n_nl;
  const int64_t* off;  // n + 1 message offsets, or nullptr
  int64_t n;
  int32_t* status;
  uint64_t* hash;
  int64_t* uoff;
  int32_t* ulen;
  int64_t* time;
  float* lat;
  float* lon;
  int32_t* acc;
  int64_t* flag;            // kept | dropped << 32: one scan gives both counts
  unsigned long long* bad;  // min over messages not kept of (message << 8 | reason)
};

// offsets must ascend from >= 0 to <= len
__global__ void k_format_check_off(const int64_t* off, int64_t n, int64_t len, int32_t* wrong) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  const int64_t o = off[i];
  if (o < 0 || o > len || (i < n && off[i + 1] < o)) *wrong = 1;
}

__global__ void __launch_bounds__(256) k_format_parse(FormatMsgs M, MsgFmt f) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M.n) return;
  int64_t b, e;
  if (M.off) {
    b = M.off[i];
    e = M.off[i + 1];
  } else {
    b = i ? M.nl[i - 1] + 1 : 0;
    e = i < M.n_nl ? M.nl[i] : M.len;
  }
  MsgPoint p{};
  const int r = format_message(M.text, b, e, f, p);
  M.status[i] = r;
  M.flag[i] = r == 0 ? 1 : (r < OTR_FORMAT_UNSUPPORTED ? (int64_t)1 << 32 : 0);
  if (r) {
    atomicMin(M.bad, ((unsigned long long)i << 8) | (unsigned)r);
    return;
  }
  M.hash[i] = p.hash;
  M.uoff[i] = p.uoff;
  M.ulen[i] = p.ulen;
  M.time[i] = p.time;
  M.lat[i] = p.lat;
  M.lon[i] = p.lon;
  M.acc[i] = p.acc;
}

struct FormatOut {
  unsigned long long* key;
  float* lat;
  float* lon;
  int32_t* acc;
  int64_t* time;
  int64_t* ts;
  int64_t* msg;
  int64_t* uoff;
  int32_t* ulen;
  int32_t* kidx;  // kept message indices, for the collision check
};

// stable compaction of the kept messages: arrival order exactly
__global__ void k_format_emit(FormatMsgs M, const int64_t* scan, const int64_t* ts_in, int64_t ts_all, FormatOut o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M.n || M.status[i] != 0) return;
  const int64_t k = (int64_t)(uint32_t)scan[i] - 1;
  o.key[k] = M.hash[i];
  o.lat[k] = M.lat[i];
  o.lon[k] = M.lon[i];
  o.acc[k] = M.acc[i];
  o.time[k] = M.time[i];
  o.ts[k] = ts_in ? ts_in[i] : ts_all;
  o.msg[k] = i;
  o.uoff[k] = M.uoff[i];
  o.ulen[k] = M.ulen[i];
  o.kidx[k] = (int32_t)i;
}

#endif  // OTR_INGEST_PARSE_ONLY
}  // namespace otr
