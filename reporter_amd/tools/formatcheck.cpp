// Host build of the stream formatter's per-message functions (reporter_amd/csrc/
// otr_formatter.h) so that the CPU tests can compare them with the restatement
// tests/formatter_ref.py on a corpus and its mutations.
// TEST INFRASTRUCTURE ONLY: the product formats on the GPU (k_format_parse).
#define OTR_POW5_QUAL static
#define OTR_INGEST_PARSE_ONLY
#include "../csrc/otr_formatter.h"

using namespace otr;

namespace {
// out: hash, uoff, time as int64 [3]; ulen, acc as int32 [2]; lat, lon as float [2]
int run(int type, int sep, int tfmt, const int32_t* idx, const uint8_t* keys, const int32_t* klen, const char* s,
        int64_t n, int64_t* o64, int32_t* o32, float* of) {
  MsgFmt f{};
  f.type = type;
  f.sep = sep;
  f.tfmt = tfmt;
  for (int k = 0; k < 5; ++k) {
    f.idx[k] = idx ? idx[k] : 0;
    f.klen[k] = klen ? klen[k] : 0;
  }
  f.keys = keys;
  MsgPoint p{};
  const int r = format_message(reinterpret_cast<const uint8_t*>(s), 0, n, f, p);
  o64[0] = (int64_t)p.hash;
  o64[1] = p.uoff;
  o64[2] = p.time;
  o32[0] = p.ulen;
  o32[1] = p.acc;
  of[0] = p.lat;
  of[1] = p.lon;
  return r;
}
}  // namespace

extern "C" {
// idx: uuid, time, lat, lon, accuracy field positions (K11's order); returns 0 or the reason
int fc_format_sv(int sep, int tfmt, const int32_t* idx, const char* s, int64_t n, int64_t* o64, int32_t* o32,
                 float* of) {
  return run(OTR_FORMAT_SV, sep, tfmt, idx, nullptr, nullptr, s, n, o64, o32, of);
}
// keys: 5 keys of 64 bytes each in the same order, klen their lengths
int fc_format_json(int tfmt, const uint8_t* keys, const int32_t* klen, const char* s, int64_t n, int64_t* o64,
                   int32_t* o32, float* of) {
  return run(OTR_FORMAT_JSON, 0, tfmt, nullptr, keys, klen, s, n, o64, o32, of);
}
}
