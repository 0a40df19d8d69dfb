// Host build of the session records' per-record rules (reporter_amd/csrc/
// otr_session_records.h) as a stand-alone program, so that the CPU tests can run them under
// AddressSanitizer / UndefinedBehaviorSanitizer and compare them with the restatement
// tests/session_records_ref.py.
// TEST INFRASTRUCTURE ONLY: the product decodes and encodes on the GPU (otr_sessions.h).
//
//   recordcheck FILE [SHIFT]
// FILE (little-endian): int64 n_records, int64 n_bytes, int64 rec_off[n_records + 1], then
// n_bytes bytes.  The bytes are placed SHIFT bytes into an exactly sized allocation (so a
// read past either end is an error, and with an odd SHIFT nothing is aligned).  Output, one
// line per record: "i bad", or "i ok count max_sep_bits last_update" followed by one line
// "lat_bits lon_bits accuracy time" per point; each good record is also encoded again from
// the decoded values and must give its bytes back ("i reencode differs" otherwise).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/otr_session_records.h"

using namespace otr;

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: recordcheck FILE [SHIFT]\n");
    return 2;
  }
  const long shift = argc > 2 ? atol(argv[2]) : 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int64_t head[2];
  if (fread(head, 8, 2, f) != 2 || head[0] < 0 || head[1] < 0 || shift < 0) {
    fprintf(stderr, "bad file\n");
    return 2;
  }
  const int64_t n = head[0], nb = head[1];
  std::vector<int64_t> off((size_t)n + 1);
  if (fread(off.data(), 8, off.size(), f) != off.size()) {
    fprintf(stderr, "bad file\n");
    return 2;
  }
  uint8_t* mem = (uint8_t*)malloc((size_t)(nb + shift) ? (size_t)(nb + shift) : 1);
  uint8_t* bytes = mem + shift;
  if (nb > 0 && fread(bytes, 1, (size_t)nb, f) != (size_t)nb) {
    fprintf(stderr, "bad file\n");
    return 2;
  }
  fclose(f);
  for (int64_t i = 0; i < n; ++i) {
    int32_t count;
    if (!rec_layout_ok(bytes, nb, off[i], off[i + 1], &count)) {
      printf("%lld bad\n", (long long)i);
      continue;
    }
    const uint8_t* rec = bytes + off[i];
    float ms;
    int64_t last;
    rec_header_get(rec, &count, &ms, &last);
    printf("%lld ok %d %u %lld\n", (long long)i, count, rec_float_bits(ms), (long long)last);
    const size_t len = (size_t)(off[i + 1] - off[i]);
    uint8_t* again = (uint8_t*)malloc(len + 1) + 1;  // odd address: the puts assume no alignment either
    rec_header_put(again, count, ms, last);
    for (int32_t k = 0; k < count; ++k) {
      float la, lo;
      int32_t ac;
      int64_t tm;
      rec_point_get(rec, k, &la, &lo, &ac, &tm);
      printf("%u %u %d %lld\n", rec_float_bits(la), rec_float_bits(lo), ac, (long long)tm);
      rec_point_put(again, k, la, lo, ac, tm);
    }
    if (memcmp(again, rec, len) != 0) printf("%lld reencode differs\n", (long long)i);
    free(again - 1);
  }
  free(mem);
  return 0;
}
