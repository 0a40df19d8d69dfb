// Host build of the tile records' per-record rules (reporter_amd/csrc/otr_tile_records.h) as a
// stand-alone program, so that the CPU tests can run them under AddressSanitizer /
// UndefinedBehaviorSanitizer and compare them with the restatement tests/tile_records_ref.py.
// TEST INFRASTRUCTURE ONLY: the product decodes and encodes on the GPU.
//
//   tilerecordcheck FILE [SHIFT]
// FILE (little-endian): int64 n_records, n_bytes, quantisation, slice_size; int64 start[n],
// tile_id[n], slice[n]; int64 rec_off[n + 1]; then n_bytes bytes.  The bytes are placed SHIFT
// bytes into an exactly sized allocation (so a read past either end is an error, and with an odd
// SHIFT nothing is aligned).  Output, per record: "i refused R" with R the lowest of the layout,
// key, count and segment reasons, or "i ok count KEY" (KEY the slice's changelog key, which must
// parse back to the record's key) followed by one line "id next_id min_bits max_bits length queue"
// per segment; each good record is also encoded again from the decoded values, by bytes and by
// dwords, and must give its bytes back ("i reencode differs" otherwise).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/otr_tile_records.h"

using namespace otr;

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: tilerecordcheck FILE [SHIFT]\n");
    return 2;
  }
  const long shift = argc > 2 ? atol(argv[2]) : 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int64_t head[4];
  if (fread(head, 8, 4, f) != 4 || head[0] < 0 || head[1] < 0 || head[2] < 1 || shift < 0) {
    fprintf(stderr, "bad file\n");
    return 2;
  }
  const int64_t n = head[0], nb = head[1], q = head[2], slice_size = head[3];
  std::vector<int64_t> start((size_t)n), tile((size_t)n), slice((size_t)n), off((size_t)n + 1);
  if (fread(start.data(), 8, (size_t)n, f) != (size_t)n || fread(tile.data(), 8, (size_t)n, f) != (size_t)n ||
      fread(slice.data(), 8, (size_t)n, f) != (size_t)n || fread(off.data(), 8, off.size(), f) != off.size()) {
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
    const int32_t sl = (int32_t)slice[i];
    int reason = 0;
    if (!tile_rec_layout_ok(bytes, nb, off[i], off[i + 1], &count)) reason = OTR_TILE_RESTORE_E_LAYOUT;
    else if (!tile_rec_key_ok(start[i], tile[i], sl, q)) reason = OTR_TILE_RESTORE_E_KEY;
    else if (count < 1 || count > slice_size) reason = OTR_TILE_RESTORE_E_COUNT;
    const uint8_t* rec = bytes + off[i];
    if (!reason)
      for (int32_t k = 0; k < count && !reason; ++k)
        if (!tile_rec_segment_ok(tile_rec_segment_get(rec, k), tile[i], start[i] / q, q))
          reason = OTR_TILE_RESTORE_E_SEGMENT;
    if (reason) {
      printf("%lld refused %d\n", (long long)i, reason);
      continue;
    }
    char key[kTileKeyMax + 1];
    const int32_t kl = tile_key_put(start[i], tile[i], sl, (uint8_t*)key);
    key[kl] = 0;
    int64_t ps = -1, pt = -1;
    int32_t pl = -1;
    if (kl != tile_key_len(start[i], tile[i], sl) || !tile_key_parse(key, kl, &ps, &pt, &pl) || ps != start[i] ||
        pt != tile[i] || pl != sl)
      printf("%lld key differs\n", (long long)i);
    printf("%lld ok %d %s\n", (long long)i, count, key);
    const size_t len = (size_t)(off[i + 1] - off[i]);
    uint8_t* again = (uint8_t*)malloc(len + 1) + 1;  // odd address: the puts assume no alignment either
    std::vector<uint32_t> words(len / 4);
    rec_put32(again, (uint32_t)count);
    words[0] = tr_bswap32((uint32_t)count);
    for (int32_t k = 0; k < count; ++k) {
      const TileSegment s = tile_rec_segment_get(rec, k);
      printf("%llu %llu %llu %llu %d %d\n", (unsigned long long)s.id, (unsigned long long)s.next_id,
             (unsigned long long)tr_double_bits(s.t0), (unsigned long long)tr_double_bits(s.t1), s.length, s.queue);
      tile_rec_segment_put(again, k, s);
      for (int32_t w = 0; w < 10; ++w) words[1 + 10 * (size_t)k + w] = tile_rec_segment_word(s, w);
    }
    if (memcmp(again, rec, len) != 0 || memcmp(words.data(), rec, len) != 0)
      printf("%lld reencode differs\n", (long long)i);
    free(again - 1);
  }
  free(mem);
  return 0;
}
