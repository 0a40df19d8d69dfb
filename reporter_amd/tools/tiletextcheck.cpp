// Host build of the tile file texts' per-row and per-file rules (reporter_amd/csrc/
// otr_tiletext.h) as a stand-alone program, so that the CPU tests can run them under
// AddressSanitizer / UndefinedBehaviorSanitizer and compare them with the restatement
// tests/tile_text_ref.py.
// TEST INFRASTRUCTURE ONLY: the product writes the texts on the GPU (the kernels of the same header).
//
//   tiletextcheck FILE [SHIFT]
// FILE (little-endian): int64 n_rows, quantisation, source_len, mode_len; n_rows otr_tile_row
// records (56 bytes each); the source bytes; the mode bytes.  The rows are read from SHIFT bytes
// into an exactly sized allocation, and every text and every name is written SHIFT bytes into
// an exactly sized allocation (a byte before or behind is an error, and with an odd SHIFT
// nothing is aligned).  Runs of equal `file` are the files.  Output, for rules 0 and 1:
//   "rules R files F rows N text T names M"
//   "lens l0 l1 ..."                      the rows' own lengths (tile_text_row_len)
//   per file "file FILE ROW_OFF TEXT_OFF NAME" and "text HEX" (the file's whole text)
// A length that disagrees with the bytes put is reported as "mismatch ..." (exit status 1).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/otr_tiletext.h"

using namespace otr;

static uint8_t* exact(size_t n, long shift, uint8_t** mem) {
  *mem = (uint8_t*)malloc(n + (size_t)shift ? n + (size_t)shift : 1);
  return *mem + shift;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: tiletextcheck FILE [SHIFT]\n");
    return 2;
  }
  const long shift = argc > 2 ? atol(argv[2]) : 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int64_t head[4];
  if (fread(head, 8, 4, f) != 4 || head[0] < 0 || head[1] < 1 || head[2] < 0 || head[2] > kTileTextTagPart ||
      head[3] < 0 || head[3] > kTileTextTagPart || shift < 0) {
    fprintf(stderr, "bad file\n");
    return 2;
  }
  const int64_t n = head[0], q = head[1];
  const int32_t src_len = (int32_t)head[2], mode_len = (int32_t)head[3];
  const size_t row_bytes = (size_t)n * sizeof(otr_tile_row);
  uint8_t *row_mem, *src_mem, *mode_mem;
  uint8_t* raw = exact(row_bytes, shift, &row_mem);
  uint8_t* src = exact((size_t)src_len, shift, &src_mem);
  uint8_t* mode = exact((size_t)mode_len, shift, &mode_mem);
  if ((row_bytes && fread(raw, 1, row_bytes, f) != row_bytes) ||
      (src_len && fread(src, 1, (size_t)src_len, f) != (size_t)src_len) ||
      (mode_len && fread(mode, 1, (size_t)mode_len, f) != (size_t)mode_len)) {
    fprintf(stderr, "bad file\n");
    return 2;
  }
  fclose(f);
  std::vector<otr_tile_row> rows((size_t)n);
  for (int64_t i = 0; i < n; ++i) memcpy(&rows[(size_t)i], raw + (size_t)i * sizeof(otr_tile_row), sizeof(otr_tile_row));
  int status = 0;
  for (int32_t rules = 0; rules < 2; ++rules) {
    uint8_t* tag_mem;
    const int32_t want_tag = 2 + src_len + mode_len + (rules == OTR_TILE_RULES_STREAM ? 0 : 1);
    uint8_t* tag = exact((size_t)want_tag, shift, &tag_mem);
    const int32_t tag_len = tile_text_tag_put(src, src_len, mode, mode_len, rules, tag);
    if (tag_len != want_tag) {
      printf("mismatch tag %d %d\n", tag_len, want_tag);
      status = 1;
    }
    std::vector<int64_t> off((size_t)n + 1, 0), starts;
    std::vector<int32_t> lens((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      const bool is_head = i == 0 || rows[(size_t)i].file != rows[(size_t)i - 1].file;
      if (is_head) starts.push_back(i);
      lens[(size_t)i] = tile_text_row_len(rows[(size_t)i], rules, tag_len);
      off[(size_t)i + 1] = off[(size_t)i] + lens[(size_t)i] + (is_head ? tile_text_header_len(rules) : 0);
    }
    const int64_t nf = (int64_t)starts.size(), total = off[(size_t)n];
    starts.push_back(n);
    uint8_t* text_mem;
    uint8_t* text = exact((size_t)total, shift, &text_mem);
    for (int64_t i = 0; i < n; ++i) {
      int64_t pos = off[(size_t)i];
      if (i == 0 || rows[(size_t)i].file != rows[(size_t)i - 1].file)
        pos = tile_text_header_emit(rules, TtPtrSink{text}, pos);
      pos += tile_text_row_put(rows[(size_t)i], rules, tag, tag_len, text + pos);
      if (pos != off[(size_t)i + 1]) {
        printf("mismatch row %lld %lld %lld\n", (long long)i, (long long)pos, (long long)off[(size_t)i + 1]);
        status = 1;
      }
    }
    int64_t name_total = 0;
    for (int64_t k = 0; k < nf; ++k) name_total += tile_text_name_len(rows[(size_t)starts[(size_t)k]].file, q);
    printf("rules %d files %lld rows %lld text %lld names %lld\n", rules, (long long)nf, (long long)n,
           (long long)total, (long long)name_total);
    printf("lens");
    for (int64_t i = 0; i < n; ++i) printf(" %d", lens[(size_t)i]);
    printf("\n");
    for (int64_t k = 0; k < nf; ++k) {
      const uint64_t file = rows[(size_t)starts[(size_t)k]].file;
      const int32_t nl = tile_text_name_len(file, q);
      uint8_t* name_mem;
      uint8_t* name = exact((size_t)nl, shift, &name_mem);
      if (tile_text_name_put(file, q, name) != nl) {
        printf("mismatch name %lld\n", (long long)k);
        status = 1;
      }
      const int64_t t0 = off[(size_t)starts[(size_t)k]], t1 = off[(size_t)starts[(size_t)k + 1]];
      printf("file %llu %lld %lld %.*s\ntext ", (unsigned long long)file, (long long)starts[(size_t)k], (long long)t0,
             (int)nl, (const char*)name);
      for (int64_t p = t0; p < t1; ++p) printf("%02x", text[p]);
      printf("\n");
      free(name_mem);
    }
    free(text_mem);
    free(tag_mem);
  }
  free(row_mem);
  free(src_mem);
  free(mode_mem);
  return status;
}
