// Host build of the tile file parser's per-line and per-name rules and of its line table
// (reporter_amd/csrc/otr_tileparse.h) as a stand-alone program, so that the CPU tests can run them
// under AddressSanitizer / UndefinedBehaviorSanitizer and compare them with the restatement
// tests/tile_parse_ref.py.
// TEST INFRASTRUCTURE ONLY: the product parses the texts on the GPU (the kernels of the same header).
//
//   tileparsecheck FILE [SHIFT]
// FILE (little-endian): int64 n_files, quantisation, rules, source_len, mode_len, text_len,
// names_len; text_off[n_files + 1]; name_off[n_files + 1]; the text; the names; the source bytes;
// the mode bytes.  The text, the names and the tag are each read from SHIFT bytes into an exactly
// sized allocation (a byte before or behind is an error, and with an odd SHIFT nothing is
// aligned).  The steps are the kernels': the newline positions, per file its newlines and line
// count, the counts' running sum, per file the name, per line the status and the row.  Output:
//   "files F lines L rows R headers H bad B bad_names M first_bad LINE FILE REASON"
//   per file "file FILE STATUS LINE_OFF ROW_OFF"
//   "status s0 s1 ..."
//   per row "row FILE ID NEXT START END DURATION LENGTH QUEUE SPEED_BIN"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/otr_tileparse.h"

using namespace otr;

static uint8_t* exact(size_t n, long shift, uint8_t** mem) {
  *mem = (uint8_t*)malloc(n + (size_t)shift ? n + (size_t)shift : 1);
  return *mem + shift;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: tileparsecheck FILE [SHIFT]\n");
    return 2;
  }
  const long shift = argc > 2 ? atol(argv[2]) : 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int64_t head[7];
  if (fread(head, 8, 7, f) != 7 || head[0] < 0 || head[1] < 1 || !tile_text_rules_ok((int32_t)head[2]) || head[3] < 0 ||
      head[3] > kTileTextTagPart || head[4] < 0 || head[4] > kTileTextTagPart || head[5] < 0 || head[6] < 0 || shift < 0) {
    fprintf(stderr, "bad file\n");
    return 2;
  }
  const int64_t nf = head[0], q = head[1], text_len = head[5], names_len = head[6];
  const int32_t rules = (int32_t)head[2], src_len = (int32_t)head[3], mode_len = (int32_t)head[4];
  std::vector<int64_t> text_off((size_t)nf + 1), name_off((size_t)nf + 1);
  uint8_t *text_mem, *names_mem, *src_mem, *mode_mem, *tag_mem;
  uint8_t* text = exact((size_t)text_len, shift, &text_mem);
  uint8_t* names = exact((size_t)names_len, shift, &names_mem);
  uint8_t* src = exact((size_t)src_len, shift, &src_mem);
  uint8_t* mode = exact((size_t)mode_len, shift, &mode_mem);
  bool ok = fread(text_off.data(), 8, (size_t)nf + 1, f) == (size_t)nf + 1 &&
            fread(name_off.data(), 8, (size_t)nf + 1, f) == (size_t)nf + 1 &&
            (!text_len || fread(text, 1, (size_t)text_len, f) == (size_t)text_len) &&
            (!names_len || fread(names, 1, (size_t)names_len, f) == (size_t)names_len) &&
            (!src_len || fread(src, 1, (size_t)src_len, f) == (size_t)src_len) &&
            (!mode_len || fread(mode, 1, (size_t)mode_len, f) == (size_t)mode_len);
  fclose(f);
  ok = ok && text_off[0] == 0 && name_off[0] == 0 && text_off[(size_t)nf] == text_len && name_off[(size_t)nf] == names_len;
  for (int64_t k = 0; ok && k < nf; ++k)
    ok = text_off[(size_t)k + 1] >= text_off[(size_t)k] && name_off[(size_t)k + 1] >= name_off[(size_t)k];
  if (!ok) {
    fprintf(stderr, "bad file\n");
    return 2;
  }
  const int32_t want_tag = 2 + src_len + mode_len + (rules == OTR_TILE_RULES_STREAM ? 0 : 1);
  uint8_t* tag = exact((size_t)want_tag, shift, &tag_mem);
  const int32_t tag_len = tile_text_tag_put(src, src_len, mode, mode_len, rules, tag);
  // the newline positions
  std::vector<int64_t> nl;
  for (int64_t p = 0; p < text_len; ++p)
    if (text[p] == '\n') nl.push_back(p);
  const int64_t n_nl = (int64_t)nl.size();
  // the line table
  std::vector<int64_t> nl_lo((size_t)nf + 1), file_line_off((size_t)nf + 1, 0);
  for (int64_t k = 0; k <= nf; ++k) nl_lo[(size_t)k] = tp_lower_bound(nl.data(), n_nl, text_off[(size_t)k]);
  for (int64_t k = 0; k < nf; ++k)
    file_line_off[(size_t)k + 1] =
        file_line_off[(size_t)k] + tile_parse_file_lines(nl.data(), nl_lo[(size_t)k], nl_lo[(size_t)k + 1],
                                                         text_off[(size_t)k], text_off[(size_t)k + 1], rules);
  const int64_t n_lines = file_line_off[(size_t)nf];
  // the names
  std::vector<uint64_t> file((size_t)nf);
  std::vector<uint8_t> file_status((size_t)nf);
  int64_t n_bad_names = 0;
  for (int64_t k = 0; k < nf; ++k) {
    uint64_t v = OTR_NO_ID;
    const bool good = tile_parse_name(names, name_off[(size_t)k], name_off[(size_t)k + 1], q, v);
    file[(size_t)k] = good ? v : OTR_NO_ID;
    file_status[(size_t)k] = good ? 0 : 1;
    n_bad_names += good ? 0 : 1;
  }
  // the lines
  std::vector<uint8_t> status((size_t)n_lines);
  std::vector<otr_tile_row> rows;
  std::vector<int64_t> row_off((size_t)nf + 1, 0);
  int64_t n_headers = 0, n_bad = 0, first_bad = -1, first_bad_file = -1;
  int32_t first_bad_reason = 0;
  for (int64_t i = 0; i < n_lines; ++i) {
    const int64_t k = tile_parse_file_of(file_line_off.data(), nf, i);
    int32_t st = OTR_TILE_LINE_U_NAME;
    if (!file_status[(size_t)k]) {
      const int64_t j = i - file_line_off[(size_t)k];
      int64_t b, e;
      const bool terminated = tile_parse_piece(nl.data(), nl_lo[(size_t)k], nl_lo[(size_t)k + 1], text_off[(size_t)k],
                                               text_off[(size_t)k + 1], j, &b, &e);
      otr_tile_row r;
      st = tile_parse_line(text, b, e, j == 0, terminated, rules, tag, tag_len, file[(size_t)k], &r);
      if (st == OTR_TILE_LINE_ROW) {
        rows.push_back(r);
        ++row_off[(size_t)k + 1];  // the file's own count; summed below
      }
    }
    status[(size_t)i] = (uint8_t)st;
    n_headers += st == OTR_TILE_LINE_HEADER;
    if (st >= OTR_TILE_LINE_E_FIELDS) {
      if (!n_bad++) {
        first_bad = i;
        first_bad_file = k;
        first_bad_reason = st;
      }
    }
  }
  for (int64_t k = 0; k < nf; ++k) row_off[(size_t)k + 1] += row_off[(size_t)k];
  printf("files %lld lines %lld rows %lld headers %lld bad %lld bad_names %lld first_bad %lld %lld %d\n", (long long)nf,
         (long long)n_lines, (long long)rows.size(), (long long)n_headers, (long long)n_bad, (long long)n_bad_names,
         (long long)first_bad, (long long)first_bad_file, first_bad_reason);
  for (int64_t k = 0; k < nf; ++k)
    printf("file %llu %d %lld %lld\n", (unsigned long long)file[(size_t)k], (int)file_status[(size_t)k],
           (long long)file_line_off[(size_t)k], (long long)row_off[(size_t)k]);
  printf("status");
  for (int64_t i = 0; i < n_lines; ++i) printf(" %d", (int)status[(size_t)i]);
  printf("\n");
  for (const otr_tile_row& r : rows)
    printf("row %llu %llu %llu %lld %lld %d %d %d %d\n", (unsigned long long)r.file, (unsigned long long)r.id,
           (unsigned long long)r.next_id, (long long)r.start, (long long)r.end, r.duration, r.length, r.queue_length,
           r.speed_bin);
  free(text_mem);
  free(names_mem);
  free(src_mem);
  free(mode_mem);
  free(tag_mem);
  return 0;
}
