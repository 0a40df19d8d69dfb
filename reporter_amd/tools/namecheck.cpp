// Host build of the uuid directory's per-name rules (reporter_amd/csrc/otr_session_names.h) as
// a stand-alone program, so that the CPU tests can run them under AddressSanitizer /
// UndefinedBehaviorSanitizer and compare them with the restatement tests/session_names_ref.py.
// TEST INFRASTRUCTURE ONLY: the product checks, stores and sorts names on the GPU (otr_sessions.h).
//
//   namecheck FILE [SHIFT]
// FILE (little-endian int64 words, then bytes): uuid_bytes, n_rows, n_names, n_bytes; per row
// (off, len) of the name it holds; per name (off, len, row, first): row >= 0: the directory
// row its key's live session has, first >= 0: the name of its key's first arrival; then n_bytes
// bytes.  The bytes are placed SHIFT bytes into an exactly sized allocation (a read past either
// end is an error, and with an odd SHIFT nothing is aligned).  The rows are written with
// name_write_row into 16-byte aligned rows that held 0xAA before.  Output: one line
// "row r len tail w0 w1 ..." per row (tail: 1 when every byte beyond the length is zero; the
// sort words in hex), then one line "i reason" per name.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/otr_session_names.h"

using namespace otr;

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: namecheck FILE [SHIFT]\n");
    return 2;
  }
  const long shift = argc > 2 ? atol(argv[2]) : 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int64_t head[4];
  if (fread(head, 8, 4, f) != 4 || head[0] < 1 || head[0] > 255 || head[1] < 0 || head[2] < 0 || head[3] < 0 ||
      shift < 0) {
    fprintf(stderr, "bad file\n");
    return 2;
  }
  const int32_t ub = (int32_t)head[0], row_bytes = name_row_bytes(ub), words = name_sort_words(ub);
  const int64_t n_rows = head[1], n_names = head[2], nb = head[3];
  std::vector<int64_t> rows((size_t)n_rows * 2), names((size_t)n_names * 4);
  if (fread(rows.data(), 8, rows.size(), f) != rows.size() || fread(names.data(), 8, names.size(), f) != names.size()) {
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
  const size_t dir_bytes = (size_t)(n_rows ? n_rows : 1) * (size_t)row_bytes;
  uint8_t* dir = (uint8_t*)aligned_alloc(16, dir_bytes);
  memset(dir, 0xAA, dir_bytes);
  std::vector<int32_t> dir_len((size_t)n_rows, 0);
  for (int64_t r = 0; r < n_rows; ++r) {
    const int64_t off = rows[2 * r];
    const int32_t len = (int32_t)rows[2 * r + 1];
    if (name_own_reason(off, len, nb, ub)) {
      fprintf(stderr, "bad file: row %lld\n", (long long)r);
      return 2;
    }
    uint8_t* row = dir + (size_t)r * (size_t)row_bytes;
    name_write_row(row, row_bytes, bytes, off, len);
    dir_len[r] = len;
    int tail = 1;
    for (int32_t k = len; k < row_bytes; ++k) tail &= row[k] == 0;
    printf("row %lld %d %d", (long long)r, len, tail);
    for (int32_t w = 0; w < words; ++w) printf(" %016llx", (unsigned long long)name_sort_word(row, w));
    printf("\n");
  }
  for (int64_t i = 0; i < n_names; ++i) {
    const int64_t off = names[4 * i], len64 = names[4 * i + 1], r = names[4 * i + 2], first = names[4 * i + 3];
    if (len64 < INT32_MIN || len64 > INT32_MAX || r >= n_rows || first >= n_names) {
      fprintf(stderr, "bad file: name %lld\n", (long long)i);
      return 2;
    }
    const bool has_first = first >= 0;
    const int64_t foff = has_first ? names[4 * first] : 0;
    const int32_t flen = has_first ? (int32_t)names[4 * first + 1] : 0;
    const int32_t why = name_reason(bytes, nb, ub, off, (int32_t)len64, r >= 0 ? dir + (size_t)r * (size_t)row_bytes : nullptr,
                                    r >= 0 ? dir_len[r] : 0, has_first, foff, flen);
    printf("%lld %d\n", (long long)i, why);
  }
  free(dir);
  free(mem);
  return 0;
}
