/* hash_capture.c -- calls libxsmm_hash, libxsmm_memcmp, libxsmm_diff and libxsmm_diff_n of the unmodified reference and writes
 * what they return as raw binary, for tools/golden/hash_capture.py to pack into tests/golden/hash.npz. It includes the
 * reference header-only, as tools/golden/matdiff_capture.c does, so it needs the reference's generated headers (its make
 * writes include/libxsmm.h and include/libxsmm_config.h) and no library:
 *   gcc -O1 -I<reference>/include hash_capture.c -lm -lpthread -ldl -lrt -o hash_capture
 * Usage: hash_capture check                                       the guard: exits 0 if hash("123456789", 9, ~0) is 0x1CF96D7C
 *        hash_capture hash seed file out                           one unsigned int
 *        hash_capture cmp file_a file_b out                        two ints: libxsmm_memcmp, and libxsmm_diff if the size allows (else -1)
 *        hash_capture diff_n size stride hint n file_a file_bn out one unsigned int
 * An empty operand is a file of no bytes. */
#include <libxsmm_source.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static void* slurp(const char* path, size_t* size)
{
  FILE* const f = fopen(path, "rb");
  long bytes;
  void* p;
  if (NULL == f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END); bytes = ftell(f); fseek(f, 0, SEEK_SET);
  p = malloc((size_t)bytes + 64);
  if (NULL == p || (size_t)bytes != fread(p, 1, (size_t)bytes, f)) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fclose(f);
  *size = (size_t)bytes;
  return p;
}

static void put(const char* path, const void* data, size_t size)
{
  FILE* const f = fopen(path, "wb");
  if (NULL == f || 1 != fwrite(data, size, 1, f)) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}

int main(int argc, char* argv[])
{
  const char* const what = (1 < argc ? argv[1] : "");
  size_t na = 0, nb = 0;
  if (0 == strcmp(what, "check")) {
    return (0x1CF96D7Cu == libxsmm_hash("123456789", 9, 0xFFFFFFFFu) && 0x58E3FA20u == libxsmm_hash("123456789", 9, 0)) ? 0 : 1;
  }
  if (0 == strcmp(what, "hash") && 5 == argc) {
    const void* const data = slurp(argv[3], &na);
    const unsigned int h = libxsmm_hash(data, (unsigned int)na, (unsigned int)strtoul(argv[2], NULL, 0));
    put(argv[4], &h, sizeof(h));
    return 0;
  }
  if (0 == strcmp(what, "cmp") && 5 == argc) {
    const void *const a = slurp(argv[2], &na), *const b = slurp(argv[3], &nb);
    int r[2];
    if (na != nb) return 2;
    r[0] = libxsmm_memcmp(a, b, na);
    r[1] = (na <= 255 ? (int)libxsmm_diff(a, b, (unsigned char)na) : -1);
    put(argv[4], r, sizeof(r));
    return 0;
  }
  if (0 == strcmp(what, "diff_n") && 9 == argc) {
    const void *const a = slurp(argv[6], &na), *const bn = slurp(argv[7], &nb);
    const unsigned int r = libxsmm_diff_n(a, bn, (unsigned char)atoi(argv[2]), (unsigned char)atoi(argv[3]), (unsigned int)strtoul(argv[4], NULL, 0),
      (unsigned int)strtoul(argv[5], NULL, 0));
    put(argv[8], &r, sizeof(r));
    return 0;
  }
  fprintf(stderr, "usage: see the head of hash_capture.c\n");
  return 1;
}
