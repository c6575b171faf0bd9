/* hash_caller.c -- a caller of the reference's hash and compare functions (include/libxsmm_math.h:76-89; what
 * samples/utilities/diff/diff.c exercises): libxsmm_hash, libxsmm_memcmp, libxsmm_diff and libxsmm_diff_n on host buffers and,
 * where a device is there, on device copies of them. The four functions are called exactly as with the reference; the only
 * other calls are the ones that put the copies into device memory. The answers must not depend on where the bytes lie.
 *   gcc -std=c89 -Wall -I include examples/hash_caller.c -L libxsmm-1_amd/lib -lxsmm */
#include <libxsmm.h>
#include <libxsmm_amd.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define ITEM 16
#define ITEMS 1000

int main(void)
{
  const size_t bytes = (size_t)ITEM * ITEMS;
  const unsigned int seed = 0x9E3779B9u, wanted = 617;
  unsigned char *a = (unsigned char*)malloc(bytes), *b = (unsigned char*)malloc(bytes), key[ITEM];
  unsigned int hash_a, hash_b, found, none;
  int result = EXIT_SUCCESS;
  size_t i;
  if (NULL == a || NULL == b) return EXIT_FAILURE;
  for (i = 0; i < bytes; ++i) b[i] = a[i] = (unsigned char)((i * 7 + i / 251) % 253);
  b[bytes - 1] ^= 1; /* the copy differs in its last byte */
  for (i = 0; i < ITEM; ++i) key[i] = (unsigned char)(0xA0 + i); /* an item that occurs nowhere else ... */
  memcpy(a + wanted * ITEM, key, ITEM);                          /* ... but here */

  libxsmm_init();
  if (0x1CF96D7Cu != libxsmm_hash("123456789", 9, 0xFFFFFFFFu)) { fprintf(stderr, "hash_caller: not CRC-32C\n"); result = EXIT_FAILURE; }
  hash_a = libxsmm_hash(a, (unsigned int)bytes, seed);
  hash_b = libxsmm_hash(b, (unsigned int)bytes, seed);
  found = libxsmm_diff_n(key, a, ITEM, ITEM, 900, ITEMS); /* the search starts at item 900 and goes round */
  none = libxsmm_diff_n(key, b, ITEM, ITEM, 0, ITEMS);
  if (hash_a == hash_b || 0 != libxsmm_memcmp(a, a, bytes) || 0 == libxsmm_memcmp(a, b, bytes) || 0 != libxsmm_diff(a, b, 255)
    || 0 == libxsmm_diff(a + bytes - 255, b + bytes - 255, 255) || wanted != found || ITEMS != none)
  {
    fprintf(stderr, "hash_caller: host buffers: %08x %08x, found %u, none %u\n", hash_a, hash_b, found, none); result = EXIT_FAILURE;
  }

  if (0 < libxsmm_amd_device_count()) { /* the same calls on device copies: the values come back, the bytes do not */
    unsigned char *da = (unsigned char*)libxsmm_amd_device_malloc(bytes), *db = (unsigned char*)libxsmm_amd_device_malloc(bytes);
    if (NULL == da || NULL == db) { fprintf(stderr, "hash_caller: no device memory\n"); return EXIT_FAILURE; }
    libxsmm_amd_memcpy_h2d(da, a, bytes);
    libxsmm_amd_memcpy_h2d(db, b, bytes);
    if (hash_a != libxsmm_hash(da, (unsigned int)bytes, seed) || hash_b != libxsmm_hash(db, (unsigned int)bytes, seed)
      || 0 != libxsmm_memcmp(da, a, bytes) /* one operand on the device, the other pageable */
      || 0 == libxsmm_memcmp(da, db, bytes) || 0 != libxsmm_diff(da, db, 255) || 0 == libxsmm_diff(da + bytes - 255, db + bytes - 255, 255)
      || wanted != libxsmm_diff_n(key, da, ITEM, ITEM, 900, ITEMS) || wanted != libxsmm_diff_n(da + wanted * ITEM, da, ITEM, ITEM, 0, ITEMS)
      || ITEMS != libxsmm_diff_n(key, db, ITEM, ITEM, 0, ITEMS))
    {
      fprintf(stderr, "hash_caller: the device copies answer differently\n"); result = EXIT_FAILURE;
    }
    else printf("hash_caller: device copies agree\n");
    libxsmm_amd_device_free(da); libxsmm_amd_device_free(db);
  }
  if (EXIT_SUCCESS == result) printf("hash_caller: ok (hash %08x, found %u)\n", hash_a, found);
  free(a); free(b);
  libxsmm_finalize();
  return result;
}
