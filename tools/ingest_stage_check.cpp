// Stand-alone check of the ingest kernel's row staging (csrc/ita_ingest_kernel.h: ita_ingest_stage_load / _store) on the
// CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.  The two functions decide which bytes of a source row a
// lane loads (single pixels at a misaligned head and tail, 16-byte pieces between) and where they land in the LDS image;
// here the 64 lanes of a wave are run one after the other over rows of every width class and every alignment, and the
// LDS image lies in an allocation of exactly its size.  Behind the row: it ends at the end of its allocation, so ASan's
// red zone starts at the byte after its last pixel -- a load past the row aborts, at any alignment.  In front of the row:
// a 16-byte pad and the part of the misalignment that fills whole 8-byte shadow granules are poisoned; ASan cannot
// poison the leading bytes of a granule, so the up to 7 bytes directly in front of a row that does not start on an
// 8-byte boundary are NOT watched (rows at misalignment 0 and 8 are watched to the byte).  A 16-byte load that started
// in those bytes would be a misaligned one, which UBSan aborts on; a single-pixel load cannot reach them (its index is
// a lane number >= 0).  A store outside the image aborts likewise, and the staged image is then compared with the row
// pixel by pixel.  Host code only: no GPU call is made.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/ingest_stage_check.cpp -o /tmp/ingest_stage_check && /tmp/ingest_stage_check
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../drone-oa-iree-vit-accelerator_amd/csrc/ita_ingest_kernel.h"

template <typename T>
static long check_width(int W) {
  constexpr int PS = (int)sizeof(T);
  const int nb = W * PS;
  long rows = 0;
  for (int mis = 0; mis < 16; mis += PS) {
    // [16-aligned base | 16-byte pad + mis bytes, poisoned as far as whole granules go | the row | ASan's red zone]
    const int front = 16 + mis, watched = front & ~7;
    void* base = nullptr;
    if (posix_memalign(&base, 16, (size_t)front + nb)) abort();
    unsigned char* bytes = static_cast<unsigned char*>(base);
    for (int i = 0; i < front + nb; ++i) bytes[i] = (unsigned char)(i * 131 + W * 7 + mis + 1);
    ASAN_POISON_MEMORY_REGION(bytes, watched);
    const T* row = reinterpret_cast<const T*>(bytes + front);
    const int lds_bytes = ita_ingest_row_lds(nb);
    void* lds = nullptr;
    if (posix_memalign(&lds, 16, (size_t)lds_bytes)) abort();
    memset(lds, 0xEE, lds_bytes);
    static ItaIngestStage<T> st[64];
    for (int lane = 0; lane < 64; ++lane) ita_ingest_stage_load(st[lane], row, W, lane);
    for (int lane = 0; lane < 64; ++lane) ita_ingest_stage_store(st[lane], static_cast<unsigned char*>(lds), lane);
    if (st[0].mis != mis || st[0].nh * PS + st[0].nbody * 16 + st[0].nt * PS != nb || st[0].nbody > 256) {
      fprintf(stderr, "bad split: W %d pixel %d mis %d -> head %d body %d tail %d\n", W, PS, mis, st[0].nh, st[0].nbody, st[0].nt);
      exit(1);
    }
    if (memcmp(static_cast<unsigned char*>(lds) + mis, row, nb)) {
      fprintf(stderr, "staged image differs from the row: W %d pixel %d mis %d\n", W, PS, mis);
      exit(1);
    }
    ASAN_UNPOISON_MEMORY_REGION(bytes, watched);
    free(base);
    free(lds);
    ++rows;
  }
  return rows;
}

template <typename T>
static long check_type() {
  const int wmax = ITA_INGEST_ROW_BYTES / (int)sizeof(T);
  long rows = 0;
  for (int W = 1; W <= 700 && W <= wmax; ++W) rows += check_width<T>(W);
  for (int W = wmax - 40; W <= wmax; ++W) rows += check_width<T>(W);
  return rows;
}

int main() {
#if !defined(__has_feature) || !__has_feature(address_sanitizer)
  fprintf(stderr, "built without AddressSanitizer: the bounds are not being checked\n");
  return 2;
#else
  const long rows = check_type<uint8_t>() + check_type<uint16_t>() + check_type<float>();
  printf("ingest staging: %ld rows staged inside their bounds, images equal\n", rows);
  return 0;
#endif
}
