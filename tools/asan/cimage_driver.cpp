// Stand-alone sanitizer driver for the packed image of L~ of the K = 5 quad strips (csrc/cheb_tiles.hip: QStrip::img, cimg_rows;
// dsph_plan_strip_image): links the SANITIZER build of the library (`make -C deepsphere-cosmo-tf2_amd/csrc asan-cimage`: host
// code under AddressSanitizer + UBSan on the stub HIP runtime, device memory = host memory, launches dropped; no GPU) and has its
// own main: no interpreter, nothing preloaded.
//   cimage_driver CASE.ell ...        (the cases: tools/asan/dump_cimage_cases.py DIR, run WITHOUT a sanitizer)
// For every strip of every case, in both bases: the strip's rows are copied out of the image into a buffer of exactly their size
// -- a strip whose offset + rows passed the allocation would be a heap-buffer-overflow report --, the size must be
// (yhi - ylo + 8) x 576 floats (the rows ylo - 1 .. yhi + 6), and those rows must exist in the map (dsph_plan_strip_rows).
// Prints one line per case and "CIMAGE-DRIVER-OK"; any sanitizer report aborts the process.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dsphere.h"

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " [%s]\n", dsph_last_error()); exit(1); } } while (0)

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    REQUIRE(f, "cannot open %s", argv[a]);
    int64_t hdr[2];
    REQUIRE(fread(hdr, 8, 2, f) == 2, "%s: no header", argv[a]);
    const int64_t M = hdr[0], W = hdr[1];
    std::vector<int32_t> cols((size_t)(M * W));
    std::vector<float> vals((size_t)(M * W));
    REQUIRE(fread(cols.data(), 4, cols.size(), f) == cols.size() && fread(vals.data(), 4, vals.size(), f) == vals.size(), "%s: short", argv[a]);
    fclose(f);
    dsph_plan* h = nullptr;
    REQUIRE(dsph_plan_create(&h, M, M, (int32_t)W, cols.data(), vals.data(), 0) == DSPH_OK, "plan_create");
    REQUIRE(dsph_plan_set_option(h, DSPH_OPT_STRIPS, 1) == DSPH_OK && dsph_plan_set_option(h, DSPH_OPT_QSTRIP_IMAGE, 1) == DSPH_OK, "set_option");
    REQUIRE(dsph_plan_prepare_layer(h, 5, 64, 64, 0) == DSPH_OK, "prepare");
    int64_t n = 0;
    REQUIRE(dsph_plan_strip_pairs(h, 5, nullptr, 0, &n) == DSPH_OK, "strip_pairs");
    if (n == 0) {  // (a map too ragged for a rectangle: nothing to look at)
      printf("%s: %lld rows, no quad strips\n", argv[a], (long long)M);
      dsph_plan_destroy(h);
      continue;
    }
    std::vector<int32_t> rec((size_t)n * 12);
    REQUIRE(dsph_plan_strip_pairs(h, 5, rec.data(), n, &n) == DSPH_OK, "strip_pairs");
    int64_t floats = 0;
    for (int flip = 0; flip < 2; ++flip) {  // (the second round after the option went off and on again: freed and rebuilt)
      for (int64_t s = 0; s < n; ++s) {
        const int32_t* r = &rec[(size_t)s * 12];
        const int xlo = r[8], xhi = r[9], ylo = r[10], yhi = r[11];
        const int64_t want = (int64_t)(yhi - ylo + 8) * 576;
        for (int basis = 0; basis < 2; ++basis) {
          int64_t nf = 0;
          REQUIRE(dsph_plan_strip_image(h, basis, s, nullptr, 0, &nf) == DSPH_OK && nf == want, "%s: strip %lld: %lld floats, want %lld",
                  argv[a], (long long)s, (long long)nf, (long long)want);
          std::vector<float> img((size_t)nf);
          REQUIRE(dsph_plan_strip_image(h, basis, s, img.data(), nf, &nf) == DSPH_OK, "strip_image");
          floats += nf;
        }
        std::vector<int32_t> xy;
        for (int y : {ylo - 1, yhi + 6})
          for (int x = xlo; x <= xhi; ++x) { xy.push_back(x); xy.push_back(y); }
        std::vector<int64_t> rows(xy.size() / 2);
        REQUIRE(dsph_plan_strip_rows(h, 5, s, (int64_t)rows.size(), xy.data(), rows.data()) == DSPH_OK, "strip_rows");
        for (int64_t row : rows) REQUIRE(row >= 0 && row < M, "%s: strip %lld: image row %lld of %lld does not exist", argv[a], (long long)s, (long long)row, (long long)M);
      }
      REQUIRE(dsph_plan_set_option(h, DSPH_OPT_QSTRIP_IMAGE, 2) == DSPH_OK, "set_option off");
      int64_t nf = 0;
      REQUIRE(dsph_plan_strip_image(h, 0, 0, nullptr, 0, &nf) == DSPH_E_UNSUPPORTED, "an image with the option off");
      REQUIRE(dsph_plan_set_option(h, DSPH_OPT_QSTRIP_IMAGE, 1) == DSPH_OK, "set_option on");
    }
    printf("%s: %lld rows, %lld strips, %lld floats of image copied out, rows ylo - 1 .. yhi + 6 present\n", argv[a], (long long)M, (long long)n, (long long)floats);
    dsph_plan_destroy(h);
  }
  printf("CIMAGE-DRIVER-OK\n");
  return 0;
}
