// Host program: the weight-fragment writers of csrc/dsphere_wfrag.h, run on the CPU (tests/test_wfrag_host.py).
//   hipcc --offload-host-only -I include -I deepsphere-cosmo-tf2_amd/csrc tools/wfrag_image.hip -o wfrag_image
//   wfrag_image CASES IMAGES
// CASES is a sequence of records: twelve int32 {geometry (32 | 16), form, Fin, Fout, K, k, ld, pack, slices, blocks, rows, 0}, one float
// (the scale), then the rows x ld float32 matrix.  For every record, IMAGES receives slices x blocks fragment groups (slice-major):
// element (l, j) of group (c, nb) <- the gather at channel  SLICE c + inner, column  COLS nb + col  (SLICE, COLS = 16, 32 or 32, 16 by
// geometry; `pack` != 0: the block-diagonal gather, scale unused), written by wf_put in the record's form.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dsphere_wfrag.h"

using namespace dsph;

static int group_bytes(int form) { return form == WF_BF16X6 ? 3 * WF_FRAG : 2 * WF_FRAG; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s CASES IMAGES\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "wfrag_image: cannot open the files\n"); return 2; }
  int32_t h[12];
  while (fread(h, sizeof(int32_t), 12, in) == 12) {
    const int geo = h[0], form = h[1], Fin = h[2], Fout = h[3], K = h[4], k = h[5], ld = h[6], pack = h[7], C = h[8], NB = h[9], rows = h[10];
    float sc;
    std::vector<float> w((size_t)rows * ld);
    if (fread(&sc, sizeof(float), 1, in) != 1 || fread(w.data(), sizeof(float), w.size(), in) != w.size()) { fprintf(stderr, "wfrag_image: short record\n"); return 2; }
    if ((geo != 32 && geo != 16) || form < 0 || form > WF_FP32_HALVES) { fprintf(stderr, "wfrag_image: geometry %d, form %d\n", geo, form); return 2; }
    const int slice = geo == 32 ? 16 : 32, cols = geo == 32 ? 32 : 16;
    std::vector<unsigned char> img((size_t)C * NB * group_bytes(form), 0xa5);  // (every byte of a group is written: none of these survive)
    for (int c = 0; c < C; ++c)
      for (int nb = 0; nb < NB; ++nb) {
        unsigned char* base = img.data() + (size_t)(c * NB + nb) * group_bytes(form);
        for (int e = 0; e < WF_ELEMS; ++e) {
          const WfElem p = geo == 32 ? wf_elem32(e) : wf_elem16(e);
          const int ch = slice * c + p.inner, col = cols * nb + p.col;
          const float v = pack ? wf_gather_pack(w.data(), ch, col, Fin, Fout, K, k, ld, pack) : wf_gather(w.data(), ch, col, Fin, Fout, K, k, ld, sc);
          wf_put(base, form, p.l, p.j, v);
        }
      }
    if (fwrite(img.data(), 1, img.size(), out) != img.size()) { fprintf(stderr, "wfrag_image: write failed\n"); return 2; }
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
