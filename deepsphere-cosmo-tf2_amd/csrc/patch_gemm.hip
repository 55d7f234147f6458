// The pseudo-convolutions HealpyPseudoConv / HealpyPseudoConv_Transpose (reference healpy_layers.py:81-216: Conv1D and
// Conv2DTranspose with kernel = stride = 4^p on NEST-ordered maps) as ONE row GEMM with the bias and the activation in its store:
//     Y[r, c] = act( sum_j X[r, j] * W[j, c] + b[c mod P] ),   X (R, Kd), W (Kd, C), Y (R, C), b (P) or NULL      (include/dsphere.h)
// Both X views are free reshapes of the map (the 4^p children of a pixel are consecutive rows), so the layer reads its input once
// and writes its output once; W is tiny (at most 4^p * Fin * Fout floats).  The gradient of the epilogue is the second kernel here:
//     dZ = dY * act'(Y)  (from the stored output),   dbias[o] = sum_r sum_{c = o mod P} dZ[r, c]
// and the rest of the backward reuses what exists: dX = dZ W^T is this GEMM again, dW = X^T dZ is dsph_cheb_wgrad on one plane.
//
// gfx950 mapping of the GEMM (the layout of cheb_tcontract.hip, which it generalises to any contraction length):
//   * a wave owns 32 rows; lane = (row px, half g) loads 8 neighbouring floats of its row per 16-long slice of Kd -- two 16-byte
//     loads, straight into the B operand of v_mfma_f32_32x32x16_bf16, split to bf16 in registers (wf_contract of
//     dsphere_wfrag.h: exact fp32 on v_mfma_f32_32x32x2_f32, the six-term and the three-term bf16 split) -- four slices
//     in flight per lane.  No LDS round trip for the map.
//   * W goes through LDS as A-operand fragments, already split: [slice][32-column tile][term].  Where the whole image fits
//     (PG_LDS_MAX; every p = 1 layer up to 64 -> 64, p = 2 up to 32 -> 32) a workgroup builds it once and walks row groups
//     grid-stride; otherwise it is staged per row group in chunks of Kd for NB column tiles at a time (W up to 1,024 x 64 and more).
//   * the accumulators of NB = 1, 2 or 4 column tiles (32 x 32 fp32 each, lane = row) live in registers; where C has more tiles the
//     row is read again for the next NB (from L2: a row group is 8 x 32 rows).
//   * epilogue: bias by column mod P, apply_act, the only store of Y, 16 bytes per lane where C % 4 == 0 and y is aligned.
// Kd % 4 != 0 or x off 16-byte alignment: scalar loads of the same elements (vec_width of dsphere_mapops.h).
//
// Nothing here allocates, synchronises or reads the host: every launch goes on the caller's stream and is legal under capture.
#include <algorithm>

#include "dsphere_mapops.h"
#include "dsphere_wfrag.h"

namespace dsph {

namespace {

constexpr int PG_THREADS = 512;
constexpr int PG_WAVES = PG_THREADS / 64;
constexpr int PG_LDS_MAX = 96 * 1024;
constexpr int32_t PG_MAX_DIM = 4096;            // Kd and C
constexpr int64_t PG_MAX_ROWS = (int64_t)1 << 40;
constexpr int PG_MAX_GRID = 1024;               // workgroups of the GEMM: a constant, so the walk is the same on every device
constexpr int PG_BATCH = 4;                     // slices of a row a lane has in flight

constexpr int PE_THREADS = 256;
constexpr int64_t PE_MAX_PARTIALS = 2048;
constexpr int64_t PE_PARTIAL_ELEMS = 8192;      // elements of the map per partial, at least (until PE_MAX_PARTIALS)
constexpr int PE_ITEMS = 16;                    // floats of a period a thread holds at most (P <= 4096 = 256 threads x 16)

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct PatchArgs {
  const float* x; const float* w; const float* bias; float* y;
  int64_t R, ngroups;     // ngroups = ceil(R / (32 * PG_WAVES))
  int32_t Kd, C, P, act;
  int32_t nslices, ntiles;  // ceil(Kd / 16), ceil(C / 32)
  int32_t cs, tg;           // slices and column tiles per staging of W (resident: all of them)
  int32_t resident, vec_y;
};

// fragments of W rows [16 c0, 16 (c0 + nc)) x column tiles [t0, t0 + nt) -> LDS [slice][tile][term], the element order of
// wf_contract: (lane l, slot j) <- W[16 c + 8 (l >> 5) + j][32 t + (l & 31)], zero outside W
template <int PREC>
__device__ __forceinline__ void pg_stage(unsigned char* smem, const PatchArgs& a, int c0, int nc, int t0, int nt) {
  constexpr int LEVB = wf_terms(PREC) * wf_term_bytes(PREC);
  for (int e = threadIdx.x; e < nc * nt * WF_ELEMS; e += PG_THREADS) {
    const int blk = e / WF_ELEMS;
    const WfElem p = wf_elem32(e);
    const int t = blk % nt, c = blk / nt;
    // (a tile past the last one lies past column C: zero like every column there)
    wf_put<PREC>(smem + (size_t)blk * LEVB, p.l, p.j, wf_gather(a.w, 16 * (c0 + c) + p.inner, 32 * (t0 + t) + p.col, a.Kd, a.C, 1, 0, a.C));
  }
}

template <int PREC, int NB, bool VEC>  // VEC: Kd a multiple of four and x 16-byte aligned
__global__ __launch_bounds__(PG_THREADS) void patch_gemm_kernel(PatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pg_smem[];
  constexpr int LEVB = wf_terms(PREC) * wf_term_bytes(PREC);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px = lane & 31, g = lane >> 5;
  if (a.resident) {
    pg_stage<PREC>(pg_smem, a, 0, a.nslices, 0, a.ntiles);
    __syncthreads();
  }
  // (every wave of the workgroup walks the same groups: the barriers of the staged form are met by all of them)
  for (int64_t grp = blockIdx.x; grp < a.ngroups; grp += gridDim.x) {
    const int64_t m = (grp * PG_WAVES + wave) * 32 + px;
    const bool row_ok = m < a.R;
    const float* xrow = a.x + (row_ok ? m : 0) * (int64_t)a.Kd;
    for (int t0 = 0; t0 < a.ntiles; t0 += a.tg) {
      const int tend = t0 + a.tg < a.ntiles ? t0 + a.tg : a.ntiles;
      for (int nb0 = t0; nb0 < tend; nb0 += NB) {
        sp_f32x16 acc[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
        for (int c0 = 0; c0 < a.nslices; c0 += a.cs) {
          const int nc = c0 + a.cs < a.nslices ? a.cs : a.nslices - c0;
          if (!a.resident) {
            __syncthreads();  // (the fragments of the last staging have been read)
            pg_stage<PREC>(pg_smem, a, c0, nc, t0, a.tg);
            __syncthreads();
          }
          for (int cb = 0; cb < nc; cb += PG_BATCH) {
            float row[PG_BATCH][8];
#pragma unroll
            for (int u = 0; u < PG_BATCH; ++u) {
              const int ch = 16 * (c0 + cb + u) + 8 * g;
              const bool live = row_ok && cb + u < nc;
              if (VEC) {
                const sp_f32x4 v0 = (live && ch < a.Kd) ? *reinterpret_cast<const sp_f32x4*>(xrow + ch) : sp_f32x4{0.f, 0.f, 0.f, 0.f};
                const sp_f32x4 v1 = (live && ch + 4 < a.Kd) ? *reinterpret_cast<const sp_f32x4*>(xrow + ch + 4) : sp_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j) { row[u][j] = v0[j]; row[u][4 + j] = v1[j]; }
              } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) row[u][j] = (live && ch + j < a.Kd) ? xrow[ch + j] : 0.f;
              }
            }
#pragma unroll
            for (int u = 0; u < PG_BATCH; ++u) {
              if (cb + u < nc) {
#pragma unroll
                for (int q = 0; q < NB; ++q)
                  if (nb0 + q < tend)
                    wf_contract<8, PREC, false>(acc[q], row[u], pg_smem + (size_t)((cb + u) * a.tg + (nb0 - t0) + q) * LEVB, lane);
              }
            }
          }
        }
        // accumulator tile: lane = row, element 4 tq + e = column 8 tq + 4 g + e of the tile
#pragma unroll
        for (int q = 0; q < NB; ++q) {
          if (nb0 + q >= tend || !row_ok) continue;
          float* dst = a.y + m * (int64_t)a.C + 32 * (nb0 + q);
#pragma unroll
          for (int tq = 0; tq < 4; ++tq) {
            const int o = 8 * tq + 4 * g, oc = 32 * (nb0 + q) + o;
            if (oc >= a.C) continue;
            float r[4];
            int bc = oc % a.P;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              r[e] = apply_act(acc[q][4 * tq + e] + (a.bias != nullptr ? a.bias[bc] : 0.f), a.act);
              bc = bc + 1 == a.P ? 0 : bc + 1;
            }
            if (a.vec_y && oc + 3 < a.C) *reinterpret_cast<sp_f32x4*>(dst + o) = sp_f32x4{r[0], r[1], r[2], r[3]};
            else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (oc + e < a.C) dst[o + e] = r[e];
            }
          }
        }
      }
    }
  }
}

// -- the epilogue's gradient.  The (R, C) map is (R C / P) rows of one bias period: L = min(256, 2^ceil(log2(P / VEC))) threads share
//    a period row, thread j of them owning the vectors j, j + L, ..; a workgroup holds 256 / L period rows per step and walks the
//    steps grid-stride.  Column sums in float64: registers, then the threads of a column through LDS in a fixed order, one
//    partial per workgroup and column; the merge kernel adds the partials in a fixed order. -------------------------------------------
struct EpiGeo {
  int64_t prow, nsteps;  // period rows R C / P, ceil(prow / rpb)
  int32_t P, nv, L, lshift, rpb, npl;
};

template <int VEC>
__global__ __launch_bounds__(PE_THREADS) void patch_epilogue_bwd_kernel(const float* __restrict__ y, const float* dy, float* dz, double* __restrict__ part,
                                                                        int want_part, int act, EpiGeo g) {
  constexpr int NI = PE_ITEMS / VEC;
  __shared__ double lds[PE_THREADS];
  const int sub = (int)threadIdx.x & (g.L - 1), slot = (int)threadIdx.x >> g.lshift;
  double acc[NI][VEC];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[i][e] = 0.0;
  for (int64_t step = blockIdx.x; step < g.nsteps; step += gridDim.x) {
    const int64_t row = step * g.rpb + slot;
    if (row >= g.prow) continue;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int cv = i * g.L + sub;
      if (i < g.npl && cv < g.nv) {
        const int64_t o = row * g.P + (int64_t)cv * VEC;
        float d[VEC], yy[VEC];
        ldv<VEC>(dy + o, d);
        if (act != DSPH_ACT_NONE) {
          ldv<VEC>(y + o, yy);
#pragma unroll
          for (int e = 0; e < VEC; ++e) d[e] *= act_grad(yy[e], act);
        }
        if (act != DSPH_ACT_NONE || dz != dy) stv<VEC>(dz + o, d);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[i][e] += (double)d[e];
      }
    }
  }
  if (!want_part) return;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      if (i >= g.npl) continue;  // (uniform over the workgroup: so are the barriers)
      __syncthreads();
      lds[threadIdx.x] = acc[i][e];
      __syncthreads();
      const int cv = i * g.L + sub;
      if (slot == 0 && cv < g.nv) {
        double s = acc[i][e];
        for (int t = 1; t < g.rpb; ++t) s += lds[t * g.L + sub];
        part[(int64_t)blockIdx.x * g.P + (int64_t)cv * VEC + e] = s;
      }
    }
  }
}

// workgroups of the epilogue's backward = partials per bias element: of the shape alone
inline int64_t pe_partials(int64_t R, int32_t C) {
  const int64_t p = ceil_div(R * (int64_t)C, PE_PARTIAL_ELEMS);
  return p > PE_MAX_PARTIALS ? PE_MAX_PARTIALS : (p < 1 ? 1 : p);
}

EpiGeo pe_geo(int64_t R, int32_t C, int32_t P, int vec) {
  EpiGeo g;
  g.P = P;
  g.prow = R * (int64_t)(C / P);
  g.nv = P / vec;
  g.L = 1;
  g.lshift = 0;
  while (g.L < g.nv && g.L < PE_THREADS) { g.L <<= 1; ++g.lshift; }
  g.rpb = PE_THREADS / g.L;
  g.npl = (g.nv + g.L - 1) / g.L;
  g.nsteps = ceil_div(g.prow, g.rpb);
  return g;
}

// R, Kd (0: not part of the call), C, P of either entry point
bool patch_shape_ok(const char* who, int64_t R, int32_t Kd, int32_t C, int32_t P, int* rc) {
  if (R < 1 || Kd < 0 || C < 1 || P < 1) {
    set_error("%s: R = %lld, Kd = %d, C = %d, P = %d: every one must be at least 1", who, (long long)R, (int)Kd, (int)C, (int)P);
    *rc = DSPH_E_BADARG;
    return false;
  }
  if (C % P != 0) {
    set_error("%s: C = %d is not a multiple of the bias period P = %d", who, (int)C, (int)P);
    *rc = DSPH_E_BADARG;
    return false;
  }
  if (R > PG_MAX_ROWS || Kd > PG_MAX_DIM || C > PG_MAX_DIM) {
    set_error("%s: R = %lld, Kd = %d, C = %d: at most 2^40 rows, Kd and C in [1, %d]", who, (long long)R, (int)Kd, (int)C, (int)PG_MAX_DIM);
    *rc = DSPH_E_UNSUPPORTED;
    return false;
  }
  return true;
}

bool act_ok(int32_t act) { return act >= DSPH_ACT_NONE && act <= DSPH_ACT_TANH; }

}  // namespace

}  // namespace dsph

#define PG_LAUNCH(PREC, NBV)                                                                                                        \
  do {                                                                                                                              \
    if (vec_x) hipLaunchKernelGGL((patch_gemm_kernel<PREC, NBV, true>), dim3(grid), dim3(PG_THREADS), lds, stream, a);               \
    else hipLaunchKernelGGL((patch_gemm_kernel<PREC, NBV, false>), dim3(grid), dim3(PG_THREADS), lds, stream, a);                    \
  } while (0)
#define PG_LAUNCH_NB(PREC)                                                                                                          \
  do {                                                                                                                              \
    if (nb == 4) PG_LAUNCH(PREC, 4);                                                                                                \
    else if (nb == 2) PG_LAUNCH(PREC, 2);                                                                                           \
    else PG_LAUNCH(PREC, 1);                                                                                                        \
  } while (0)

extern "C" {

// every argument is checked here, before any HIP call
int dsph_patch_gemm(const float* x, const float* w, const float* bias, float* y, int64_t R, int32_t Kd, int32_t C, int32_t P, int32_t act,
                    int32_t precision, int device, void* hip_stream) {
  using namespace dsph;
  int rc = DSPH_OK;
  if (!x || !w || !y) { set_error("patch_gemm: NULL pointer (x, w and y are required)"); return DSPH_E_BADARG; }
  if (Kd < 1) { set_error("patch_gemm: Kd = %d must be at least 1", (int)Kd); return DSPH_E_BADARG; }
  if (!patch_shape_ok("patch_gemm", R, Kd, C, P, &rc)) return rc;
  if (!act_ok(act)) { set_error("patch_gemm: unknown activation code %d", (int)act); return DSPH_E_BADARG; }
  if (precision < DSPH_PREC_FP32 || precision > DSPH_PREC_F16X3) { set_error("patch_gemm: unknown precision code %d", (int)precision); return DSPH_E_BADARG; }
  const size_t xb = (size_t)R * Kd * sizeof(float), yb = (size_t)R * C * sizeof(float), wb = (size_t)Kd * C * sizeof(float);
  if (ranges_overlap(y, yb, x, xb) || ranges_overlap(y, yb, w, wb)) { set_error("patch_gemm: y overlaps x or w"); return DSPH_E_BADARG; }
  if (precision == DSPH_PREC_F16X3) precision = DSPH_PREC_BF16X6;  // (no scale rule here: the fp32-equivalent split that needs none)

  PatchArgs a;
  a.x = x; a.w = w; a.bias = bias; a.y = y;
  a.R = R; a.Kd = Kd; a.C = C; a.P = P; a.act = act;
  a.ngroups = ceil_div(R, 32 * PG_WAVES);
  a.nslices = (Kd + 15) / 16;
  a.ntiles = (C + 31) / 32;
  const int nb = a.ntiles >= 4 ? 4 : (a.ntiles >= 2 ? 2 : 1);
  const size_t levb = (size_t)wf_terms(precision) * wf_term_bytes(precision);
  size_t lds = (size_t)a.nslices * a.ntiles * levb;
  a.resident = lds <= (size_t)PG_LDS_MAX;
  if (a.resident) {
    a.cs = a.nslices;
    a.tg = a.ntiles;
  } else {
    a.tg = nb;
    a.cs = (int32_t)std::min<size_t>((size_t)a.nslices, (size_t)PG_LDS_MAX / ((size_t)nb * levb));
    a.cs = std::max<int32_t>(PG_BATCH, a.cs / PG_BATCH * PG_BATCH);
    lds = (size_t)a.cs * a.tg * levb;
  }
  const bool vec_x = vec_width(Kd, ptr_bits({x}), false) == 4;
  a.vec_y = vec_width(C, ptr_bits({y}), false) == 4;
  const int grid = (int)std::min<int64_t>(a.ngroups, PG_MAX_GRID);
  DeviceGuard guard(device);
  if (!select_device("patch_gemm", device, guard)) return DSPH_E_BADARG;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (precision == DSPH_PREC_FP32) PG_LAUNCH_NB(DSPH_PREC_FP32);
  else if (precision == DSPH_PREC_BF16X6) PG_LAUNCH_NB(DSPH_PREC_BF16X6);
  else PG_LAUNCH_NB(DSPH_PREC_BF16X3);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

size_t dsph_patch_backward_workspace_bytes(int64_t R, int32_t C, int32_t P) {
  using namespace dsph;
  if (R < 1 || C < 1 || P < 1 || C % P != 0 || R > PG_MAX_ROWS || C > PG_MAX_DIM) return 0;
  return (size_t)pe_partials(R, C) * (size_t)P * sizeof(double);
}

int dsph_patch_epilogue_backward(const float* y, const float* dy, float* dz, float* dbias, int64_t R, int32_t C, int32_t P, int32_t act,
                                 void* workspace, size_t workspace_bytes, int device, void* hip_stream) {
  using namespace dsph;
  int rc = DSPH_OK;
  if (!dy || !dz) { set_error("patch_epilogue_backward: NULL pointer (dy and dz are required)"); return DSPH_E_BADARG; }
  if (!patch_shape_ok("patch_epilogue_backward", R, 0, C, P, &rc)) return rc;
  if (!act_ok(act)) { set_error("patch_epilogue_backward: unknown activation code %d", (int)act); return DSPH_E_BADARG; }
  if (act != DSPH_ACT_NONE && !y) { set_error("patch_epilogue_backward: y is NULL (the activation's derivative is taken from it)"); return DSPH_E_BADARG; }
  const size_t mb = (size_t)R * C * sizeof(float);
  if ((y && ranges_overlap(dz, mb, y, mb)) || (dz != dy && ranges_overlap(dz, mb, dy, mb))) {
    set_error("patch_epilogue_backward: dz overlaps y, or dy without being dy (in place means the same pointer)");
    return DSPH_E_BADARG;
  }
  const int64_t NP = pe_partials(R, C);
  if (dbias) {
    if (!workspace) { set_error("patch_epilogue_backward: workspace is NULL (dbias is reduced through it)"); return DSPH_E_BADARG; }
    if (!workspace_ok("patch_epilogue_backward", workspace, workspace_bytes, (size_t)NP * P * sizeof(double), &rc)) return rc;
  }
  const int vec = vec_width(P, ptr_bits({act != DSPH_ACT_NONE ? y : nullptr, dy, dz}), false);
  const EpiGeo g = pe_geo(R, C, P, vec);
  double* part = static_cast<double*>(workspace);
  DeviceGuard guard(device);
  if (!select_device("patch_epilogue_backward", device, guard)) return DSPH_E_BADARG;
  hipStream_t stream = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)NP), block(PE_THREADS);
  if (vec == 4) hipLaunchKernelGGL((patch_epilogue_bwd_kernel<4>), grid, block, 0, stream, y, dy, dz, part, dbias ? 1 : 0, (int)act, g);
  else hipLaunchKernelGGL((patch_epilogue_bwd_kernel<1>), grid, block, 0, stream, y, dy, dz, part, dbias ? 1 : 0, (int)act, g);
  DSPH_HIP(hipGetLastError());
  if (dbias) {
    hipLaunchKernelGGL(partials_merge_kernel<1>, merge_grid(P, 1), dim3(MERGE_THREADS), 0, stream, (const double*)part, NP, (int64_t)P, (int64_t)0, P,
                       dbias, (float*)nullptr);
    DSPH_HIP(hipGetLastError());
  }
  return DSPH_OK;
}

}  // extern "C"

#undef PG_LAUNCH
#undef PG_LAUNCH_NB
