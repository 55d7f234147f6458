// Layer normalisation over the trailing axis of channels-last maps (rows = N * M, d) fp32, the residual add in front of it fused:
//     a = x + res (written out as `sum`),   z = (a - mean) * rstd * gamma + beta,   mean, var per ROW (plan-free; include/dsphere.h).
// Replaces the host framework's LayerNorm and the add before it in the transformer blocks (reference gnn_transformers.py:149-245)
// and GCNN_ResidualLayer's norm_type="layer_norm" (reference gnn_layers.py:373-374), forward and backward.
//
// Passes over the map: forward reads x (and res) once and writes z (and sum) once, in ONE launch; backward reads a, dz (and dsum)
// once and writes da once in one launch that also leaves the parameter gradients' partials, and a second launch merges those.
// mean, rstd and x^ are recomputed from `a` in the backward (the row is being read anyway): nothing row- or map-sized is kept
// between the two calls and no rounded statistic comes back in.  Everything is bound by memory, so the work is laid out for the loads:
//
//   * A row lives in registers.  A lane owns VEC neighbouring channels per item (VEC = 4: one 16-byte access, where d % 4 == 0 and
//     every map of the call is 16-byte aligned; else 1) -- nv = d / VEC column vectors per row.  L = min(64, 2^ceil(log2 nv))
//     lanes of a wave share a row, lane j of them owning the vectors j, j + L, j + 2 L, .. (NPL = ceil(nv / L) of them, 1 .. 4
//     vectors or 1 .. 16 scalars: d <= 1024); a wave holds 64 / L rows, a workgroup of four waves 256 / L.  Neighbouring lanes
//     read neighbouring addresses for every d, and with L < 64 the rows of a wave follow each other without a gap.
//   * The row sums run through a shuffle butterfly among the L lanes: no LDS, every lane of the row ends with the same bits.
//   * Row groups (256 / L rows) are dealt to the workgroups grid-stride; the grid is a function of (rows, d) alone and bounded.
//     Row numbers and element offsets are 64-bit.
//   * Arithmetic: never E[a^2] - E[a]^2 -- the mean, then the centred sum of squares, both from the registers.  Row scalars (mean,
//     variance, rstd, the backward's two row means), x^ and the column partials are float64: at d = 2, x^ = +-(1 - e) and da is a
//     cancellation that one fp32 rounding of mean or rstd swamps (the reason batch_norm.hip gives for its smallest batch), and a
//     row of mean 10 loses the same digits.
//   * Parameter gradients by the batch-norm scheme: the P = ln_partials(rows, d) workgroups of the backward each leave one float64
//     partial per channel in the caller's workspace (lanes of a wave that share a column by shuffles, the four waves through LDS
//     in a fixed order), the second launch merges the P partials in a fixed order.  No atomics, one writer per word: two runs on
//     the same input give the same bits.
//
// Nothing here allocates, synchronises or reads the host: every launch goes on the caller's stream and is legal under capture.
#include "dsphere_mapops.h"

namespace dsph {

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_WAVES = LN_THREADS / 64;
constexpr int32_t LN_MAX_D = 1024;
constexpr int64_t LN_MAX_PARTIALS = 2048;
constexpr int64_t LN_PARTIAL_ELEMS = 8192;  // elements of the map per partial, at least (until LN_MAX_PARTIALS is reached)
constexpr int64_t LN_FWD_ELEMS = 4096;      // elements of the map per workgroup of the forward, at least (until LN_MAX_GRID)
constexpr int64_t LN_MAX_GRID = 8192;
constexpr int64_t LN_MAX_ROWS = (int64_t)1 << 40;

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Workgroups of the backward = partials per channel: the documented function of (rows, d) alone.  (A workgroup takes at least
// four rows per step, so more than ceil(rows / 4) of them would have nothing to do.)
inline int64_t ln_partials(int64_t rows, int32_t d) {
  int64_t p = ceil_div(rows * d, LN_PARTIAL_ELEMS);
  if (p > LN_MAX_PARTIALS) p = LN_MAX_PARTIALS;
  if (p > ceil_div(rows, LN_WAVES)) p = ceil_div(rows, LN_WAVES);
  return p < 1 ? 1 : p;
}
inline size_t ln_workspace_bytes(int64_t rows, int32_t d) { return (size_t)(2 * ln_partials(rows, d)) * (size_t)d * sizeof(double); }
// workgroups of the forward, of (rows, d) alone as well
inline int64_t ln_fwd_grid(int64_t rows, int32_t d) {
  int64_t g = ceil_div(rows * d, LN_FWD_ELEMS);
  if (g > LN_MAX_GRID) g = LN_MAX_GRID;
  if (g > ceil_div(rows, LN_WAVES)) g = ceil_div(rows, LN_WAVES);
  return g < 1 ? 1 : g;
}

// how a launch walks the map
struct LnGeo {
  int64_t rows, ngroups;  // ngroups = ceil(rows / rpb)
  int32_t d, nv;          // nv = d / VEC
  int32_t L, lshift;      // lanes per row = 1 << lshift
  int32_t rpw, rpb;       // rows per wave (64 / L) and per workgroup step
  double inv_d;
};

// sum over the L lanes that share a row; every one of them gets the same bits.  Called by all 64 lanes of the wave.
__device__ __forceinline__ double row_sum(double v, int L) {
  for (int off = L >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// this lane's place: which row of a workgroup step, which vectors of the row
struct LnLane {
  int sub, slot;
};
__device__ __forceinline__ LnLane ln_lane(const LnGeo& g) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  LnLane l;
  l.sub = lane & (g.L - 1);
  l.slot = wave * g.rpw + (lane >> g.lshift);
  return l;
}

// mean and rstd of the row whose elements the L lanes hold in a[][] (0 where masked), in float64 by the two-pass formula
template <int VEC, int NPL>
__device__ __forceinline__ void row_stats(const float (&a)[NPL][VEC], const bool (&on)[NPL], const LnGeo& g, double eps, double& mean, double& rstd) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NPL; ++i)
#pragma unroll
    for (int e = 0; e < VEC; ++e) s += (double)a[i][e];
  mean = row_sum(s, g.L) / (double)g.d;  // (a division: the mean of a constant row is that constant exactly, so z = beta there)
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < NPL; ++i)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double c = (double)a[i][e] - mean;
      q = on[i] ? fma(c, c, q) : q;
    }
  rstd = 1.0 / sqrt(row_sum(q, g.L) * g.inv_d + eps);
}

// row groups a workgroup has in flight per step: two where a lane holds one vector or up to four scalars of a row (its loads
// of the second group do not wait for the first one's butterfly), one where the row itself fills the registers
template <int VEC, int NPL> constexpr int ln_unroll() { return NPL * VEC <= 4 ? 2 : 1; }

// -- forward: a = x + res -> sum, z = (a - mean) * rstd * gamma + beta; sum may be x or res (a lane reads its elements first) -------
template <int VEC, int NPL>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_kernel(const float* x, const float* res, float* sum, float* __restrict__ z,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, double eps,
                                                             LnGeo g) {
  constexpr int U = ln_unroll<VEC, NPL>();
  const LnLane l = ln_lane(g);
  bool on[NPL];
  float ga[NPL][VEC], be[NPL][VEC];
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int cv = i * g.L + l.sub;
    on[i] = cv < g.nv;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      ga[i][e] = on[i] && gamma ? gamma[cv * VEC + e] : 1.f;
      be[i][e] = on[i] && beta ? beta[cv * VEC + e] : 0.f;
    }
  }
  for (int64_t grp0 = blockIdx.x; grp0 < g.ngroups; grp0 += (int64_t)gridDim.x * U) {
    float a[U][NPL][VEC];
    bool live[U];
    int64_t base[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = (grp0 + (int64_t)u * gridDim.x) * g.rpb + l.slot;  // (a group past the last one: rows past the last one)
      live[u] = row < g.rows;
      base[u] = row * g.d;
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        if (live[u] && on[i]) {
          ldv<VEC>(x + base[u] + (int64_t)(i * g.L + l.sub) * VEC, a[u][i]);
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) a[u][i][e] = 0.f;
        }
      }
    }
    if (res) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
          if (live[u] && on[i]) {
            const int64_t o = base[u] + (int64_t)(i * g.L + l.sub) * VEC;
            float r[VEC];
            ldv<VEC>(res + o, r);
#pragma unroll
            for (int e = 0; e < VEC; ++e) a[u][i][e] += r[e];
            stv<VEC>(sum + o, a[u][i]);
          }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double mean, rstd;
      row_stats<VEC, NPL>(a[u], on, g, eps, mean, rstd);
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        if (live[u] && on[i]) {
          float out[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) out[e] = (float)fma(((double)a[u][i][e] - mean) * rstd, (double)ga[i][e], (double)be[i][e]);
          stv<VEC>(z + base[u] + (int64_t)(i * g.L + l.sub) * VEC, out);
        }
      }
    }
  }
}

// -- backward, first launch: da = rstd * (g - mean_d(g) - x^ mean_d(g x^)) + dsum, g = dz * gamma; and per workgroup p
//    part[p][0][c] = sum dz, part[p][1][c] = sum dz x^ over the rows it walked (want_part) ---------------------------------------
template <int VEC, int NPL>
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_kernel(const float* __restrict__ a_in, const float* __restrict__ dz_in,
                                                             const float* __restrict__ dsum, const float* __restrict__ gamma, double eps,
                                                             float* __restrict__ da, double* __restrict__ part, int want_part, LnGeo g) {
  constexpr int U = ln_unroll<VEC, NPL>();
  __shared__ double lds[LN_WAVES - 1][2 * VEC][64];
  const LnLane l = ln_lane(g);
  bool on[NPL];
  float ga[NPL][VEC];
  double pb[NPL][VEC], pg[NPL][VEC];
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int cv = i * g.L + l.sub;
    on[i] = cv < g.nv;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      ga[i][e] = on[i] && gamma ? gamma[cv * VEC + e] : 1.f;
      pb[i][e] = pg[i][e] = 0.0;
    }
  }
  for (int64_t grp0 = blockIdx.x; grp0 < g.ngroups; grp0 += (int64_t)gridDim.x * U) {
    float a[U][NPL][VEC], dz[U][NPL][VEC];
    bool live[U];
    int64_t base[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = (grp0 + (int64_t)u * gridDim.x) * g.rpb + l.slot;
      live[u] = row < g.rows;
      base[u] = row * g.d;
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const int64_t o = base[u] + (int64_t)(i * g.L + l.sub) * VEC;
        if (live[u] && on[i]) {
          ldv<VEC>(a_in + o, a[u][i]);
          ldv<VEC>(dz_in + o, dz[u][i]);
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) a[u][i][e] = dz[u][i][e] = 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double mean, rstd;
      row_stats<VEC, NPL>(a[u], on, g, eps, mean, rstd);
      double xh[NPL][VEC], s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int i = 0; i < NPL; ++i)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          xh[i][e] = on[i] ? ((double)a[u][i][e] - mean) * rstd : 0.0;
          const double gv = (double)dz[u][i][e] * (double)ga[i][e];
          s1 += gv;
          s2 = fma(gv, xh[i][e], s2);
        }
      const double m1 = row_sum(s1, g.L) * g.inv_d, m2 = row_sum(s2, g.L) * g.inv_d;
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        if (live[u] && on[i]) {
          const int64_t o = base[u] + (int64_t)(i * g.L + l.sub) * VEC;
          float ds[VEC], out[VEC];
          if (dsum) {
            ldv<VEC>(dsum + o, ds);
          } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) ds[e] = 0.f;
          }
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const double gv = (double)dz[u][i][e] * (double)ga[i][e];
            out[e] = (float)fma(rstd, gv - m1 - xh[i][e] * m2, (double)ds[e]);
            pb[i][e] += (double)dz[u][i][e];
            pg[i][e] = fma((double)dz[u][i][e], xh[i][e], pg[i][e]);
          }
          stv<VEC>(da + o, out);
        }
      }
    }
  }
  if (!want_part) return;
  // lanes of the wave that share a column (sub, sub + L, ..) -> the lanes below L; then the four waves through LDS, in a fixed order
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    for (int off = 32; off >= g.L; off >>= 1) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        pb[i][e] += __shfl_down(pb[i][e], off, 64);  // (meaningful in the lanes below `off`; the others' results are not read)
        pg[i][e] += __shfl_down(pg[i][e], off, 64);
      }
    }
    __syncthreads();
    if (wave > 0 && lane < g.L) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        lds[wave - 1][e][lane] = pb[i][e];
        lds[wave - 1][VEC + e][lane] = pg[i][e];
      }
    }
    __syncthreads();
    if (wave == 0 && lane < g.L && on[i]) {
      double* out = part + (int64_t)blockIdx.x * 2 * g.d + (int64_t)(i * g.L + lane) * VEC;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        double b = pb[i][e], gm = pg[i][e];
        for (int w = 0; w < LN_WAVES - 1; ++w) {
          b += lds[w][e][lane];
          gm += lds[w][VEC + e][lane];
        }
        out[e] = b;
        out[g.d + e] = gm;
      }
    }
  }
}

LnGeo ln_geo(int64_t rows, int32_t d, int vec) {
  LnGeo g;
  g.rows = rows;
  g.d = d;
  g.nv = d / vec;
  g.L = 1;
  g.lshift = 0;
  while (g.L < g.nv && g.L < 64) { g.L <<= 1; ++g.lshift; }
  g.rpw = 64 / g.L;
  g.rpb = LN_WAVES * g.rpw;
  g.ngroups = ceil_div(rows, g.rpb);
  g.inv_d = 1.0 / (double)d;
  return g;
}
// items per lane, rounded up to the power of two a kernel is instantiated for
int ln_npl(const LnGeo& g) {
  const int n = (g.nv + g.L - 1) / g.L;
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// do two maps of the call share a byte (an optional map that is not given shares none)
inline bool overlap(const void* p, const void* q, int64_t rows, int32_t d) {
  const size_t bytes = (size_t)rows * (size_t)d * sizeof(float);
  return p && q && ranges_overlap(p, bytes, q, bytes);
}

// rows >= 0 (0: nothing to do), 1 <= d <= 1024
bool ln_shape_ok(const char* who, int64_t rows, int32_t d, int* rc) {
  if (rows < 0 || d < 1 || d > LN_MAX_D) {
    set_error("%s: rows = %lld, d = %d: rows must not be negative and d must lie in [1, %d]", who, (long long)rows, (int)d, (int)LN_MAX_D);
    *rc = DSPH_E_BADARG;
    return false;
  }
  if (rows > LN_MAX_ROWS) {
    set_error("%s: rows = %lld: more than 2^40 rows", who, (long long)rows);
    *rc = DSPH_E_UNSUPPORTED;
    return false;
  }
  return true;
}

}  // namespace

}  // namespace dsph

// (VEC, NPL) pairs the kernels exist for: 1 .. 4 vectors of four, 1 .. 16 scalars per lane
#define LN_DISPATCH(KERNEL, vec, npl, grid, stream, ...)                                                                               \
  do {                                                                                                                               \
    if ((vec) == 4) {                                                                                                                \
      switch (npl) {                                                                                                                 \
        case 1: hipLaunchKernelGGL((KERNEL<4, 1>), grid, dim3(LN_THREADS), 0, stream, __VA_ARGS__); break;                           \
        case 2: hipLaunchKernelGGL((KERNEL<4, 2>), grid, dim3(LN_THREADS), 0, stream, __VA_ARGS__); break;                           \
        default: hipLaunchKernelGGL((KERNEL<4, 4>), grid, dim3(LN_THREADS), 0, stream, __VA_ARGS__); break;                          \
      }                                                                                                                              \
    } else {                                                                                                                         \
      switch (npl) {                                                                                                                 \
        case 1: hipLaunchKernelGGL((KERNEL<1, 1>), grid, dim3(LN_THREADS), 0, stream, __VA_ARGS__); break;                           \
        case 2: hipLaunchKernelGGL((KERNEL<1, 2>), grid, dim3(LN_THREADS), 0, stream, __VA_ARGS__); break;                           \
        case 4: hipLaunchKernelGGL((KERNEL<1, 4>), grid, dim3(LN_THREADS), 0, stream, __VA_ARGS__); break;                           \
        case 8: hipLaunchKernelGGL((KERNEL<1, 8>), grid, dim3(LN_THREADS), 0, stream, __VA_ARGS__); break;                           \
        default: hipLaunchKernelGGL((KERNEL<1, 16>), grid, dim3(LN_THREADS), 0, stream, __VA_ARGS__); break;                         \
      }                                                                                                                              \
    }                                                                                                                                \
  } while (0)

extern "C" {

size_t dsph_ln_workspace_bytes(int64_t rows, int32_t d) {
  using namespace dsph;
  if (rows < 1 || d < 1 || d > LN_MAX_D || rows > LN_MAX_ROWS) return 0;
  return ln_workspace_bytes(rows, d);
}

// every argument is checked here, before any HIP call
int dsph_ln_forward(const float* x, const float* res, float* sum, float* z, int64_t rows, int32_t d, float eps, const float* gamma,
                    const float* beta, int device, void* hip_stream) {
  using namespace dsph;
  int rc = DSPH_OK;
  if (!x || !z) { set_error("ln_forward: NULL pointer (x and z are required)"); return DSPH_E_BADARG; }
  if ((res == nullptr) != (sum == nullptr)) {
    set_error("ln_forward: res and sum are given together or not at all (res %s, sum %s)", res ? "given" : "NULL", sum ? "given" : "NULL");
    return DSPH_E_BADARG;
  }
  if (!ln_shape_ok("ln_forward", rows, d, &rc)) return rc;
  if (!(eps > 0.f)) { set_error("ln_forward: eps = %g, must be positive", (double)eps); return DSPH_E_BADARG; }
  // a written map overlaps no other map; the one exception is sum == x or sum == res (in place: a lane reads before it writes)
  const int64_t nr = rows < 1 ? 1 : rows;
  if (overlap(z, x, nr, d) || overlap(z, res, nr, d) || overlap(z, sum, nr, d)) {
    set_error("ln_forward: z overlaps x, res or sum");
    return DSPH_E_BADARG;
  }
  if ((sum != x && overlap(sum, x, nr, d)) || (sum != res && overlap(sum, res, nr, d))) {
    set_error("ln_forward: sum overlaps x or res without being one of them (in place means the same pointer)");
    return DSPH_E_BADARG;
  }
  if (rows == 0) return DSPH_OK;
  const int vec = vec_width(d, ptr_bits({x, z, res, sum}), false);
  const LnGeo g = ln_geo(rows, d, vec);
  const int npl = ln_npl(g);
  const dim3 grid((unsigned)ln_fwd_grid(rows, d));
  DeviceGuard guard(device);
  if (!select_device("ln_forward", device, guard)) return DSPH_E_BADARG;
  hipStream_t stream = (hipStream_t)hip_stream;
  LN_DISPATCH(ln_fwd_kernel, vec, npl, grid, stream, x, res, sum, z, gamma, beta, (double)eps, g);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_ln_backward(const float* a, const float* dz, const float* dsum, const float* gamma, float eps, float* da, float* dgamma,
                     float* dbeta, int64_t rows, int32_t d, void* workspace, size_t workspace_bytes, int device, void* hip_stream) {
  using namespace dsph;
  int rc = DSPH_OK;
  if (!a || !dz || !da) { set_error("ln_backward: NULL pointer (a, dz and da are required)"); return DSPH_E_BADARG; }
  if (!ln_shape_ok("ln_backward", rows, d, &rc)) return rc;
  if (!(eps > 0.f)) { set_error("ln_backward: eps = %g, must be positive", (double)eps); return DSPH_E_BADARG; }
  const int64_t nr = rows < 1 ? 1 : rows;
  if (overlap(da, a, nr, d) || overlap(da, dz, nr, d) || overlap(da, dsum, nr, d)) {
    set_error("ln_backward: da overlaps a, dz or dsum");
    return DSPH_E_BADARG;
  }
  const bool want_part = dgamma || dbeta;
  if (want_part && rows > 0) {
    if (!workspace) { set_error("ln_backward: workspace is NULL (dgamma and dbeta are reduced through it)"); return DSPH_E_BADARG; }
    if (!workspace_ok("ln_backward", workspace, workspace_bytes, ln_workspace_bytes(rows, d), &rc)) return rc;
  }
  if (rows == 0) return DSPH_OK;
  const int vec = vec_width(d, ptr_bits({a, dz, da, dsum}), false);
  const LnGeo g = ln_geo(rows, d, vec);
  const int npl = ln_npl(g);
  const int64_t P = ln_partials(rows, d);
  const dim3 grid((unsigned)P);
  double* part = static_cast<double*>(workspace);
  DeviceGuard guard(device);
  if (!select_device("ln_backward", device, guard)) return DSPH_E_BADARG;
  hipStream_t stream = (hipStream_t)hip_stream;
  LN_DISPATCH(ln_bwd_kernel, vec, npl, grid, stream, a, dz, dsum, gamma, (double)eps, da, part, want_part ? 1 : 0, g);
  DSPH_HIP(hipGetLastError());
  if (want_part) {
    // second launch: the P partials [p][dbeta | dgamma][d] of a channel in a fixed order
    hipLaunchKernelGGL(partials_merge_kernel<2>, merge_grid(d, 2), dim3(MERGE_THREADS), 0, stream, (const double*)part, P, (int64_t)2 * d, (int64_t)d, d,
                       dbeta, dgamma);
    DSPH_HIP(hipGetLastError());
  }
  return DSPH_OK;
}

}  // extern "C"
