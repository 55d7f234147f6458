// Batch normalisation with batch statistics over channels-last maps (rows = N * M, F) fp32, the epilogue fused:
//     z = act((y - mean) * rstd * gamma + shift),   mean, var per channel over all rows (plan-free; include/dsphere.h).
// Replaces, in a training step, the host framework's BatchNormalization between the contraction and the bias (reference
// gnn_layers.py:152-159 and GCNN_ResidualLayer.call, :395-405), which wants channels first: a transposed copy of the map,
// the statistics, the normalisation, the bias and the activation as separate passes, and their mirror image backwards.
//
// Passes over the map: forward 3 (statistics: read y; apply: read y, write z), backward 7 (reduction: read dz, z, y;
// input gradient: read dz, z, y, write dy).  Launches: statistics 2, apply 1, backward 3 (the reduction's two and the pass).  Everything is bound by memory, so the work is laid out for the loads:
//
//   * Columns.  A lane owns VEC neighbouring channels (VEC = 4: one 16-byte load per row, where F % 4 == 0 and the maps are
//     16-byte aligned; 2 where F % 2 == 0 and they are 8-byte aligned; else 1) -- nv = F / VEC column vectors.  A workgroup of
//     256 lanes covers CW = min(nv, 256) column vectors by RPI = 256 / CW rows per step, lane t at (row t / CW, column t % CW):
//     neighbouring lanes read neighbouring addresses, rows follow each other without a gap when CW == nv, and a lane keeps its
//     channels' parameters in registers for the whole call.  nv > 256 (F > 1024, or > 256 unvectorised) adds column chunks in
//     grid.x.  Any F >= 1 runs; there is no cap.
//   * Rows.  Workgroup p of P owns the contiguous rows [rows p / P, rows (p + 1) / P) and walks them four steps (4 RPI rows) at
//     a time, the four loads of a lane independent of each other.  Row numbers and element offsets are 64-bit.
//   * Reductions (statistics; s1 = sum g, s2 = sum g x^ of the backward) run in two launches.  The first leaves one partial per
//     (workgroup, channel) in the caller's workspace: lane -> wave by shuffles where the lanes of a wave that share a column are
//     a power of two apart (CW divides 64), -> workgroup through LDS in a fixed order.  The second (one workgroup per channel)
//     merges the P partials in a fixed order in float64.  P = bn_partials(rows, F) depends on the shape alone -- not on the
//     device, the pointers or VEC -- and every lane's share of the rows is fixed by (rows, F, VEC): no atomics, one writer per
//     word, two runs on the same input give the same bits.
//   * Arithmetic: never E[y^2] - E[y]^2.  A lane turns every four rows into (count, mean, M2) by the two-pass formula in
//     registers and merges that into its running triple by Chan's formula; triples merge the same way up to the channel's.  All
//     of it in float64 (the kernels are bound by memory: the float64 work hides behind the loads), and so are x^, s1, s2 and dy
//     of the backward, which take mean and rstd as fp32 arrays PLUS what those rounded away (mean_lo, rstd_lo from
//     dsph_bn_stats).  The reason is the smallest batch: with two rows x^ = +-(1 - e), e = eps / 2 (var + eps), and dy cancels
//     down to (g1 - g2) / 2 * (1 - x^2), 4e-5 of the gradient at eps = 1e-5 -- one fp32 rounding of mean or rstd is 5 % of that.
//
// Nothing here allocates, synchronises or reads the host: every launch goes on the caller's stream and is legal under capture.
#include "dsphere_mapops.h"

namespace dsph {

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_UNROLL = 4;          // row steps per chunk: independent loads in flight per lane
constexpr int64_t BN_MAX_PARTIALS = 2048;
constexpr int64_t BN_PARTIAL_ELEMS = 8192;  // elements of the map per partial, at least (until BN_MAX_PARTIALS is reached)
constexpr int64_t BN_MAX_ROWS = (int64_t)1 << 40, BN_MAX_ELEMS = (int64_t)1 << 62;
static_assert(BN_UNROLL == 4, "the chunk mean of bn_stats_partial_kernel is written out for four rows");

// Partials per channel of the two reductions: the documented function of (rows, F) alone
inline int64_t bn_partials(int64_t rows, int32_t F) {
  int64_t p = (rows * F + BN_PARTIAL_ELEMS - 1) / BN_PARTIAL_ELEMS;
  if (p > BN_MAX_PARTIALS) p = BN_MAX_PARTIALS;
  if (p > rows) p = rows;
  return p < 1 ? 1 : p;
}
inline size_t bn_workspace_bytes(int64_t rows, int32_t F) { return (size_t)(2 * (bn_partials(rows, F) + 1)) * (size_t)F * sizeof(double); }

// how a launch walks the map
struct BnGeo {
  int64_t rows;
  int64_t nblk;  // workgroups along the rows (grid.y): the reductions' P, or the elementwise kernels' own count
  int32_t F, nv, cw, rpi;
};

// this lane's place: row slot r, first channel c0 (of VEC), whether it holds a column at all
struct BnLane {
  int r, cl;
  int64_t c0;
  bool active;
  int64_t row_begin, row_end;
};
template <int VEC>
__device__ __forceinline__ BnLane bn_lane(const BnGeo& g) {
  BnLane l;
  l.r = (int)threadIdx.x / g.cw;
  l.cl = (int)threadIdx.x - l.r * g.cw;
  const int64_t cv = (int64_t)blockIdx.x * g.cw + l.cl;
  l.active = l.r < g.rpi && cv < g.nv;
  l.c0 = cv * VEC;
  l.row_begin = g.rows * (int64_t)blockIdx.y / g.nblk;  // rows <= 2^40, grid.y < 2^16: fits
  l.row_end = g.rows * ((int64_t)blockIdx.y + 1) / g.nblk;
  return l;
}

// -- what the two reductions accumulate -------------------------------------------------------------------------------------
// (count, mean[VEC], M2[VEC]) merged by Chan's formula
template <int VEC>
struct Moments {
  static constexpr int NF = 1 + 2 * VEC;
  double f[NF];  // f[0] count, f[1 + u] mean, f[1 + VEC + u] M2
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < NF; ++i) f[i] = 0.0;
  }
  __device__ __forceinline__ void merge(const Moments& b) {
    const double n = f[0] + b.f[0];
    if (b.f[0] > 0.0) {
      const double w = b.f[0] / n, nab = f[0] * w;
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const double d = b.f[1 + u] - f[1 + u];
        f[1 + u] = fma(d, w, f[1 + u]);
        f[1 + VEC + u] += b.f[1 + VEC + u] + d * d * nab;
      }
    }
    f[0] = n;
  }
};
// (s1[VEC], s2[VEC]): plain sums
template <int VEC>
struct Sums {
  static constexpr int NF = 2 * VEC;
  double f[NF];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < NF; ++i) f[i] = 0.0;
  }
  __device__ __forceinline__ void merge(const Sums& b) {
#pragma unroll
    for (int i = 0; i < NF; ++i) f[i] += b.f[i];
  }
};

// The lanes of one workgroup that share a column -> the lane with r == 0 (threadIdx.x < cw), in a fixed order.
// `lds`: ACC::NF * BN_THREADS doubles.  Every lane of the workgroup calls this (inactive ones with a cleared accumulator).
template <class ACC>
__device__ __forceinline__ void bn_block_combine(ACC& acc, const BnGeo& g, double* lds) {
  const int tid = (int)threadIdx.x;
  if (64 % g.cw == 0) {
    // cw divides the wave: lane l holds column l % cw, the lanes l + cw, l + 2 cw, .. hold the same one
    for (int off = 32; off >= g.cw; off >>= 1) {
      ACC o;
#pragma unroll
      for (int i = 0; i < ACC::NF; ++i) o.f[i] = __shfl_down(acc.f[i], off, 64);
      acc.merge(o);  // (meaningful in the lanes below `off`; the others' results are not read)
    }
    const int lane = tid & 63, wave = tid >> 6;
    if (lane < g.cw) {
#pragma unroll
      for (int i = 0; i < ACC::NF; ++i) lds[i * BN_THREADS + wave * 64 + lane] = acc.f[i];
    }
    __syncthreads();
    if (tid < g.cw) {
      for (int w = 1; w < BN_THREADS / 64; ++w) {
        ACC o;
#pragma unroll
        for (int i = 0; i < ACC::NF; ++i) o.f[i] = lds[i * BN_THREADS + w * 64 + tid];
        acc.merge(o);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < ACC::NF; ++i) lds[i * BN_THREADS + tid] = acc.f[i];
    __syncthreads();
    if (tid < g.cw) {
      for (int r = 1; r < g.rpi; ++r) {
        ACC o;
#pragma unroll
        for (int i = 0; i < ACC::NF; ++i) o.f[i] = lds[i * BN_THREADS + r * g.cw + tid];
        acc.merge(o);
      }
    }
  }
}

// -- statistics, first launch: part[p][0][c] = mean, part[p][1][c] = M2 of channel c over the rows of workgroup p -------------
template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_partial_kernel(const float* __restrict__ y, double* __restrict__ part, BnGeo g) {
  __shared__ double lds[Moments<VEC>::NF * BN_THREADS];
  const BnLane l = bn_lane<VEC>(g);
  Moments<VEC> acc;
  acc.clear();
  if (l.active) {
    const int64_t step = (int64_t)g.rpi;
    for (int64_t row0 = l.row_begin + l.r; row0 < l.row_end; row0 += BN_UNROLL * step) {
      float v[BN_UNROLL][VEC];
      int cnt = 0;
      if (row0 + (BN_UNROLL - 1) * step < l.row_end) {
#pragma unroll
        for (int u = 0; u < BN_UNROLL; ++u) ldv<VEC>(y + (row0 + u * step) * g.F + l.c0, v[u]);
        cnt = BN_UNROLL;
      } else {
#pragma unroll
        for (int u = 0; u < BN_UNROLL; ++u) {
          if (row0 + u * step < l.row_end) {
            ldv<VEC>(y + (row0 + u * step) * g.F + l.c0, v[u]);
            cnt = u + 1;
          } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[u][e] = 0.f;
          }
        }
      }
      // the chunk's (cnt, mean, M2) by the two-pass formula, then Chan's merge into the lane's running triple
      Moments<VEC> ch;
      ch.f[0] = (double)cnt;
      const double inv = 1.0 / (double)cnt;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double m = (((double)v[0][e] + (double)v[1][e]) + ((double)v[2][e] + (double)v[3][e])) * inv;
        double m2 = 0.0;
#pragma unroll
        for (int u = 0; u < BN_UNROLL; ++u) {
          const double d = (double)v[u][e] - m;
          m2 = u < cnt ? fma(d, d, m2) : m2;
        }
        ch.f[1 + e] = m;
        ch.f[1 + VEC + e] = m2;
      }
      acc.merge(ch);
    }
  }
  bn_block_combine(acc, g, lds);
  if ((int)threadIdx.x < g.cw && l.active) {
    double* out = part + (int64_t)blockIdx.y * 2 * g.F + l.c0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      out[e] = acc.f[1 + e];
      out[g.F + e] = acc.f[1 + VEC + e];
    }
  }
}

// -- statistics, second launch: one workgroup per channel merges the P partials in a fixed order, in float64 ------------------
__global__ __launch_bounds__(BN_THREADS) void bn_stats_final_kernel(const double* __restrict__ part, int64_t rows, int64_t P, int32_t F, float eps,
                                                                     float* __restrict__ mean, float* __restrict__ var, float* __restrict__ rstd,
                                                                     float* __restrict__ mean_lo, float* __restrict__ rstd_lo,
                                                                     float* running_mean, float* running_var, float momentum) {
  __shared__ double sn[BN_THREADS], sm[BN_THREADS], s2[BN_THREADS];
  const int c = (int)blockIdx.x, t = (int)threadIdx.x;
  double n = 0.0, m = 0.0, M2 = 0.0;
  for (int64_t p = t; p < P; p += BN_THREADS) {
    const double nb = (double)(rows * (p + 1) / P - rows * p / P);  // the rows of workgroup p (bn_lane)
    if (nb > 0.0) {
      const double mb = part[p * 2 * F + c], M2b = part[p * 2 * F + F + c];
      const double nn = n + nb, d = mb - m;
      m += d * (nb / nn);
      M2 += M2b + d * d * (n * nb / nn);
      n = nn;
    }
  }
  sn[t] = n; sm[t] = m; s2[t] = M2;
  __syncthreads();
  for (int s = BN_THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) {
      const double na = sn[t], nb = sn[t + s];
      if (nb > 0.0) {
        const double nn = na + nb, d = sm[t + s] - sm[t];
        sm[t] += d * (nb / nn);
        s2[t] += s2[t + s] + d * d * (na * nb / nn);
        sn[t] = nn;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    const double mu = sm[0], v = s2[0] / (double)rows;  // biased
    const double rs = 1.0 / sqrt(v + (double)eps);
    mean[c] = (float)mu;
    var[c] = (float)v;
    rstd[c] = (float)rs;
    // what the fp32 arrays round away, for the backward (mean = mean[c] + mean_lo[c] to 2^-48)
    if (mean_lo) mean_lo[c] = (float)(mu - (double)(float)mu);
    if (rstd_lo) rstd_lo[c] = (float)(rs - (double)(float)rs);
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mu;
    if (running_var) {  // the unbiased variance, as torch.nn.BatchNorm1d keeps it (rows >= 2: checked by the entry point)
      const float unb = (float)(s2[0] / (double)(rows - 1));
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * unb;
    }
  }
}

// per-channel parameters of a lane, NULL = the neutral value
template <int VEC>
__device__ __forceinline__ void bn_param(const float* p, int64_t c0, float neutral, float (&r)[VEC]) {
#pragma unroll
  for (int e = 0; e < VEC; ++e) r[e] = p ? p[c0 + e] : neutral;
}

// the same in float64 from an fp32 array and, where the caller has it, what that array rounded away
template <int VEC>
__device__ __forceinline__ void bn_param2(const float* hi, const float* lo, int64_t c0, double (&r)[VEC]) {
#pragma unroll
  for (int e = 0; e < VEC; ++e) r[e] = (double)hi[c0 + e] + (lo ? (double)lo[c0 + e] : 0.0);
}

// -- apply: z = act((y - mean) * rstd * gamma + shift); z may be y (a lane reads its elements before it writes them) -----------
template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const float* y, float* z, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                               const float* __restrict__ shift, int act, BnGeo g) {
  const BnLane l = bn_lane<VEC>(g);
  if (!l.active) return;
  float mu[VEC], rs[VEC], ga[VEC], sh[VEC];
  bn_param<VEC>(mean, l.c0, 0.f, mu);
  bn_param<VEC>(rstd, l.c0, 1.f, rs);
  bn_param<VEC>(gamma, l.c0, 1.f, ga);
  bn_param<VEC>(shift, l.c0, 0.f, sh);
  const int64_t step = (int64_t)g.rpi;
  for (int64_t row0 = l.row_begin + l.r; row0 < l.row_end; row0 += BN_UNROLL * step) {
    float v[BN_UNROLL][VEC];
    const bool full = row0 + (BN_UNROLL - 1) * step < l.row_end;
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u)
      if (full || row0 + u * step < l.row_end) ldv<VEC>(y + (row0 + u * step) * g.F + l.c0, v[u]);
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      if (full || row0 + u * step < l.row_end) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[u][e] = apply_act(fmaf((v[u][e] - mu[e]) * rs[e], ga[e], sh[e]), act);
        stv<VEC>(z + (row0 + u * step) * g.F + l.c0, v[u]);
      }
    }
  }
}

// -- backward, first launch: part[p][0][c] = sum g, part[p][1][c] = sum g x^ over the rows of workgroup p ----------------------
template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_partial_kernel(const float* __restrict__ y, const float* __restrict__ z,
                                                                     const float* __restrict__ dz, const float* __restrict__ mean,
                                                                     const float* __restrict__ rstd, const float* __restrict__ mean_lo,
                                                                     const float* __restrict__ rstd_lo, double* __restrict__ part, int act,
                                                                     BnGeo g) {
  __shared__ double lds[Sums<VEC>::NF * BN_THREADS];
  const BnLane l = bn_lane<VEC>(g);
  Sums<VEC> acc;
  acc.clear();
  if (l.active) {
    double mu[VEC], rs[VEC];
    bn_param2<VEC>(mean, mean_lo, l.c0, mu);
    bn_param2<VEC>(rstd, rstd_lo, l.c0, rs);
    const int64_t step = (int64_t)g.rpi;
    for (int64_t row0 = l.row_begin + l.r; row0 < l.row_end; row0 += BN_UNROLL * step) {
      double s1[VEC], s2[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) s1[e] = s2[e] = 0.0;
      const bool full = row0 + (BN_UNROLL - 1) * step < l.row_end;
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        if (full || row0 + u * step < l.row_end) {
          const int64_t o = (row0 + u * step) * g.F + l.c0;
          float gv[VEC], yv[VEC];
          ldv<VEC>(dz + o, gv);
          ldv<VEC>(y + o, yv);
          if (act != DSPH_ACT_NONE) {
            float zv[VEC];
            ldv<VEC>(z + o, zv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) gv[e] *= act_grad(zv[e], act);
          }
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            s1[e] += (double)gv[e];
            s2[e] = fma((double)gv[e], ((double)yv[e] - mu[e]) * rs[e], s2[e]);
          }
        }
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        acc.f[e] += s1[e];
        acc.f[VEC + e] += s2[e];
      }
    }
  }
  bn_block_combine(acc, g, lds);
  if ((int)threadIdx.x < g.cw && l.active) {
    double* out = part + (int64_t)blockIdx.y * 2 * g.F + l.c0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      out[e] = acc.f[e];
      out[g.F + e] = acc.f[VEC + e];
    }
  }
}

// -- backward, second launch: the P partial sums of a channel in a fixed order, in float64 -> sums[0][c] = s1, sums[1][c] = s2 ---
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_final_kernel(const double* __restrict__ part, int64_t P, int32_t F, double* __restrict__ sums,
                                                                   float* __restrict__ dgamma, float* __restrict__ dshift) {
  __shared__ double a1[BN_THREADS], a2[BN_THREADS];
  const int c = (int)blockIdx.x, t = (int)threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t p = t; p < P; p += BN_THREADS) {
    s1 += part[p * 2 * F + c];
    s2 += part[p * 2 * F + F + c];
  }
  a1[t] = s1; a2[t] = s2;
  __syncthreads();
  for (int s = BN_THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) {
      a1[t] += a1[t + s];
      a2[t] += a2[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    sums[c] = a1[0];
    sums[F + c] = a2[0];
    if (dshift) dshift[c] = (float)a1[0];
    if (dgamma) dgamma[c] = (float)a2[0];
  }
}

// -- backward, third launch (elementwise): dy = gamma * rstd * (g - s1 / R - x^ * s2 / R) --------------------------------------
template <int VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(const float* y, const float* z, const float* dz, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd, const float* __restrict__ mean_lo,
                                                                   const float* __restrict__ rstd_lo, const float* __restrict__ gamma,
                                                                   const double* __restrict__ sums, float* dy, double inv_rows, int act, BnGeo g) {
  const BnLane l = bn_lane<VEC>(g);
  if (!l.active) return;
  double mu[VEC], rs[VEC], k[VEC], m1[VEC], m2[VEC];
  float ga[VEC];
  bn_param2<VEC>(mean, mean_lo, l.c0, mu);
  bn_param2<VEC>(rstd, rstd_lo, l.c0, rs);
  bn_param<VEC>(gamma, l.c0, 1.f, ga);
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    k[e] = (double)ga[e] * rs[e];
    m1[e] = sums[l.c0 + e] * inv_rows;
    m2[e] = sums[g.F + l.c0 + e] * inv_rows;
  }
  const int64_t step = (int64_t)g.rpi;
  for (int64_t row0 = l.row_begin + l.r; row0 < l.row_end; row0 += BN_UNROLL * step) {
    const bool full = row0 + (BN_UNROLL - 1) * step < l.row_end;
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      if (full || row0 + u * step < l.row_end) {
        const int64_t o = (row0 + u * step) * g.F + l.c0;
        float gv[VEC], yv[VEC];
        ldv<VEC>(dz + o, gv);
        ldv<VEC>(y + o, yv);
        if (act != DSPH_ACT_NONE) {
          float zv[VEC];
          ldv<VEC>(z + o, zv);
#pragma unroll
          for (int e = 0; e < VEC; ++e) gv[e] *= act_grad(zv[e], act);
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) gv[e] = (float)(k[e] * ((double)gv[e] - m1[e] - ((double)yv[e] - mu[e]) * rs[e] * m2[e]));
        stv<VEC>(dy + o, gv);
      }
    }
  }
}

// `nblk` <= 0: the elementwise kernels' own split of the rows (one workgroup per 4 chunks, at most 16,384 workgroups)
BnGeo bn_geo(int64_t rows, int32_t F, int vec, int64_t nblk) {
  BnGeo g;
  g.rows = rows;
  g.F = F;
  g.nv = F / vec;
  g.cw = g.nv < BN_THREADS ? g.nv : BN_THREADS;
  g.rpi = BN_THREADS / g.cw;
  if (nblk <= 0) {
    const int64_t per = (int64_t)g.rpi * BN_UNROLL * 4;
    nblk = (rows + per - 1) / per;
    if (nblk > 16384) nblk = 16384;
    if (nblk < 1) nblk = 1;
  }
  g.nblk = nblk;
  return g;
}
dim3 bn_grid(const BnGeo& g) { return dim3((unsigned)((g.nv + g.cw - 1) / g.cw), (unsigned)g.nblk); }  // (column chunks, row blocks <= 16,384)

bool bn_shape_ok(const char* who, int64_t rows, int32_t F, int* rc) {
  if (rows < 1 || F < 1) {
    set_error("%s: rows = %lld, F = %d, both must be at least 1", who, (long long)rows, (int)F);
    *rc = DSPH_E_BADARG;
    return false;
  }
  if (rows > BN_MAX_ROWS || rows > BN_MAX_ELEMS / F) {
    set_error("%s: rows = %lld, F = %d: more than 2^40 rows or 2^62 elements", who, (long long)rows, (int)F);
    *rc = DSPH_E_UNSUPPORTED;
    return false;
  }
  return true;
}

}  // namespace

}  // namespace dsph

extern "C" {

size_t dsph_bn_workspace_bytes(int64_t rows, int32_t F) {
  using namespace dsph;
  if (rows < 1 || F < 1 || rows > BN_MAX_ROWS || rows > BN_MAX_ELEMS / F) return 0;
  return bn_workspace_bytes(rows, F);
}

// every argument is checked here, before any HIP call
int dsph_bn_stats(const float* y, int64_t rows, int32_t F, float eps, float* mean, float* var, float* rstd, float* mean_lo, float* rstd_lo,
                  float* running_mean, float* running_var, float momentum, void* workspace, size_t workspace_bytes, int device, void* hip_stream) {
  using namespace dsph;
  int rc = DSPH_OK;
  if (!y || !mean || !var || !rstd || !workspace) {
    set_error("bn_stats: NULL pointer (y, mean, var, rstd and workspace are required)");
    return DSPH_E_BADARG;
  }
  if (!bn_shape_ok("bn_stats", rows, F, &rc)) return rc;
  if (!(eps > 0.f)) { set_error("bn_stats: eps = %g, must be positive", (double)eps); return DSPH_E_BADARG; }
  if ((running_mean || running_var) && !(momentum >= 0.f && momentum <= 1.f)) {
    set_error("bn_stats: momentum = %g, must lie in [0, 1]", (double)momentum);
    return DSPH_E_BADARG;
  }
  if (running_var && rows < 2) {
    set_error("bn_stats: rows = 1 has no unbiased variance to update running_var with");
    return DSPH_E_BADARG;
  }
  if (!workspace_ok("bn_stats", workspace, workspace_bytes, bn_workspace_bytes(rows, F), &rc)) return rc;
  const int64_t P = bn_partials(rows, F);
  const int vec = vec_width(F, ptr_bits({y}), true);
  const BnGeo g = bn_geo(rows, F, vec, P);
  double* part = static_cast<double*>(workspace);
  DeviceGuard guard(device);
  if (!select_device("bn_stats", device, guard)) return DSPH_E_BADARG;
  hipStream_t stream = (hipStream_t)hip_stream;
  DSPH_LAUNCH_BY_VEC(vec, bn_stats_partial_kernel, bn_grid(g), dim3(BN_THREADS), stream, y, part, g);
  DSPH_HIP(hipGetLastError());
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((unsigned)F), dim3(BN_THREADS), 0, stream, (const double*)part, rows, P, F, eps, mean, var,
                     rstd, mean_lo, rstd_lo, running_mean, running_var, momentum);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_bn_apply(const float* y, float* z, int64_t rows, int32_t F, const float* mean, const float* rstd, const float* gamma,
                  const float* shift, int32_t act, int device, void* hip_stream) {
  using namespace dsph;
  int rc = DSPH_OK;
  if (!y || !z || !mean || !rstd) { set_error("bn_apply: NULL pointer (y, z, mean and rstd are required)"); return DSPH_E_BADARG; }
  if (!bn_shape_ok("bn_apply", rows, F, &rc)) return rc;
  if (act < DSPH_ACT_NONE || act > DSPH_ACT_TANH) { set_error("bn_apply: unknown activation %d", (int)act); return DSPH_E_BADARG; }
  const int vec = vec_width(F, ptr_bits({y, z}), true);
  const BnGeo g = bn_geo(rows, F, vec, 0);
  DeviceGuard guard(device);
  if (!select_device("bn_apply", device, guard)) return DSPH_E_BADARG;
  hipStream_t stream = (hipStream_t)hip_stream;
  DSPH_LAUNCH_BY_VEC(vec, bn_apply_kernel, bn_grid(g), dim3(BN_THREADS), stream, y, z, mean, rstd, gamma, shift, (int)act, g);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_bn_backward(const float* y, const float* z, const float* dz, const float* mean, const float* rstd, const float* mean_lo,
                     const float* rstd_lo, const float* gamma, float* dy,
                     float* dgamma, float* dshift, int64_t rows, int32_t F, int32_t act, void* workspace, size_t workspace_bytes, int device,
                     void* hip_stream) {
  using namespace dsph;
  int rc = DSPH_OK;
  if (!y || !dz || !mean || !rstd || !dy || !workspace) {
    set_error("bn_backward: NULL pointer (y, dz, mean, rstd, dy and workspace are required)");
    return DSPH_E_BADARG;
  }
  if (!bn_shape_ok("bn_backward", rows, F, &rc)) return rc;
  if (act < DSPH_ACT_NONE || act > DSPH_ACT_TANH) { set_error("bn_backward: unknown activation %d", (int)act); return DSPH_E_BADARG; }
  if (act != DSPH_ACT_NONE && !z) {
    set_error("bn_backward: z is NULL; the derivative of activation %d is taken from the forward's output", (int)act);
    return DSPH_E_BADARG;
  }
  if (!workspace_ok("bn_backward", workspace, workspace_bytes, bn_workspace_bytes(rows, F), &rc)) return rc;
  const int64_t P = bn_partials(rows, F);
  const int vec = vec_width(F, ptr_bits({y, dz, dy, act != DSPH_ACT_NONE ? z : nullptr}), true);  // (z is read only behind an activation)
  const BnGeo gr = bn_geo(rows, F, vec, P), ge = bn_geo(rows, F, vec, 0);
  double* part = static_cast<double*>(workspace);
  double* sums = part + 2 * P * F;  // s1[F], s2[F]
  const double inv_rows = 1.0 / (double)rows;
  DeviceGuard guard(device);
  if (!select_device("bn_backward", device, guard)) return DSPH_E_BADARG;
  hipStream_t stream = (hipStream_t)hip_stream;
  DSPH_LAUNCH_BY_VEC(vec, bn_bwd_partial_kernel, bn_grid(gr), dim3(BN_THREADS), stream, y, z, dz, mean, rstd, mean_lo, rstd_lo, part,
                     (int)act, gr);
  DSPH_HIP(hipGetLastError());
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((unsigned)F), dim3(BN_THREADS), 0, stream, (const double*)part, P, F, sums, dgamma, dshift);
  DSPH_HIP(hipGetLastError());
  DSPH_LAUNCH_BY_VEC(vec, bn_bwd_apply_kernel, bn_grid(ge), dim3(BN_THREADS), stream, y, z, dz, mean, rstd, mean_lo, rstd_lo, gamma,
                     (const double*)sums, dy, inv_rows, (int)act, ge);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
