// Attention restricted to the edges of the pixel graph: pixel i attends to the rows its neighbour table names (7 - 22 of them on
// a HEALPix graph).  Replaces gnn_transformers.scaled_dot_product_sparse_attention of the reference (gnn_transformers.py:54-106),
// which looks q, k and v up PER EDGE (three tensors of N * E * d floats, E = 8 - 20 M) and follows them with two segment sums;
// here q, k, v are read once per (row, neighbour) from L2 / HBM as whole channel rows and the softmax stays in registers.
//
//   s_ij = q_i,h . k_j,h / sqrt(D)     p_ij = softmax_j(s_ij)     out_i,h = sum_j p_ij v_j,h     lse_i,h = log sum_j exp(s_ij)
//
// Layout: q, k, v channels-last (N, M, d) with a row stride ld >= d (three views of one (N, M, 3 d) projection), heads are
// contiguous groups of D channels (the reference's split_heads without its transposes); out (N, M, d) and lse (N, M, heads)
// contiguous.  nbr is int32 [M][W], a row's neighbours first, -1 in the unused slots; slots are summed in slot order.  An entry
// outside [0, M) is treated as unused, so no table can make the kernels read out of bounds.
//
// A lane owns four channels (16-byte loads); a row takes d / 4 lanes and a wave floor(64 / (d / 4)) rows; the dot products are
// reduced over the D / 4 lanes of a head with xor shuffles (the groups are aligned: a row starts at a multiple of D / 4 lanes).
// Online softmax (running maximum m, sum l, float4 accumulator): the stable form, unlike the reference, which exponentiates the
// raw logits and overflows above 88 -- mathematically the same number.  The k / v rows of NBR_UNROLL slots are requested before
// the first is consumed.  Workgroups take contiguous row ranges of one XCD (xcd_remap), so most neighbour rows come from the L2
// the neighbouring workgroups filled.  A row without neighbours yields out = 0, lse = 0 (the reference: 0 / 0).
//
// Backward, no atomics, bitwise reproducible.  With delta_i,h = dout_i,h . out_i,h and p_ij = exp(s_ij - lse_i):
//   pass 1, over nbr  (out-edges of i):  ds_ij = p_ij (dout_i . v_j - delta_i)    dq_i = scale sum_j ds_ij k_j     (writes delta)
//   pass 2, over nbrT (in-edges of j):   dv_j = sum_i p_ij dout_i                 dk_j = scale sum_i ds_ij q_i
// Two launches on the caller's stream; every output element has one writer and a fixed order of summation.
#include <cmath>

#include "dsphere_mapops.h"

namespace dsph {

#define NBR_UNROLL 4

template <int LPH>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
  for (int m = LPH / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }
__device__ __forceinline__ void axpy4(float4& a, float s, const float4& b) {
  a.x = fmaf(s, b.x, a.x); a.y = fmaf(s, b.y, a.y); a.z = fmaf(s, b.z, a.z); a.w = fmaf(s, b.w, a.w);
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// which (map, row, channel quad) a lane works on
struct NbrLane {
  int64_t n, row;
  int c;       // channel quad inside the row
  bool valid;  // idle lanes (64 % lanes-per-row, rows past M) run the shuffles and touch no memory
};

__device__ __forceinline__ bool nbr_lane(NbrLane& L, unsigned nblk, int64_t waves, int64_t groups, int64_t M, int lpr, int rpw) {
  const int64_t wv = (int64_t)xcd_remap(blockIdx.x, nblk) * 4 + (threadIdx.x >> 6);
  if (wv >= waves) return false;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int r = lane / lpr;
  L.n = wv / groups;
  L.c = lane - r * lpr;
  L.row = (wv - L.n * groups) * rpw + r;
  L.valid = r < rpw && L.row < M;
  return true;
}

// slot s of the lane's table row, -1 when there is none
__device__ __forceinline__ int nbr_slot(const int32_t* __restrict__ nb, int s, int W, bool valid, int64_t M) {
  const int t = (valid && s < W) ? nb[s] : -1;
  return (t >= 0 && (int64_t)t < M) ? t : -1;
}

template <int D>
__global__ __launch_bounds__(256) void nbr_attention_forward_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                     const float* __restrict__ v, int64_t ld, float* __restrict__ out,
                                                                     float* __restrict__ lse, const int32_t* __restrict__ nbr, int W,
                                                                     int64_t M, int heads, int lpr, int rpw, int64_t groups,
                                                                     int64_t waves, unsigned nblk, float scale) {
  constexpr int LPH = D / 4;
  NbrLane L;
  if (!nbr_lane(L, nblk, waves, groups, M, lpr, rpw)) return;
  const int64_t base = L.n * M;
  const int32_t* __restrict__ nb = nbr + (L.valid ? L.row : 0) * W;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 qv = L.valid ? ld4(q + (base + L.row) * ld + 4 * L.c) : z4;
  float m = -__builtin_huge_valf(), l = 0.f;
  float4 acc = z4;
  for (int s0 = 0; s0 < W; s0 += NBR_UNROLL) {
    int j[NBR_UNROLL];
    float4 kk[NBR_UNROLL], vv[NBR_UNROLL];
#pragma unroll
    for (int u = 0; u < NBR_UNROLL; ++u) j[u] = nbr_slot(nb, s0 + u, W, L.valid, M);
    if (__all(j[0] < 0)) break;  // a row's neighbours come first
#pragma unroll
    for (int u = 0; u < NBR_UNROLL; ++u) {
      kk[u] = j[u] >= 0 ? ld4(k + (base + j[u]) * ld + 4 * L.c) : z4;
      vv[u] = j[u] >= 0 ? ld4(v + (base + j[u]) * ld + 4 * L.c) : z4;
    }
#pragma unroll
    for (int u = 0; u < NBR_UNROLL; ++u) {
      const float s = head_sum<LPH>(dot4(qv, kk[u])) * scale;
      if (j[u] >= 0) {
        const float mn = fmaxf(m, s);
        const float corr = expf(m - mn), p = expf(s - mn);  // (first neighbour: m = -inf, corr = 0)
        l = fmaf(l, corr, p);
        acc.x = fmaf(acc.x, corr, p * vv[u].x); acc.y = fmaf(acc.y, corr, p * vv[u].y);
        acc.z = fmaf(acc.z, corr, p * vv[u].z); acc.w = fmaf(acc.w, corr, p * vv[u].w);
        m = mn;
      }
    }
  }
  if (!L.valid) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;
  *reinterpret_cast<float4*>(out + (base + L.row) * (int64_t)(4 * lpr) + 4 * L.c) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
  if (lse != nullptr && L.c % LPH == 0) lse[(base + L.row) * heads + L.c / LPH] = l > 0.f ? m + logf(l) : 0.f;
}

// pass 1 of the backward: delta and dq of the lane's row, over its out-edges
template <int D>
__global__ __launch_bounds__(256) void nbr_attention_dq_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                const float* __restrict__ v, int64_t ld, const float* __restrict__ out,
                                                                const float* __restrict__ lse, const float* __restrict__ dout,
                                                                const int32_t* __restrict__ nbr, int W, float* __restrict__ delta,
                                                                float* __restrict__ dq, int64_t ldg, int64_t M, int heads, int lpr,
                                                                int rpw, int64_t groups, int64_t waves, unsigned nblk, float scale) {
  constexpr int LPH = D / 4;
  NbrLane L;
  if (!nbr_lane(L, nblk, waves, groups, M, lpr, rpw)) return;
  const int64_t base = L.n * M, d = 4 * lpr;
  const int32_t* __restrict__ nb = nbr + (L.valid ? L.row : 0) * W;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int h = L.c / LPH;
  const float4 qv = L.valid ? ld4(q + (base + L.row) * ld + 4 * L.c) : z4;
  const float4 gv = L.valid ? ld4(dout + (base + L.row) * d + 4 * L.c) : z4;
  const float4 ov = L.valid ? ld4(out + (base + L.row) * d + 4 * L.c) : z4;
  const float ls = L.valid ? lse[(base + L.row) * heads + h] : 0.f;
  const float dl = head_sum<LPH>(dot4(gv, ov));
  float4 acc = z4;
  for (int s0 = 0; s0 < W; s0 += NBR_UNROLL) {
    int j[NBR_UNROLL];
    float4 kk[NBR_UNROLL], vv[NBR_UNROLL];
#pragma unroll
    for (int u = 0; u < NBR_UNROLL; ++u) j[u] = nbr_slot(nb, s0 + u, W, L.valid, M);
    if (__all(j[0] < 0)) break;
#pragma unroll
    for (int u = 0; u < NBR_UNROLL; ++u) {
      kk[u] = j[u] >= 0 ? ld4(k + (base + j[u]) * ld + 4 * L.c) : z4;
      vv[u] = j[u] >= 0 ? ld4(v + (base + j[u]) * ld + 4 * L.c) : z4;
    }
#pragma unroll
    for (int u = 0; u < NBR_UNROLL; ++u) {
      const float s = head_sum<LPH>(dot4(qv, kk[u])) * scale;
      const float gvv = head_sum<LPH>(dot4(gv, vv[u]));
      if (j[u] >= 0) axpy4(acc, expf(s - ls) * (gvv - dl), kk[u]);
    }
  }
  if (!L.valid) return;
  if (L.c % LPH == 0) delta[(base + L.row) * heads + h] = dl;
  *reinterpret_cast<float4*>(dq + (base + L.row) * ldg + 4 * L.c) = make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale);
}

// pass 2: dk and dv of the lane's row j, over its in-edges (the rows i whose table names j)
template <int D>
__global__ __launch_bounds__(256) void nbr_attention_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                 const float* __restrict__ v, int64_t ld, const float* __restrict__ lse,
                                                                 const float* __restrict__ dout, const int32_t* __restrict__ nbrT, int W,
                                                                 const float* __restrict__ delta, float* __restrict__ dk,
                                                                 float* __restrict__ dv, int64_t ldg, int64_t M, int heads, int lpr,
                                                                 int rpw, int64_t groups, int64_t waves, unsigned nblk, float scale) {
  constexpr int LPH = D / 4;
  NbrLane L;
  if (!nbr_lane(L, nblk, waves, groups, M, lpr, rpw)) return;
  const int64_t base = L.n * M, d = 4 * lpr;
  const int32_t* __restrict__ nb = nbrT + (L.valid ? L.row : 0) * W;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int h = L.c / LPH;
  const float4 kv = L.valid ? ld4(k + (base + L.row) * ld + 4 * L.c) : z4;
  const float4 vv = L.valid ? ld4(v + (base + L.row) * ld + 4 * L.c) : z4;
  float4 ak = z4, av = z4;
  for (int s0 = 0; s0 < W; s0 += NBR_UNROLL) {
    int i[NBR_UNROLL];
    float4 qq[NBR_UNROLL], gg[NBR_UNROLL];
    float ls[NBR_UNROLL], dl[NBR_UNROLL];
#pragma unroll
    for (int u = 0; u < NBR_UNROLL; ++u) i[u] = nbr_slot(nb, s0 + u, W, L.valid, M);
    if (__all(i[0] < 0)) break;
#pragma unroll
    for (int u = 0; u < NBR_UNROLL; ++u) {
      qq[u] = i[u] >= 0 ? ld4(q + (base + i[u]) * ld + 4 * L.c) : z4;
      gg[u] = i[u] >= 0 ? ld4(dout + (base + i[u]) * d + 4 * L.c) : z4;
      ls[u] = i[u] >= 0 ? lse[(base + i[u]) * heads + h] : 0.f;
      dl[u] = i[u] >= 0 ? delta[(base + i[u]) * heads + h] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NBR_UNROLL; ++u) {
      const float s = head_sum<LPH>(dot4(qq[u], kv)) * scale;
      const float gvv = head_sum<LPH>(dot4(gg[u], vv));
      if (i[u] >= 0) {
        const float p = expf(s - ls[u]);
        axpy4(av, p, gg[u]);
        axpy4(ak, p * (gvv - dl[u]), qq[u]);
      }
    }
  }
  if (!L.valid) return;
  *reinterpret_cast<float4*>(dv + (base + L.row) * ldg + 4 * L.c) = av;
  *reinterpret_cast<float4*>(dk + (base + L.row) * ldg + 4 * L.c) = make_float4(ak.x * scale, ak.y * scale, ak.z * scale, ak.w * scale);
}

// how a launch spreads (map, row) over waves
struct NbrGrid {
  int lpr, rpw;
  int64_t groups, waves;
  unsigned nblk;
  float scale;
};

static int nbr_grid(NbrGrid& g, const char* who, int64_t N, int64_t M, int32_t heads, int32_t depth) {
  g.lpr = heads * depth / 4;
  g.rpw = 64 / g.lpr;
  g.groups = (M + g.rpw - 1) / g.rpw;
  g.waves = N * g.groups;
  const int64_t nblk = (g.waves + 3) / 4;
  if (nblk > 0x7fffffffLL) { set_error("%s: grid too large (%lld workgroups)", who, (long long)nblk); return DSPH_E_UNSUPPORTED; }
  g.nblk = (unsigned)nblk;
  g.scale = (float)(1.0 / std::sqrt((double)depth));
  return DSPH_OK;
}

#define NBR_BY_DEPTH(depth, CALL) \
  switch (depth) {                \
    case 4: CALL(4); break;       \
    case 8: CALL(8); break;       \
    case 16: CALL(16); break;     \
    case 32: CALL(32); break;     \
    default: CALL(64); break;     \
  }

// the shape limits of the kernels above, each named in its message
static int nbr_attention_args_ok(const char* who, int64_t ld, int32_t width, int64_t N, int64_t M, int32_t heads, int32_t depth) {
  if (N < 0 || M < 0) { set_error("%s: negative size (N %lld, M %lld)", who, (long long)N, (long long)M); return DSPH_E_BADARG; }
  if (M > 0x7fffffffLL) { set_error("%s: M = %lld exceeds the int32 row indices of the neighbour table", who, (long long)M); return DSPH_E_BADARG; }
  const int rc = attention_shape_ok(who, heads, depth, " (one wave holds a row)");
  if (rc != DSPH_OK) return rc;
  if (width < 1) { set_error("%s: neighbour table width %d, must be at least 1", who, (int)width); return DSPH_E_BADARG; }
  return attention_stride_ok(who, ld, heads, depth);
}

}  // namespace dsph

extern "C" {

int dsph_nbr_attention_forward(const float* q, const float* k, const float* v, int64_t ld, float* out, float* lse, const int32_t* nbr,
                               int32_t width, int64_t N, int64_t M, int32_t heads, int32_t depth, int device, void* hip_stream) {
  using namespace dsph;
  if (!q || !k || !v || !out || !nbr) { set_error("nbr_attention_forward: NULL pointer"); return DSPH_E_BADARG; }
  int rc = nbr_attention_args_ok("nbr_attention_forward", ld, width, N, M, heads, depth);
  if (rc != DSPH_OK) return rc;
  if (!aligned16({q, k, v, out})) { set_error("nbr_attention_forward: q, k, v and out must be 16-byte aligned"); return DSPH_E_BADARG; }
  DeviceGuard guard(device);
  if (N <= 0 || M <= 0) return DSPH_OK;
  NbrGrid g;
  rc = nbr_grid(g, "nbr_attention_forward", N, M, heads, depth);
  if (rc != DSPH_OK) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
#define NBR_FWD(DD)                                                                                                              \
  hipLaunchKernelGGL(nbr_attention_forward_kernel<DD>, dim3(g.nblk), dim3(256), 0, stream, q, k, v, ld, out, lse, nbr, (int)width, M, \
                     (int)heads, g.lpr, g.rpw, g.groups, g.waves, g.nblk, g.scale)
  NBR_BY_DEPTH(depth, NBR_FWD)
#undef NBR_FWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_nbr_attention_backward(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* lse,
                                const float* dout, const int32_t* nbr, int32_t width, const int32_t* nbrT, int32_t widthT, float* delta,
                                float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N, int64_t M, int32_t heads, int32_t depth,
                                int device, void* hip_stream) {
  using namespace dsph;
  if (!q || !k || !v || !out || !lse || !dout || !nbr || !nbrT || !delta || !dq || !dk || !dv) {
    set_error("nbr_attention_backward: NULL pointer");
    return DSPH_E_BADARG;
  }
  int rc = nbr_attention_args_ok("nbr_attention_backward", ld, width, N, M, heads, depth);
  if (rc == DSPH_OK) rc = nbr_attention_args_ok("nbr_attention_backward (gradients, transposed table)", ld_grad, widthT, N, M, heads, depth);
  if (rc != DSPH_OK) return rc;
  if (!aligned16({q, k, v, out, dout, dq, dk, dv})) {
    set_error("nbr_attention_backward: q, k, v, out, dout, dq, dk and dv must be 16-byte aligned");
    return DSPH_E_BADARG;
  }
  DeviceGuard guard(device);
  if (N <= 0 || M <= 0) return DSPH_OK;
  NbrGrid g;
  rc = nbr_grid(g, "nbr_attention_backward", N, M, heads, depth);
  if (rc != DSPH_OK) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
#define NBR_BWD(DD)                                                                                                                  \
  hipLaunchKernelGGL(nbr_attention_dq_kernel<DD>, dim3(g.nblk), dim3(256), 0, stream, q, k, v, ld, out, lse, dout, nbr, (int)width, delta, \
                     dq, ld_grad, M, (int)heads, g.lpr, g.rpw, g.groups, g.waves, g.nblk, g.scale);                                  \
  hipLaunchKernelGGL(nbr_attention_dkv_kernel<DD>, dim3(g.nblk), dim3(256), 0, stream, q, k, v, ld, lse, dout, nbrT, (int)widthT, delta,   \
                     dk, dv, ld_grad, M, (int)heads, g.lpr, g.rpw, g.groups, g.waves, g.nblk, g.scale)
  NBR_BY_DEPTH(depth, NBR_BWD)
#undef NBR_BWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
