// Weight fragments: what every MFMA kernel of this library reads its weights as, and the one place that says so.
//
// A fragment is one MFMA operand for a whole wave: 64 lanes x 16 bytes = 1 KiB, lane l holding eight slots j.  A weight image is a
// sequence of fragments; which (slice, level, column block) a fragment belongs to, and in which order they lie, is the business of
// the kernel that reads the image (its *_wprep_kernel or staging loop decodes the block index).  Here: which element of the
// weight matrix a (lane, slot) holds -- the two operand geometries --, how the layer's [Fin K, ld] matrix is gathered with zero
// padding, and how one value is split and stored -- the five forms.  The writers are host-callable (tests/test_wfrag_host.py
// runs them on the CPU against a numpy yardstick); the contraction of a plane row with such fragments follows at the end.
#pragma once

#include "dsphere_common.h"

namespace dsph {

typedef float sp_f32x16 __attribute__((ext_vector_type(16)));
typedef float sp_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 sp_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int WF_FRAG = 1024;   // bytes of one fragment (64 lanes x 16 B)
constexpr int WF_ELEMS = 512;   // (lane, slot) pairs of one fragment: element e = 8 l + j

// The five forms of a stored value.  The first four are the precision codes of include/dsphere.h, so a writer whose kernel reads
// the common form of its precision passes the code itself.
//   WF_FP32_STEPS : float at [j * 64 + l]: step j of v_mfma_f32_32x32x2_f32 reads one float per lane (8 terms of 256 B)
//   WF_FP32_HALVES: float at (j >> 2) * 1024 + l * 16 + (j & 3) * 4: two 1 KiB halves of four floats per lane (the structured kernel)
//   WF_BF16X3     : hi = bf16(v) at [l * 8 + j], lo = bf16(v - hi) one fragment behind; both round to nearest even: hi + lo = v to
//                   16 significant bits
//   WF_BF16X6     : hi | mid | lo, 8 + 8 + 8 significant bits, hi and mid by truncation of v and of v - hi: hi + mid + lo = v exactly
//   WF_F16X3      : hi = f16(v) at [l * 8 + j], lo = f16(v - hi) one fragment behind; round to nearest even: 22 significant bits
//                   while lo is a normal f16, which is the caller's scale rule (qt_wimg_pow2: the largest weight in [2048, 4096))
// Third term of WF_BF16X6: v - hi - mid is exact in fp32 and has at most 8 significant bits, so as long as it is a normal number
// a bf16 holds it exactly and truncation and round-to-nearest give the same 16 bits.  A subnormal remainder (possible from
// |v| < 2^-110 down) can own bits below 2^-133, the last place of a subnormal bf16; there truncation drops them and rounding
// may carry.  The rule, for every writer: the ROUNDING convert, the one wf_split below applies to the plane rows, so both operands
// of a six-term product are split alike.
constexpr int WF_FP32_STEPS = DSPH_PREC_FP32, WF_BF16X3 = DSPH_PREC_BF16X3, WF_BF16X6 = DSPH_PREC_BF16X6, WF_F16X3 = DSPH_PREC_F16X3,
              WF_FP32_HALVES = 4;

// fragments per level of a 16-long slice, and bytes of one: hi | lo (three-term split), hi | mid | lo (six-term), 8 fp32 steps (exact)
__host__ __device__ constexpr int wf_terms(int prec) { return prec == DSPH_PREC_BF16X3 ? 2 : (prec == DSPH_PREC_BF16X6 ? 3 : 8); }
__host__ __device__ constexpr int wf_term_bytes(int prec) { return prec == DSPH_PREC_FP32 ? 256 : WF_FRAG; }

// The operand geometries: element e of a fragment (or of a run of them: e mod 512) is (lane l = e >> 3, slot j = e & 7), and holds the weight at
// (inner index within the slice, column within the block) =
//   32x32x16 / 32x32x2 (wf_elem32): (8 (l >> 5) + j, l & 31) -- a 16-long slice against 32 columns
//   16x16x32           (wf_elem16): (8 (l >> 4) + j, l & 15) -- a 32-long slice against 16 columns
struct WfElem {
  int l, j, inner, col;
};
__host__ __device__ constexpr WfElem wf_elem32(int e) {
  const int l = (e >> 3) & 63, j = e & 7;
  return {l, j, 8 * (l >> 5) + j, l & 31};
}
__host__ __device__ constexpr WfElem wf_elem16(int e) {
  const int l = (e >> 3) & 63, j = e & 7;
  return {l, j, 8 * (l >> 4) + j, l & 15};
}

// The zero-padded gather from the layer's matrix: sc * w[(ch K + k) ld + col], +0 outside [0, Fin) x [0, Fout)
__host__ __device__ __forceinline__ float wf_gather(const float* __restrict__ w, int ch, int col, int Fin, int Fout, int K, int k, int ld,
                                                    float sc = 1.f) {
  return (ch < Fin && col < Fout) ? sc * w[((int64_t)ch * K + k) * ld + col] : 0.f;
}
// pack = P maps per item (the tile kernels' 4 -> 16 and 8 -> 32 layers): one slice and two column blocks, block diagonal -- map q owns
// the inner indices [16 / P q, 16 / P (q + 1)) against the columns [64 / P q, 64 / P (q + 1)); pack = 0: wf_gather
__host__ __device__ __forceinline__ float wf_gather_pack(const float* __restrict__ w, int ch, int col, int Fin, int Fout, int K, int k, int ld,
                                                         int pack) {
  if (!pack) return wf_gather(w, ch, col, Fin, Fout, K, k, ld);
  const int ci = 16 / pack, cm = 64 / pack;
  return ch / ci == col / cm ? wf_gather(w, ch % ci, col % cm, Fin, Fout, K, k, ld) : 0.f;
}

// The element writer: value v of (lane l, slot j) into the fragment(s) at `base`, in the given form
__host__ __device__ __forceinline__ void wf_put(unsigned char* base, int form, int l, int j, float v) {
  if (form == WF_FP32_STEPS) {
    reinterpret_cast<float*>(base)[j * 64 + l] = v;
  } else if (form == WF_FP32_HALVES) {
    reinterpret_cast<float*>(base + (j >> 2) * WF_FRAG)[l * 4 + (j & 3)] = v;
  } else if (form == WF_BF16X3) {
    const __bf16 hi = (__bf16)v;
    reinterpret_cast<__bf16*>(base)[l * 8 + j] = hi;
    reinterpret_cast<__bf16*>(base + WF_FRAG)[l * 8 + j] = (__bf16)(v - (float)hi);
  } else if (form == WF_F16X3) {
    const _Float16 hi = (_Float16)v;
    reinterpret_cast<_Float16*>(base)[l * 8 + j] = hi;
    reinterpret_cast<_Float16*>(base + WF_FRAG)[l * 8 + j] = (_Float16)(v - (float)hi);
  } else {
    const unsigned au = __builtin_bit_cast(unsigned, v);
    const float r = v - __builtin_bit_cast(float, au & 0xffff0000u);
    const unsigned ru = __builtin_bit_cast(unsigned, r);
    reinterpret_cast<unsigned short*>(base)[l * 8 + j] = (unsigned short)(au >> 16);
    reinterpret_cast<unsigned short*>(base + WF_FRAG)[l * 8 + j] = (unsigned short)(ru >> 16);
    reinterpret_cast<__bf16*>(base + 2 * WF_FRAG)[l * 8 + j] = (__bf16)(r - __builtin_bit_cast(float, ru & 0xffff0000u));
  }
}
template <int FORM> __host__ __device__ __forceinline__ void wf_put(unsigned char* base, int l, int j, float v) { wf_put(base, FORM, l, j, v); }

// ---- the contraction of a plane row with the fragments of its level (the input-side strip kernels, cheb_tcontract, patch_gemm) ----

// the B operand(s) of a plane row: 8 inner-index slots per lane, slot j <- channel j of the lane's CH (zero beyond CH)
struct WfFrag {
  sp_bf16x8 t[3];  // hi, lo (three-term) / hi, mid, lo (six-term)
};
template <int CH, int PREC>
__device__ __forceinline__ WfFrag wf_split(const float (&v)[CH]) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  u32x4 w[3] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
  for (int j = 0; j < CH / 2; ++j) {
    const float a0 = v[2 * j], a1 = v[2 * j + 1];
    if (PREC == DSPH_PREC_BF16X3) {
      // per pair: one packed convert for the two hi halves, a shift and a mask to get them back as floats, two subtractions,
      // one packed convert for the lo halves (cheb_strip_kernel.h, xstore)
      const unsigned hu = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a0, a1}, bf16x2));
      const float h0 = __builtin_bit_cast(float, hu << 16), h1 = __builtin_bit_cast(float, hu & 0xffff0000u);
      w[0][j] = hu;
      w[1][j] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a0 - h0, a1 - h1}, bf16x2));
    } else {
      // exact split into 8 + 8 + 8 mantissa bits by truncation (cheb_struct_kernel.h, st_contract): a = h + m + l
      const unsigned u0 = __builtin_bit_cast(unsigned, a0), u1 = __builtin_bit_cast(unsigned, a1);
      const float r0 = a0 - __builtin_bit_cast(float, u0 & 0xffff0000u), r1 = a1 - __builtin_bit_cast(float, u1 & 0xffff0000u);
      const unsigned q0 = __builtin_bit_cast(unsigned, r0), q1 = __builtin_bit_cast(unsigned, r1);
      const float l0 = r0 - __builtin_bit_cast(float, q0 & 0xffff0000u), l1 = r1 - __builtin_bit_cast(float, q1 & 0xffff0000u);
      w[0][j] = (u0 >> 16) | (u1 & 0xffff0000u);
      w[1][j] = (q0 >> 16) | (q1 & 0xffff0000u);
      w[2][j] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{l0, l1}, bf16x2));  // (at most 8 significant bits left: exact)
    }
  }
  WfFrag f;
#pragma unroll
  for (int t = 0; t < 3; ++t) f.t[t] = __builtin_bit_cast(sp_bf16x8, w[t]);
  return f;
}

// acc (+)= W_level . row: the contraction of one plane row with the weights of its level
template <int CH, int PREC, bool INIT>
__device__ __forceinline__ void wf_contract(sp_f32x16& acc, const float (&row)[CH], const unsigned char* __restrict__ wlev, int lane) {
  if (INIT) {
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.f;
  }
  if (PREC == DSPH_PREC_FP32) {
    // v_mfma_f32_32x32x2_f32: inner index = 2 s + (lane >> 5); the lane's operand of step s is slot j = s of the OTHER layout,
    // so the eight steps walk the lane's eight slots: step s contracts channels {slot s of half 0, slot s of half 1}
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      const float b = row[s];
      const float wa = *reinterpret_cast<const float*>(wlev + s * 256 + lane * 4);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, b, acc, 0, 0, 0);
    }
    return;
  }
  const WfFrag f = wf_split<CH, PREC>(row);
  const sp_bf16x8 w0 = *reinterpret_cast<const sp_bf16x8*>(wlev + lane * 16);
  const sp_bf16x8 w1 = *reinterpret_cast<const sp_bf16x8*>(wlev + 1024 + lane * 16);
  if (PREC == DSPH_PREC_BF16X3) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, f.t[1], acc, 0, 0, 0);  // small terms first
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, f.t[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, f.t[0], acc, 0, 0, 0);
  } else {
    const sp_bf16x8 w2 = *reinterpret_cast<const sp_bf16x8*>(wlev + 2048 + lane * 16);
    // the six products down to 2^-16: hl, lh, mm, hm, mh, hh (w index first)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, f.t[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, f.t[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, f.t[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, f.t[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, f.t[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, f.t[0], acc, 0, 0, 0);
  }
}

}  // namespace dsph
